"""The device-resident greedy evaluation of a bag network on the test-only HIP emulation: the candidate forward on a shared trunk
(dtqn_forward_bag_candidates), the dtqn_deval_*_bag entry points, DeviceBagEvaluator and `run.py --bag-size K --device-bag-eval-envs N`
(device_bag_eval_helpers.py; the MI355X runs the same checks in test_gpu_device_bag_eval.py)."""
import pytest

from dtqn_amd import _binding as B

import device_bag_eval_helpers as H


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.mark.parametrize("case", list(H.CANDIDATE_CASES))
def test_candidate_forward_equals_the_bag_forward_on_tiled_inputs(emu, case, capfd, monkeypatch):
    H.check_candidate_forward(emu, "cpu", case, capfd, monkeypatch)


@pytest.mark.parametrize("kind", ["car", "mem", "tiger"], ids=["carflag", "memory", "pomdp-tiger"])
def test_step_parity_with_the_host_context_and_bag(emu, kind):
    H.check_step_parity(emu, "cpu", kind)


def test_may_choose_is_the_rollouts_rule(emu):
    H.check_may_choose(emu, "cpu")


def test_episodes_and_bag_choices_do_not_depend_on_n(emu):
    H.check_independent_of_n(emu, "cpu")


def test_an_evaluation_moves_nothing_else(emu):
    H.check_nothing_else_moves(emu, "cpu")


def test_dropout_network_evaluates_as_its_dropout_free_twin(emu):
    H.check_dropout_is_off(emu, "cpu")


def test_run_py_device_bag_eval_envs_end_to_end(emu, monkeypatch, tmp_path):
    H.check_run_py(emu, "cpu", monkeypatch, tmp_path)


def test_refusals(emu):
    H.check_refusals(emu, "cpu")
