"""-m gpu: the device-resident greedy evaluation of a bag network on the MI355X -- the candidate forward on a shared trunk
(dtqn_forward_bag_candidates), the dtqn_deval_*_bag entry points, DeviceBagEvaluator and `run.py --bag-size K --device-bag-eval-envs N`
(device_bag_eval_helpers.py; the same checks run on the HIP emulation in test_emu_device_bag_eval.py)."""
import pytest

import device_bag_eval_helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("case", list(H.CANDIDATE_CASES))
def test_candidate_forward_equals_the_bag_forward_on_tiled_inputs(lib, case, capfd, monkeypatch):
    H.check_candidate_forward(None, "cuda", case, capfd, monkeypatch)


@pytest.mark.parametrize("kind", ["car", "mem", "tiger"], ids=["carflag", "memory", "pomdp-tiger"])
def test_step_parity_with_the_host_context_and_bag(lib, kind):
    H.check_step_parity(None, "cuda", kind)


def test_may_choose_is_the_rollouts_rule(lib):
    H.check_may_choose(None, "cuda")


def test_episodes_and_bag_choices_do_not_depend_on_n(lib):
    H.check_independent_of_n(None, "cuda")


def test_an_evaluation_moves_nothing_else(lib):
    H.check_nothing_else_moves(None, "cuda")


def test_dropout_network_evaluates_as_its_dropout_free_twin(lib):
    H.check_dropout_is_off(None, "cuda")


def test_run_py_device_bag_eval_envs_end_to_end(lib, monkeypatch, tmp_path):
    H.check_run_py(None, "cuda", monkeypatch, tmp_path)


def test_refusals(lib):
    H.check_refusals(None, "cuda")
