"""The device-resident greedy evaluation on the test-only HIP emulation: dtqn_deval_* entry points, DeviceEvaluator and
`run.py --device-eval-envs N` (device_eval_helpers.py; the MI355X runs the same checks in test_gpu_device_eval.py)."""
import pytest

from dtqn_amd import _binding as B

import device_eval_helpers as R


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.mark.parametrize("kind,shape,row_block", [("car", R.WHOLE, False), ("car", R.ROWBLOCK, True), ("mem", R.WHOLE, False)],
                         ids=["carflag-whole-sequence", "carflag-row-block", "memory-whole-sequence"])
def test_every_step_equals_the_host_environment_context_and_forward(emu, kind, shape, row_block):
    R.check_step_parity(emu, "cpu", kind, shape, row_block)


@pytest.mark.parametrize("kind", ["car", "mem"])
def test_episodes_do_not_depend_on_the_number_of_environments(emu, kind):
    R.check_independent_of_n(emu, "cpu", kind)


@pytest.mark.parametrize("kind", ["car", "mem"])
def test_quota_is_exact_and_the_triple_follows_run_evaluate(emu, kind):
    R.check_quota(emu, "cpu", kind)


def test_an_evaluation_moves_nothing_else(emu):
    R.check_nothing_else_moves(emu, "cpu")


def test_a_dropout_network_evaluates_like_its_dropout_free_twin(emu):
    R.check_dropout_is_off(emu, "cpu")


def test_run_py_device_eval_envs_end_to_end(emu, monkeypatch, tmp_path):
    R.check_run_py(emu, "cpu", monkeypatch, tmp_path)


def test_refusals(emu):
    R.check_refusals(emu, "cpu")
