"""-m gpu: the device-resident greedy evaluation on the MI355X -- dtqn_deval_* entry points, DeviceEvaluator and
`run.py --device-eval-envs N` (device_eval_helpers.py; the same checks run on the HIP emulation in test_emu_device_eval.py)."""
import pytest

import device_eval_helpers as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("kind,shape,row_block", [("car", R.WHOLE, False), ("car", R.ROWBLOCK, True), ("mem", R.WHOLE, False)],
                         ids=["carflag-whole-sequence", "carflag-row-block", "memory-whole-sequence"])
def test_every_step_equals_the_host_environment_context_and_forward(lib, kind, shape, row_block):
    R.check_step_parity(None, "cuda", kind, shape, row_block)


@pytest.mark.parametrize("kind", ["car", "mem"])
def test_episodes_do_not_depend_on_the_number_of_environments(lib, kind):
    R.check_independent_of_n(None, "cuda", kind)


@pytest.mark.parametrize("kind", ["car", "mem"])
def test_quota_is_exact_and_the_triple_follows_run_evaluate(lib, kind):
    R.check_quota(None, "cuda", kind)


def test_an_evaluation_moves_nothing_else(lib):
    R.check_nothing_else_moves(None, "cuda")


def test_a_dropout_network_evaluates_like_its_dropout_free_twin(lib):
    R.check_dropout_is_off(None, "cuda")


def test_run_py_device_eval_envs_end_to_end(lib, monkeypatch, tmp_path):
    R.check_run_py(None, "cuda", monkeypatch, tmp_path)


def test_refusals(lib):
    R.check_refusals(None, "cuda")
