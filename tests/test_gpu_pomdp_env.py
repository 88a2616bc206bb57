"""-m gpu: the tabular POMDP environment kind of the device-resident rollout and evaluation on the MI355X -- the dtqn_rollout_* /
dtqn_deval_* entry points with DTQN_ROLLOUT_POMDP, DeviceVectorActor, DeviceEvaluator and run.py on POMDP ids and `.pomdp` paths
(pomdp_env_helpers.py; the same checks run on the HIP emulation in test_emu_pomdp_env.py)."""
import pytest

import pomdp_env_helpers as R

pytestmark = pytest.mark.gpu

SHAPES = pytest.mark.parametrize("shape,row_block", [(R.WHOLE, False), (R.ROWBLOCK, True)], ids=["whole-sequence", "row-block"])


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


def test_dynamics_bit_exact_against_the_host_environment(lib):
    R.check_dynamics(None, "cuda")


def test_draw_statistics(lib):
    R.check_draw_statistics(None, "cuda")


@SHAPES
def test_replay_equals_the_host_producer_and_store_0_leaves_it_alone(lib, shape, row_block):
    R.check_replay_parity(None, "cuda", shape, row_block)


@SHAPES
def test_contexts_q_rows_and_greedy_actions_equal_the_host_staged_forward(lib, shape, row_block):
    R.check_context_and_action_parity(None, "cuda", shape, row_block)


def test_evaluation_results_do_not_depend_on_the_number_of_environments(lib):
    R.check_eval_independent_of_n(None, "cuda")


def test_evaluation_steps_equal_the_host_environment(lib):
    R.check_eval_step_parity(None, "cuda")


def test_run_py_on_pomdp_ids_and_paths_end_to_end(lib, monkeypatch, tmp_path):
    R.check_run_py(None, "cuda", monkeypatch, tmp_path)


def test_refusals(lib):
    R.check_refusals(None, "cuda")
