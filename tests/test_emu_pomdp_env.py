"""The tabular POMDP environment kind of the device-resident rollout and evaluation on the test-only HIP emulation: the dtqn_rollout_* /
dtqn_deval_* entry points with DTQN_ROLLOUT_POMDP, DeviceVectorActor, DeviceEvaluator and run.py on POMDP ids and `.pomdp` paths
(pomdp_env_helpers.py; the MI355X runs the same checks in test_gpu_pomdp_env.py)."""
import pytest

from dtqn_amd import _binding as B

import pomdp_env_helpers as R

SHAPES = pytest.mark.parametrize("shape,row_block", [(R.WHOLE, False), (R.ROWBLOCK, True)], ids=["whole-sequence", "row-block"])


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


def test_dynamics_bit_exact_against_the_host_environment(emu):
    R.check_dynamics(emu, "cpu")


def test_draw_statistics(emu):
    R.check_draw_statistics(emu, "cpu")


@SHAPES
def test_replay_equals_the_host_producer_and_store_0_leaves_it_alone(emu, shape, row_block):
    R.check_replay_parity(emu, "cpu", shape, row_block)


@SHAPES
def test_contexts_q_rows_and_greedy_actions_equal_the_host_staged_forward(emu, shape, row_block):
    R.check_context_and_action_parity(emu, "cpu", shape, row_block)


def test_evaluation_results_do_not_depend_on_the_number_of_environments(emu):
    R.check_eval_independent_of_n(emu, "cpu")


def test_evaluation_steps_equal_the_host_environment(emu):
    R.check_eval_step_parity(emu, "cpu")


def test_run_py_on_pomdp_ids_and_paths_end_to_end(emu, monkeypatch, tmp_path):
    R.check_run_py(emu, "cpu", monkeypatch, tmp_path)


def test_refusals(emu):
    R.check_refusals(emu, "cpu")
