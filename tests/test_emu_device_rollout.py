"""The device-resident rollout on the test-only HIP emulation: dtqn_rollout_* entry points, DeviceVectorActor and
`run.py --device-envs N` (device_rollout_helpers.py; the MI355X runs the same checks in test_gpu_device_rollout.py)."""
import pytest

from dtqn_amd import _binding as B

import device_rollout_helpers as R


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


def test_carflag_dynamics_bit_exact_against_the_host_environment(emu):
    R.check_carflag_dynamics(emu, "cpu")


def test_memory_dynamics_bit_exact_against_the_host_environment(emu):
    R.check_memory_dynamics(emu, "cpu")


@pytest.mark.parametrize("kind", ["car", "mem"])
def test_replay_equals_the_host_producer_and_store_0_leaves_it_alone(emu, kind):
    R.check_replay_parity(emu, "cpu", kind)


@pytest.mark.parametrize("kind,shape,row_block", [("car", R.WHOLE, False), ("car", R.ROWBLOCK, True), ("mem", R.WHOLE, False)],
                         ids=["carflag-whole-sequence", "carflag-row-block", "memory-whole-sequence"])
def test_contexts_q_rows_and_greedy_actions_equal_the_host_staged_forward(emu, kind, shape, row_block):
    R.check_context_and_action_parity(emu, "cpu", kind, shape, row_block)


def test_exploration_draws(emu):
    R.check_exploration(emu, "cpu")


def test_run_py_device_envs_end_to_end(emu, monkeypatch, tmp_path):
    R.check_run_py(emu, "cpu", monkeypatch, tmp_path)


def test_checkpoint_after_sync_round_trips(emu, tmp_path):
    R.check_checkpoint_round_trip(emu, "cpu", tmp_path)


def test_refusals(emu):
    R.check_refusals(emu, "cpu")
