"""-m gpu: the device-resident rollout on the MI355X -- dtqn_rollout_* entry points, DeviceVectorActor and `run.py --device-envs N`
(device_rollout_helpers.py; the same checks run on the HIP emulation in test_emu_device_rollout.py)."""
import pytest

import device_rollout_helpers as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


def test_carflag_dynamics_bit_exact_against_the_host_environment(lib):
    R.check_carflag_dynamics(None, "cuda")


def test_memory_dynamics_bit_exact_against_the_host_environment(lib):
    R.check_memory_dynamics(None, "cuda")


@pytest.mark.parametrize("kind", ["car", "mem"])
def test_replay_equals_the_host_producer_and_store_0_leaves_it_alone(lib, kind):
    R.check_replay_parity(None, "cuda", kind)


@pytest.mark.parametrize("kind,shape,row_block", [("car", R.WHOLE, False), ("car", R.ROWBLOCK, True), ("mem", R.WHOLE, False)],
                         ids=["carflag-whole-sequence", "carflag-row-block", "memory-whole-sequence"])
def test_contexts_q_rows_and_greedy_actions_equal_the_host_staged_forward(lib, kind, shape, row_block):
    R.check_context_and_action_parity(None, "cuda", kind, shape, row_block)


def test_exploration_draws(lib):
    R.check_exploration(None, "cuda")


def test_run_py_device_envs_end_to_end(lib, monkeypatch, tmp_path):
    R.check_run_py(None, "cuda", monkeypatch, tmp_path)


def test_checkpoint_after_sync_round_trips(lib, tmp_path):
    R.check_checkpoint_round_trip(None, "cuda", tmp_path)


def test_refusals(lib):
    R.check_refusals(None, "cuda")
