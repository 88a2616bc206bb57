"""-m gpu: the device-resident rollout of a bag network on the MI355X -- dtqn_devbag_* kernels, the dtqn_rollout_*_bag entry points,
DeviceBagVectorActor and `run.py --bag-size K --device-envs N` (device_bag_helpers.py; the same checks run on the HIP emulation in
test_emu_device_bag.py)."""
import pytest

import device_bag_helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("kind,a_embed", [("car", 0), ("car", 4), ("mem", 0), ("tiger", 0)],
                         ids=["carflag", "carflag-a-embed-4", "memory", "pomdp-tiger-listen"])
def test_bag_bookkeeping_equals_the_host_context_and_bag(lib, kind, a_embed):
    H.check_bookkeeping(None, "cuda", kind, a_embed=a_embed)


def test_scores_equal_the_host_forward_and_choices_are_the_first_arg_max(lib):
    H.check_scores_and_choice(None, "cuda")


def test_acting_uses_the_bag(lib):
    H.check_acting_uses_the_bag(None, "cuda")


def test_ragged_phases(lib):
    H.check_ragged_phases(None, "cuda")


def test_same_seed_same_state_bytes(lib):
    H.check_determinism(None, "cuda")


def test_replay_and_accounting(lib):
    H.check_replay_and_accounting(None, "cuda")


def test_run_py_bag_device_envs_end_to_end(lib, monkeypatch, tmp_path):
    H.check_run_py(None, "cuda", monkeypatch, tmp_path)


def test_refusals(lib):
    H.check_refusals(None, "cuda")
