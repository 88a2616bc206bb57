"""The device-resident rollout of a bag network on the test-only HIP emulation: dtqn_devbag_* kernels, the dtqn_rollout_*_bag entry
points, DeviceBagVectorActor and `run.py --bag-size K --device-envs N` (device_bag_helpers.py; the MI355X runs the same checks in
test_gpu_device_bag.py)."""
import pytest

from dtqn_amd import _binding as B

import device_bag_helpers as H


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.mark.parametrize("kind,a_embed", [("car", 0), ("car", 4), ("mem", 0), ("tiger", 0)],
                         ids=["carflag", "carflag-a-embed-4", "memory", "pomdp-tiger-listen"])
def test_bag_bookkeeping_equals_the_host_context_and_bag(emu, kind, a_embed):
    H.check_bookkeeping(emu, "cpu", kind, a_embed=a_embed)


def test_scores_equal_the_host_forward_and_choices_are_the_first_arg_max(emu):
    H.check_scores_and_choice(emu, "cpu")


def test_acting_uses_the_bag(emu):
    H.check_acting_uses_the_bag(emu, "cpu")


def test_ragged_phases(emu):
    H.check_ragged_phases(emu, "cpu")


def test_same_seed_same_state_bytes(emu):
    H.check_determinism(emu, "cpu")


def test_replay_and_accounting(emu):
    H.check_replay_and_accounting(emu, "cpu")


def test_run_py_bag_device_envs_end_to_end(emu, monkeypatch, tmp_path):
    H.check_run_py(emu, "cpu", monkeypatch, tmp_path)


def test_refusals(emu):
    H.check_refusals(emu, "cpu")
