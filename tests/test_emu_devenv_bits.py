"""The shared device-environment layer (csrc/dtqn_devenv.hpp, agents/device_env.py) on the test-only HIP emulation: the rollout and
the evaluation produce the bytes the commit before that layer produced (devenv_bits_helpers.py, tests/golden/devenv_parent_bits.npz),
and a NaN in a Q row is the rollout's arg-max as it is torch.argmax's.  The MI355X runs its part in test_gpu_devenv_bits.py."""
import pytest

from dtqn_amd import _binding as B

import devenv_bits_helpers as H


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.mark.parametrize("eps_name", sorted(H.EPSILONS))
def test_rollout_and_evaluation_bytes_equal_the_parent_commit(emu, eps_name):
    H.check_against_fixture(emu, "cpu", eps_name, H.ROLLOUT_KEYS + H.EVAL_KEYS)


def test_a_nan_q_value_is_the_rollouts_argmax(emu):
    H.nan_argmax_case(emu, "cpu")
