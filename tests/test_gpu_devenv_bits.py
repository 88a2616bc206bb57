"""-m gpu: the shared device-environment layer on the MI355X -- the epsilon = 1 rollout (no forward) produces the state, replay and
status bytes the commit before that layer produced on this back-end, and a NaN in a Q row is the rollout's arg-max
(devenv_bits_helpers.py; the emulation runs both scenarios, with the evaluation, in test_emu_devenv_bits.py)."""
import pytest

import devenv_bits_helpers as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


def test_epsilon_1_rollout_bytes_equal_the_parent_commit(lib):
    H.check_against_fixture(None, "cuda", "eps1", H.ROLLOUT_KEYS)


def test_a_nan_q_value_is_the_rollouts_argmax(lib):
    H.nan_argmax_case(None, "cuda")
