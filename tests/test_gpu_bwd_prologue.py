"""-m gpu: the prologue of the four-slice backward chain (loss rows loaded unconditionally in front of the prefetch batch, every dq row
written by the loss wave itself, head.2 staged through LDS) on the MI355X, as the pipelined update runs it -- the device half of
tests/test_emu_bwd_prologue.py, which describes the cases.  Batch 2 - 3, one or two updates each; values are compared, nothing else."""
import pytest

from test_emu_bwd_prologue import CASES, run_case, run_ties, run_nan_rewards

pytestmark = pytest.mark.gpu

GPU = dict(device="cuda", test_lib=False)


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("name", sorted(CASES))
def test_prologue_paths_vs_oracle(lib, name):
    run_case(lib, name, **GPU)


def test_exact_ties_take_the_first_maximum(lib):
    run_ties(lib, **GPU)


def test_nan_rewards_behind_every_episode_change_no_bit(lib):
    run_nan_rewards(lib, **GPU)
