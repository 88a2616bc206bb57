"""DRQN baseline through the gfx950 library on the device: the kernel, module and agent cases of tests/test_emu_drqn.py at the same sizes,
and one case at d_model 256, L 50, B 32 for the forward and the gradients (docs/drqn_tests.md)."""
import glob

import numpy as np
import pytest

import drqn_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    yield engine.get_lib()
    H.write_report()


@pytest.mark.parametrize("lens_kind", ["ones", "full", "mix"])
@pytest.mark.parametrize("discrete", [False, True], ids=["cont", "disc"])
@pytest.mark.parametrize("Bn", [3, 17])
@pytest.mark.parametrize("d", [64, 128])
def test_kernels_match_the_oracle(lib, d, Bn, discrete, lens_kind):
    H.check_kernels(lib, DEV, d, Bn, 7, discrete, lens_kind, seed=d + Bn)


@pytest.mark.parametrize("discrete", [False, True], ids=["cont", "disc"])
def test_forward_and_gradients_at_d256_l50_b32(lib, discrete):
    H.check_kernels(lib, DEV, 256, 32, 50, discrete, "mix", seed=256, steps=False)


@pytest.mark.parametrize("discrete", [False, True], ids=["cont", "disc"])
@pytest.mark.parametrize("d", [64, 128])
def test_module_surface(lib, d, discrete):
    H.check_module(None, DEV, d, discrete)


@pytest.mark.parametrize("discrete", [False, True], ids=["cont", "disc"])
def test_agent_updates_match_the_oracle_learner(lib, monkeypatch, discrete):
    H.check_agent_updates(None, DEV, monkeypatch, discrete)


@pytest.mark.parametrize("discrete", [False, True], ids=["cont", "disc"])
def test_get_action_actions_and_exploration_stream(lib, monkeypatch, discrete):
    H.check_get_action(None, DEV, monkeypatch, discrete)


def test_checkpoint_round_trip(lib, monkeypatch, tmp_path):
    H.check_checkpoint(None, DEV, monkeypatch, tmp_path)


def test_nonfinite_norm_raises(lib, monkeypatch):
    H.check_nonfinite(None, DEV, monkeypatch)


def test_run_py_trains_drqn_on_carflag(lib, monkeypatch, tmp_path):
    import run as runpy
    monkeypatch.chdir(tmp_path)
    args = "--model DRQN --in-embed 64 --context 8 --num-steps 60 --prepopulate 200 --disable-wandb --buf-size 4000 --batch 1 --project-name drqn"
    agent = runpy.run_experiment(runpy.get_args(args.split()))
    assert type(agent).__name__ == "DrqnAgent" and agent.num_train_steps > 0 and np.isfinite(agent.td_errors.mean())
    assert len(glob.glob(str(tmp_path / "policies" / "drqn" / "**" / "*_mini_checkpoint.pt"), recursive=True)) == 1
