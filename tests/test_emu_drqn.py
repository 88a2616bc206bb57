"""DRQN baseline on the CPU emulation of the kernels: C ABI, module, agent, run.py and the resource table (docs/drqn_tests.md)."""
import ctypes
import glob
import json
import os

import numpy as np
import pytest
import torch

import drqn_helpers as H
from dtqn_amd import _binding as B

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    lib = B.load_library(emu_build.build())
    yield lib
    H.write_report()


# d_model 64: weight_hh stays in registers for the scan; 128: streamed every step.  B 3: one 16-sequence workgroup; 17: a second one
@pytest.mark.parametrize("lens_kind", ["ones", "full", "mix"])
@pytest.mark.parametrize("discrete", [False, True], ids=["cont", "disc"])
@pytest.mark.parametrize("Bn", [3, 17])
@pytest.mark.parametrize("d", [64, 128])
def test_kernels_match_the_oracle(emu, d, Bn, discrete, lens_kind):
    H.check_kernels(emu, "cpu", d, Bn, 7, discrete, lens_kind, seed=d + Bn)


def test_net_init_scope(emu):
    for d in (64, 128, 256):
        net = B.make_drqn_net(emu, obs_dim=3, num_actions=3, inner_embed=d, context_len=512)
        assert net.kep == 4 and net.ap == 4 and net.n_trainable == net.n_theta and net.n_theta % 4 == 0
        offs = [off for off, _ in B.drqn_param_table(net).values()]
        assert all(o % 4 == 0 for o in offs) and len(set(offs)) == len(offs)
    net = B.make_drqn_net(emu, obs_dim=128, num_actions=3, embed_per_obs_dim=8, inner_embed=64, context_len=50, discrete=True, vocab_sizes=64)
    assert net.ke == 1024 and net.off_obs_tab == 0
    assert B.make_drqn_net(emu, obs_dim=3, num_actions=3, action_dim=4, inner_embed=64).action_dim == 4          # accepted, unused
    for bad in (dict(inner_embed=48), dict(inner_embed=32), dict(context_len=513), dict(context_len=0), dict(num_actions=65),
                dict(obs_dim=129, discrete=True, vocab_sizes=4), dict(obs_dim=3, embed_per_obs_dim=8, discrete=True, vocab_sizes=8193),
                dict(obs_dim=(3, 24, 24))):
        with pytest.raises(NotImplementedError):
            B.make_drqn_net(emu, **{**dict(obs_dim=3, num_actions=3, inner_embed=64, context_len=50), **bad})
    net = B.make_drqn_net(emu, obs_dim=3, num_actions=3, inner_embed=64, context_len=8)
    assert emu.dtqn_drqn_workspace_floats(ctypes.byref(net), 2, 9, 0) == 0            # more rows than the context
    assert emu.dtqn_drqn_workspace_floats(ctypes.byref(net), 2, 8, 1) > emu.dtqn_drqn_workspace_floats(ctypes.byref(net), 2, 8, 0) > 0


@pytest.mark.parametrize("discrete", [False, True], ids=["cont", "disc"])
@pytest.mark.parametrize("d", [64, 128])
def test_module_surface(emu, d, discrete):
    H.check_module(emu, "cpu", d, discrete)


def test_module_refuses_what_it_cannot_run(emu):
    from dtqn_amd import engine
    from dtqn_amd.networks import DRQN
    m = DRQN(3, 3, 8, 0, 64, False, _test_lib=emu)
    with pytest.raises(engine.EngineUnavailable):                # no eager fall-back
        m(torch.zeros(1, 2, 3), None, episode_lengths=torch.tensor([2]))
    m._allow_cpu = True
    with pytest.raises(ValueError):
        m(torch.zeros(1, 2, 3), None)
    with pytest.raises(RuntimeError):
        m(torch.zeros(2, 2, 3), None, episode_lengths=torch.tensor([2, 0]))
    with pytest.raises(NotImplementedError):
        DRQN((3, 24, 24), 3, 8, 0, 64, False, _test_lib=emu)


@pytest.mark.parametrize("discrete", [False, True], ids=["cont", "disc"])
def test_agent_updates_match_the_oracle_learner(emu, monkeypatch, discrete):
    H.check_agent_updates(emu, "cpu", monkeypatch, discrete)


@pytest.mark.parametrize("discrete", [False, True], ids=["cont", "disc"])
def test_get_action_actions_and_exploration_stream(emu, monkeypatch, discrete):
    H.check_get_action(emu, "cpu", monkeypatch, discrete)


def test_checkpoint_round_trip(emu, monkeypatch, tmp_path):
    H.check_checkpoint(emu, "cpu", monkeypatch, tmp_path)


def test_nonfinite_norm_raises(emu, monkeypatch):
    H.check_nonfinite(emu, "cpu", monkeypatch)


def _patch_run(emu, monkeypatch, tmp_path):
    import run as runpy
    from dtqn_amd.networks.drqn import DRQN
    from dtqn_amd.utils import agent_utils

    def emu_drqn(*a, **k):
        m = DRQN(*a, _test_lib=emu, **k)
        m._allow_cpu = True
        return m
    monkeypatch.setitem(agent_utils.MODEL_MAP, "DRQN", emu_drqn)
    monkeypatch.chdir(tmp_path)
    return runpy


RUN = "--model DRQN --in-embed 64 --context 8 --num-steps 60 --prepopulate 200 --disable-wandb --device cpu --buf-size 4000 --batch 1"


def test_run_py_trains_drqn(emu, monkeypatch, tmp_path):
    runpy = _patch_run(emu, monkeypatch, tmp_path)
    agent = runpy.run_experiment(runpy.get_args((RUN + " --project-name drqn").split()))
    assert type(agent).__name__ == "DrqnAgent" and agent.num_train_steps > 0
    assert len(glob.glob(str(tmp_path / "policies" / "drqn" / "**" / "*_mini_checkpoint.pt"), recursive=True)) == 1
    assert np.isfinite(agent.td_errors.mean())


@pytest.mark.parametrize("switch", ["--num-envs 2", "--eval-envs 2", "--device-envs 2", "--device-eval-envs 2", "--device-bag-eval-envs 2",
                                    "--overlap", "--bag-size 4", "--sampler device"])
def test_run_py_names_the_switch_it_excludes(emu, monkeypatch, tmp_path, switch):
    runpy = _patch_run(emu, monkeypatch, tmp_path)
    with pytest.raises(NotImplementedError, match=switch.split()[0] if switch != "--sampler device" else "--sampler device"):
        runpy.run_experiment(runpy.get_args((RUN + " --project-name refused " + switch).split()))


def test_run_py_excludes_data_parallel_drqn(emu, monkeypatch, tmp_path):
    runpy = _patch_run(emu, monkeypatch, tmp_path)
    monkeypatch.setattr(runpy.ddp, "init_from_env", lambda *a, **k: (0, 2, 0))
    with pytest.raises(NotImplementedError, match="world size"):
        runpy.run_experiment(runpy.get_args((RUN + " --project-name refused").split()))


def test_kernels_are_in_the_resource_table_inside_the_default_budget():
    from dtqn_amd import build as Bd
    path = Bd.resources_path()
    stale = True
    if os.path.exists(path):
        with open(path) as f:
            stale = json.load(f).get("src", "").split("+")[0] != Bd._digest()
    if stale:
        Bd.build()
    with open(path) as f:
        kernels = {k: v for k, v in json.load(f)["kernels"].items() if v.get("source") == "dtqn_drqn.hip"}
    with open(os.path.join(HERE, "kernel_budget.json")) as f:
        limit = json.load(f)["default_scratch_max"]
    names = " ".join(kernels)
    for want in ("drqn_gemm_kernel", "drqn_colsum_kernel", "drqn_gather_kernel", "drqn_table_grad_kernel"):
        assert want in names
    for d in (64, 128, 256):                     # (Itanium mangling: ILi<D>E...)
        assert sum(f"drqn_scan_kernelILi{d}E" in k for k in kernels) == 2 and sum(f"drqn_bptt_kernelILi{d}E" in k for k in kernels) == 1
    for k, v in kernels.items():
        assert v["scratch"] <= limit, (k, v)
