"""-m gpu: HIP forward (through the C ABI) vs the CPU oracle and the reference's golden vectors."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from dtqn_amd import _binding as B
from oracle import dtqn_oracle as O

from conftest import GOLDEN
from helpers import net_from_cfg, pack_theta, ptr
from q_f64_helpers import check_forward_f64, check_pooled_f64

pytestmark = pytest.mark.gpu

Q_TOL = 1e-4   # north_star: per-timestep Q-values within 1e-4 fp32: ABSOLUTE for G1 / G4 (the metric configuration, the reference's own numbers);
               # the synthetic std-0.2 stress fixtures (G2 variants, G3: |Q| up to 3e2) scale it by |Q|max, see tests/helpers.py


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


def hip_forward(lib, cfg, params, obs, act):
    from dtqn_amd import engine
    net = net_from_cfg(lib, cfg)
    dev = torch.device("cuda")
    theta = torch.from_numpy(pack_theta(net, params)).to(dev)
    Bn, n = obs.shape[:2]
    obs_d = torch.as_tensor(np.ascontiguousarray(obs, dtype=np.float32)).to(dev)
    act_d = torch.as_tensor(np.ascontiguousarray(act.reshape(Bn, n), dtype=np.uint8)).to(dev)
    q = torch.full((Bn, n, cfg.num_actions), float("nan"), device=dev)
    if net.tiled:
        ws = torch.empty(lib.dtqn_forward_workspace_floats(ctypes.byref(net), Bn), device=dev)
        rc = lib.dtqn_forward_tiled(ctypes.byref(net), ptr(theta), ptr(obs_d), ptr(act_d), Bn, n, ptr(q), ptr(ws), engine.stream_ptr())
    else:
        rc = lib.dtqn_forward(ctypes.byref(net), ptr(theta), ptr(obs_d), ptr(act_d), Bn, n, ptr(q), engine.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return q.cpu().numpy()


def test_golden_G4_actor_variable_length(lib):
    z = np.load(os.path.join(GOLDEN, "G4_actor_varlen.npz"))
    for tag in ("res", "gru_a8_sin"):          # residual gate; GRU gate + action embedding + sinusoidal encodings
        cfg = O.NetCfg(**json.loads(str(z[f"{tag}/cfg"])))
        params = O.init_params(cfg, seed=41, perturb=True)
        pool = []              # the float64 check: one yardstick over the rows of every prefix length
        for n in (1, 2, 17, 50):
            got = hip_forward(lib, cfg, params, z[f"{tag}/n{n}_obs"], z[f"{tag}/n{n}_act"])
            ref = z[f"{tag}/n{n}_q"]
            assert np.abs(got - ref).max() <= Q_TOL * max(1.0, np.abs(ref).max()), (tag, n)
            check_forward_f64(cfg, params, z[f"{tag}/n{n}_obs"], z[f"{tag}/n{n}_act"], got, what=("G4", tag, n), pool=pool)
        check_pooled_f64(pool)


def test_golden_G1_q_values(lib):
    z = np.load(os.path.join(GOLDEN, "G1_cfg1_td.npz"))
    cfg = O.NetCfg(**json.loads(str(z["cfg"])))
    seed = int(z["seed"])
    pol = O.init_params(cfg, seed=seed, perturb=True)
    tgt = O.init_params(cfg, seed=seed + 1, perturb=True)
    scale = 1.0          # absolute tolerance
    got = hip_forward(lib, cfg, pol, z["batch0_obss"], z["batch0_actions"])
    assert np.abs(got - z["q_all"]).max() <= Q_TOL * scale
    check_forward_f64(cfg, pol, z["batch0_obss"], z["batch0_actions"], got, what=("G1", "q_all"))
    got = hip_forward(lib, cfg, pol, z["batch0_next_obss"], z["batch0_next_actions"])
    assert np.abs(got - z["q_next_pol"]).max() <= Q_TOL * scale
    check_forward_f64(cfg, pol, z["batch0_next_obss"], z["batch0_next_actions"], got, what=("G1", "q_next_pol"))
    got = hip_forward(lib, cfg, tgt, z["batch0_next_obss"], z["batch0_next_actions"])
    assert np.abs(got - z["q_next_tgt"]).max() <= Q_TOL * scale
    check_forward_f64(cfg, tgt, z["batch0_next_obss"], z["batch0_next_actions"], got, what=("G1", "q_next_tgt"))


def test_golden_G3_cfg345_q_values(lib):
    """BASELINE configs 3, 4, 5 at their full network sizes (D=128/L=50, D=128/L=128, D=256/L=256) against the
    Q-values the reference produced; cfg 3 runs on the whole-sequence kernels, cfg 4 and 5 on the tiled path."""
    z = np.load(os.path.join(GOLDEN, "G3_cfg345_td.npz"))
    for name in json.loads(str(z["names"])):
        p = name + "/"
        cfg = O.NetCfg(**json.loads(str(z[p + "cfg"])))
        seed = int(z[p + "seed"])
        pol = O.init_params(cfg, seed=seed, perturb=True)
        tgt = O.init_params(cfg, seed=seed + 1, perturb=True)
        scale = max(1.0, np.abs(z[p + "q_all"]).max())
        for params, obs_k, act_k, q_k in ((pol, "batch0_obss", "batch0_actions", "q_all"),
                                          (pol, "batch0_next_obss", "batch0_next_actions", "q_next_pol"),
                                          (tgt, "batch0_next_obss", "batch0_next_actions", "q_next_tgt")):
            got = hip_forward(lib, cfg, params, z[p + obs_k], z[p + act_k])
            err = np.abs(got - z[p + q_k]).max()
            assert err <= Q_TOL * scale, (name, q_k, err, scale)
            check_forward_f64(cfg, params, z[p + obs_k], z[p + act_k], got, what=("G3", name, q_k))


VARIANTS = [
    dict(obs_dim=3, num_actions=3, inner_embed_size=16, num_heads=2, history_len=8),
    dict(obs_dim=3, num_actions=4, inner_embed_size=32, num_heads=4, history_len=20, action_dim=4),
    dict(obs_dim=10, num_actions=10, inner_embed_size=128, num_heads=8, history_len=50, discrete=True, vocab_sizes=9),
    dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, history_len=50, identity=True, pos="sin"),
    dict(obs_dim=1, num_actions=5, inner_embed_size=64, num_heads=4, history_len=64, discrete=True, vocab_sizes=22,
         action_dim=8, pos="none"),
    dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, history_len=50, gate="gru", action_dim=8, pos="sin"),
    # tiled path (L > 64 or D > 128)
    dict(obs_dim=6, num_actions=6, inner_embed_size=128, num_heads=8, history_len=128, discrete=True, vocab_sizes=12),
    dict(obs_dim=1, num_actions=5, inner_embed_size=256, num_heads=8, history_len=256, discrete=True, vocab_sizes=22, identity=True, pos="sin"),
    dict(obs_dim=3, num_actions=3, inner_embed_size=256, num_heads=8, history_len=100, action_dim=8),
    # placed by dtqn_net_init on a larger row-tile count / the tiled path (dtqn_limits.h): short contexts, head_dim 32, 64, 4
    dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, history_len=10),
    dict(obs_dim=3, num_actions=3, inner_embed_size=128, num_heads=8, history_len=20),
    dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=2, history_len=50),
    dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=1, history_len=50),
    dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=16, history_len=30),
    dict(obs_dim=3, num_actions=3, inner_embed_size=256, num_heads=4, history_len=128),
    # width-padded (DtqnNet.d_real): 48 -> 64 with two all-zero heads, 96 -> 128
    dict(obs_dim=3, num_actions=3, inner_embed_size=48, num_heads=6, history_len=50),
    dict(obs_dim=3, num_actions=3, inner_embed_size=96, num_heads=6, history_len=100, pos="sin", gate="gru"),
    dict(obs_dim=3, num_actions=3, inner_embed_size=48, num_heads=4, history_len=50),               # heads of 12 -> 16
    dict(obs_dim=3, num_actions=3, inner_embed_size=120, num_heads=5, history_len=128),             # heads of 24 -> 32, 160 -> 256 columns
]


@pytest.mark.parametrize("kw", VARIANTS)
def test_variants_vs_oracle(lib, kw):
    cfg = O.NetCfg(**kw)
    params = O.init_params(cfg, seed=3, perturb=True)
    rng = np.random.default_rng(5)
    pool = []
    for n in sorted({1, 2, cfg.history_len // 2, cfg.history_len}):
        Bn = 5
        obs = (rng.integers(0, cfg.vocab_sizes, size=(Bn, n, cfg.obs_dim)) if cfg.discrete
               else rng.uniform(-1, 1, size=(Bn, n, cfg.obs_dim)).astype(np.float32))
        act = rng.integers(0, cfg.num_actions, size=(Bn, n, 1))
        with torch.no_grad():
            ref = O.forward(params, cfg, torch.as_tensor(obs, dtype=torch.long if cfg.discrete else torch.float32),
                            torch.as_tensor(act, dtype=torch.long)).numpy()
        got = hip_forward(lib, cfg, params, obs, act)
        assert np.isfinite(got).all()
        assert np.abs(got - ref).max() <= Q_TOL * max(1.0, np.abs(ref).max()), (n, np.abs(got - ref).max())     # std-0.2 stress weights
        check_forward_f64(cfg, params, obs, act, got, what=("variant", n), pool=pool)
    check_pooled_f64(pool)


def test_seq_longer_than_context_is_rejected(lib):
    cfg = O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=16, num_heads=2, history_len=8)
    net = net_from_cfg(lib, cfg)
    assert lib.dtqn_forward(ctypes.byref(net), ctypes.c_void_p(8), ctypes.c_void_p(8), None, 1, 9, ctypes.c_void_p(8), None) == B.DEFINES["DTQN_ERR_ARG"]
