"""Key-blocked row-block attention (tl_attn_kb_kernel, tl_attn_kb_dkv_kernel, tl_attn_kb_dq_kernel) on the CPU emulation.

The whole-tile attention kernels hold one head's q | k | v | dO rows in LDS, which caps wide heads at short contexts (head width 32 at 256
rows, 64 at 128, 128 at 64).  Beyond that tile, native d_model 128 / 256 networks run the key-blocked kernels, which stage 64 rows of
k | v (or q | dO) at a time.  DTQN_ATTN_KBLOCK=1 forces them on any row-block shape, which is how they are held against the whole-tile
kernels here."""
import numpy as np
import pytest
import torch

from dtqn_amd import _binding as B
from oracle import dtqn_oracle as O

from helpers import make_td_case, check_td_updates


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


# (d_model, heads, context, extra make_net arguments) -> padded context rows
NEW_SHAPES = [
    (256, 8, 512, {}, 512),                        # BASELINE config 5 at the context bound
    (128, 4, 300, {}, 320),
    (128, 2, 129, {}, 192),
    (256, 4, 512, {}, 512),
    (128, 1, 65, {}, 128),
    (128, 1, 512, {}, 512),
    (256, 2, 300, {}, 320),
    (128, 2, 150, {"image": (3, 16, 16)}, 192),    # image networks: the same attention launches
]


@pytest.mark.parametrize("d,h,ctx,kw,lp", NEW_SHAPES)
def test_wide_heads_at_long_contexts_construct(emu, d, h, ctx, kw, lp):
    net = B.make_net(emu, obs_dim=3, num_actions=4, inner_embed_size=d, num_heads=h, num_layers=2, history_len=ctx, **kw)
    assert net.tiled == 1 and net.lp == lp and net.head_dim == d // h and net.d_real == 0


@pytest.mark.parametrize("kw", [
    dict(inner_embed_size=64, num_heads=2, history_len=400),              # d_model 64 keeps the whole-tile bound
    dict(inner_embed_size=140, num_heads=2, history_len=100),             # width-padded (70 -> 128-wide heads)
    dict(inner_embed_size=128, num_heads=2, history_len=200, bag_size=8),  # bag networks keep the whole-tile bound
    dict(inner_embed_size=256, num_heads=8, history_len=513),             # contexts beyond 512
])
def test_shapes_outside_the_key_blocked_scope_stay_refused(emu, kw):
    with pytest.raises(NotImplementedError):
        B.make_net(emu, obs_dim=3, num_actions=4, num_layers=1, **kw)


def _launched(err):
    return {"kb": "tl_attn_kb_kernel" in err and "tl_attn_kb_dkv_kernel" in err and "tl_attn_kb_dq_kernel" in err,
            "whole": "tl_attn_kernel" in err or "tl_attn_bwd_kernel" in err}


TD_CASES = [
    (dict(obs_dim=3, num_actions=4, inner_embed_size=128, num_heads=2, num_layers=1, history_len=160), dict(batch=2, mask=-5)),
    (dict(obs_dim=3, num_actions=4, inner_embed_size=128, num_heads=1, num_layers=1, history_len=96, gate="gru"), dict(batch=2, mask=-5)),
    (dict(obs_dim=3, num_actions=4, inner_embed_size=128, num_heads=4, num_layers=1, history_len=300, pos="sin", action_dim=8),
     dict(batch=1, mask=-5)),
]


@pytest.mark.parametrize("kw,run", TD_CASES)
def test_td_update_on_the_key_blocked_kernels_vs_oracle(emu, kw, run, monkeypatch, capfd):
    monkeypatch.setenv("DTQN_TL_TRACE", "1")
    cfg = O.NetCfg(**kw)
    net, oracle, host, eng, rep = make_td_case(emu, cfg, seed=17, batch=run["batch"], T=cfg.history_len + 8, n_eps=3, mask=run["mask"])
    assert eng.net.tiled == 1
    check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1)
    assert _launched(capfd.readouterr().err) == {"kb": True, "whole": False}


def _one_update(emu, cfg, knob, monkeypatch, capfd, seed=29, batch=2):
    """One TD update against the oracle with DTQN_ATTN_KBLOCK=knob -> (Q of the three forwards, gradient, launch trace)."""
    monkeypatch.setenv("DTQN_TL_TRACE", "1")
    monkeypatch.setenv("DTQN_ATTN_KBLOCK", knob)
    net, oracle, host, eng, rep = make_td_case(emu, cfg, seed=seed, batch=batch, T=cfg.history_len + 8, n_eps=3, mask=-5)
    capfd.readouterr()
    check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1)
    err = capfd.readouterr().err
    return eng.q3.clone(), eng.grad.clone(), err


FORCED = [
    dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=100),
    dict(obs_dim=3, num_actions=4, inner_embed_size=128, num_heads=8, num_layers=1, history_len=130),
    dict(obs_dim=3, num_actions=4, inner_embed_size=48, num_heads=4, num_layers=1, history_len=100),      # heads of 12 -> 16: hd_eff
    dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=100, dropout=0.1),
]


@pytest.mark.parametrize("kw", FORCED)
def test_forced_key_blocked_kernels_match_the_whole_tile_ones(emu, kw, monkeypatch, capfd):
    """DTQN_ATTN_KBLOCK=1 on shapes the whole-tile kernels cover: both against the oracle and against each other (dropout: the same keep
    masks on both paths).  Without the knob such a shape keeps launching the whole-tile kernels."""
    monkeypatch.setenv("DTQN_FORCE_TILED", "1")
    cfg = O.NetCfg(**kw)
    q0, g0, err0 = _one_update(emu, cfg, "0", monkeypatch, capfd)
    q1, g1, err1 = _one_update(emu, cfg, "1", monkeypatch, capfd)
    assert _launched(err0) == {"kb": False, "whole": True}
    assert "tl_launch (tl_attn_kernel<" in err0 and "tl_launch (tl_attn_bwd_kernel<" in err0
    assert _launched(err1) == {"kb": True, "whole": False}
    assert (torch.abs(q1 - q0) <= 1e-5 * torch.clamp(torch.abs(q0), min=1.0)).all(), float(torch.abs(q1 - q0).max())
    assert float(torch.abs(g1 - g0).max()) <= 1e-4 * float(torch.abs(g0).max())


def test_key_blocked_update_is_deterministic(emu, monkeypatch, capfd):
    """A fixed summation order and no float atomics: the same update twice gives the same bits."""
    cfg = O.NetCfg(obs_dim=3, num_actions=4, inner_embed_size=128, num_heads=2, num_layers=1, history_len=140)
    qa, ga, erra = _one_update(emu, cfg, "0", monkeypatch, capfd, seed=31, batch=1)
    qb, gb, _ = _one_update(emu, cfg, "0", monkeypatch, capfd, seed=31, batch=1)
    assert _launched(erra) == {"kb": True, "whole": False}
    assert torch.equal(qa, qb) and torch.equal(ga, gb)
