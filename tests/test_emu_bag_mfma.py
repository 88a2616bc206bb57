"""Bag attention on the matrix core (tl_bag_attn_mfma_kernel, tl_bag_attn_mfma_dkv_kernel, tl_bag_attn_mfma_dq_kernel) on the CPU emulation.

The resident bag kernels keep the bag's k | v rows and, in the backward, an [L][bag] dS tile in LDS; dtqn_net_init admits bags up to the
padded context, and beyond (2 bag HD + L bag) 4 B = 160 KB that request cannot be launched.  Those networks run the matrix-core kernels,
which stage 64 bag entries or 64 query rows at a time.  DTQN_BAG_ATTN_MFMA=1 forces them on any bag, which is how they are held against the
resident kernels here.

Bounds: those of helpers.check_td_updates (Q 1e-4 max(1, |Q|max), gradients 2e-4 max|g| conditional on the engine's ReLU / argmax pattern
with its flip caps, statistics 2e-4); old against new: the same Q and gradient bounds; the head-averaged weights: the 1e-5 of
attention_helpers.check_weights."""
import numpy as np
import pytest
import torch

from dtqn_amd import _binding as B
from oracle import dtqn_oracle as O

from bag_mfma_helpers import (LDS_BYTES, OVERFLOW, SMALL, agent_train_run, bag_weights, launched, one_update, resident_bwd_lds, small_cfg,
                              td_and_autograd_gradients)


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.mark.parametrize("name,kw,seed", OVERFLOW, ids=[c[0] for c in OVERFLOW])
def test_td_update_beyond_the_resident_tile_vs_oracle(emu, name, kw, seed, monkeypatch, capfd):
    cfg = O.NetCfg(**kw)
    assert resident_bwd_lds(cfg) > LDS_BYTES
    _, _, err = one_update(emu, cfg, None, monkeypatch, capfd, seed=seed, batch=1)
    assert launched(err) == {"mfma": True, "resident": False, "mixed": False}


def test_small_bags_keep_the_resident_kernels(emu, monkeypatch, capfd):
    cfg = small_cfg(20, 5, 0.0)
    assert resident_bwd_lds(cfg) <= LDS_BYTES
    _, _, err = one_update(emu, cfg, None, monkeypatch, capfd, seed=29, batch=2)
    assert launched(err) == {"mfma": False, "resident": True, "mixed": False}


@pytest.mark.parametrize("ctx,bag,p", SMALL)
def test_forced_matrix_core_kernels_match_the_resident_ones(emu, ctx, bag, p, monkeypatch, capfd):
    """Both families against the oracle (dropout: the same keep masks on both) and against each other.  The captured weights are compared in
    eval mode for every p (capture refuses train-mode dropout), so the p = 0.1 cases add nothing to THAT comparison: under dropout the
    pre-dropout record is held only through the gradient bound, which reads it in both backward kernels."""
    cfg = small_cfg(ctx, bag, p)
    q0, g0, err0 = one_update(emu, cfg, "0", monkeypatch, capfd, seed=29, batch=2)
    q1, g1, err1 = one_update(emu, cfg, "1", monkeypatch, capfd, seed=29, batch=2)
    assert launched(err0) == {"mfma": False, "resident": True, "mixed": False}
    assert launched(err1) == {"mfma": True, "resident": False, "mixed": False}
    dq, dg = float(torch.abs(q1 - q0).max()), float(torch.abs(g1 - g0).max())
    print("old vs new", ctx, bag, p, "dQ", dq, "|Q|max", float(torch.abs(q0).max()), "dg", dg, "|g|max", float(torch.abs(g0).max()))
    assert dq <= 1e-4 * max(1.0, float(torch.abs(q0).max()))
    assert dg <= 2e-4 * float(torch.abs(g0).max())
    # attention capture reads the record the forward wrote (eval mode: capture refuses train-mode dropout)
    monkeypatch.setenv("DTQN_BAG_ATTN_MFMA", "0")
    qa, wa = bag_weights(emu, cfg, seed=7, batch=2, n=ctx)
    monkeypatch.setenv("DTQN_BAG_ATTN_MFMA", "1")
    qb, wb = bag_weights(emu, cfg, seed=7, batch=2, n=ctx)
    assert wa.shape == wb.shape == (2, ctx, bag)
    assert np.abs(wa - wb).max() <= 1e-5 and np.abs(wb.sum(-1) - 1.0).max() <= 1e-5
    assert np.abs(qa - qb).max() <= 1e-4 * max(1.0, float(np.abs(qa).max()))


def test_differentiable_forward_beyond_the_resident_tile(emu, monkeypatch, capfd):
    """loss.backward() through the matrix-core kernels: the fused update's gradient, bit for bit; captured weights are distributions."""
    name, kw, seed = OVERFLOW[0]
    cfg = O.NetCfg(**kw)
    monkeypatch.setenv("DTQN_TL_TRACE", "1")
    q, q_td, got, ref = td_and_autograd_gradients(emu, cfg, seed=seed, batch=1)
    assert launched(capfd.readouterr().err) == {"mfma": True, "resident": False, "mixed": False}
    assert np.array_equal(q, q_td)
    assert np.abs(ref).max() > 0 and np.isfinite(got).all() and np.array_equal(got, ref)
    monkeypatch.delenv("DTQN_TL_TRACE")
    _, w = bag_weights(emu, cfg, seed=7, batch=1, n=100)           # a partial context
    assert w.shape == (1, 100, cfg.bag_size) and (w >= 0).all()
    assert np.abs(w.sum(-1) - 1.0).max() <= 1e-5


def test_matrix_core_bag_update_is_deterministic(emu, monkeypatch, capfd):
    """A fixed summation order and no float atomics: the same update twice gives the same bits (two bag blocks, dropout on)."""
    cfg = O.NetCfg(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=100, action_dim=4, bag_size=80,
                   dropout=0.1)
    qa, ga, erra = one_update(emu, cfg, "1", monkeypatch, capfd, seed=31, batch=2)
    qb, gb, _ = one_update(emu, cfg, "1", monkeypatch, capfd, seed=31, batch=2)
    assert launched(erra) == {"mfma": True, "resident": False, "mixed": False}
    assert torch.equal(qa, qb) and torch.equal(ga, gb)


def test_agent_train_beyond_the_resident_tile_is_deterministic(emu, monkeypatch, capfd):
    """DtqnAgent.train() with the device sampler at context 256 / bag 160: finite statistics, the same bits from the same seed."""
    monkeypatch.setenv("DTQN_TL_TRACE", "1")
    sa, ta = agent_train_run(emu, 11, updates=2)
    assert launched(capfd.readouterr().err) == {"mfma": True, "resident": False, "mixed": False}
    monkeypatch.delenv("DTQN_TL_TRACE")
    sb, tb = agent_train_run(emu, 11, updates=2)
    for st in sa:
        assert st["nonfinite"] == 0.0 and all(np.isfinite(v) for v in st.values()), st
    assert np.isfinite(ta).all() and np.array_equal(ta, tb) and sa == sb
