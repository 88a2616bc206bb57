"""The one-launch weight gradients (dtqn_wgrad_direct_kernel) do not touch the rows behind the context.  The backward leaves an all-zero
dY in rows [L, lp) of every sequence; a wave whose 16-token units all sit at the same place of their sequence (16 waves on 1, 2 or 4
units per sequence) walks only the 4-token steps that hold a live row.  On the CPU emulation: after one
forward_backward, NaN is written into rows [round-up-4(L), lp) of every X and every dY operand of every job (dtqn_net_wjobs), and a
second weight-gradient launch must reproduce the first gradient bit for bit, finite throughout -- a kernel that multiplied those rows
by the zero gradient rows would produce 0 * NaN.  Shapes: a context of 50 in 64-row records (one live step in a sequence's last unit), 49
(that step ends inside it; fewer units than waves at batch 3), 40 (a two-step unit, and waves without any live step), 33 (a one-step unit),
20 in 32-row records (two units per sequence), and GRU gates (jobs that loop over layers).  A bag network contracts every row of its
records (live rows = all rows, nothing is skipped): oracle parity and a bit-identical repeat only."""
import ctypes

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


BASE = dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2)
# name -> (network, batch, records' rows lp)
POISON_CASES = {
    "L50-b2": (dict(BASE, history_len=50), 2, 64),
    "L49-b3": (dict(BASE, history_len=49), 3, 64),
    "L40-b2": (dict(BASE, history_len=40), 2, 64),
    "L33-b2": (dict(BASE, history_len=33), 2, 64),
    "L20-b3": (dict(BASE, history_len=20), 3, 32),
    "gru-L20-b3": (dict(BASE, history_len=20, gate="gru"), 3, 32),
}
BAG_CASE = (dict(BASE, history_len=20, bag_size=5), 2, 64)


def _case(emu, kw, batch, lp):
    cfg = O.NetCfg(**kw)
    L = cfg.history_len
    net, oracle, host, eng, rep = make_td_case(emu, cfg, seed=7, batch=batch, T=L + 20, n_eps=6, mask=-5)
    assert net.lp == lp and emu.dtqn_td_wgrad_is_direct(ctypes.byref(net), batch) == 1
    assert not emu.dtqn_td_wgrad_is_fused(ctypes.byref(net), ctypes.byref(eng.td))
    return cfg, net, oracle, host, eng, rep


def _wgrad(eng):
    s = eng._stream()
    assert eng.lib.dtqn_td_wgrad(eng._net_ref, eng._td_ref, s) == 0
    assert eng.lib.dtqn_td_reduce(eng._net_ref, eng._td_ref, s) == 0


def poison_padding_rows(lib, net, eng, first_row):
    """NaN into rows [first_row, lp) of every X and dY operand of every weight-gradient job, layer and sequence.  Returns the rows written."""
    jobs = (B.DtqnWJob * net.n_wjobs)()
    assert lib.dtqn_net_wjobs(ctypes.byref(net), jobs) == 0
    act = eng.act[:eng.batch * net.act_stride].view(eng.batch, net.act_stride)
    grd = eng.grd.view(eng.batch, net.grd_stride)
    rows = 0
    for j in jobs:
        for l in range(j.n_layers):
            for buf, off, ld in ((act if j.x_in_act else grd, j.x_off + l * j.x_lstride, j.ldx), (grd, j.dy_off + l * j.dy_lstride, j.ldy)):
                buf[:, off + first_row * ld:off + net.lp * ld] = float("nan")
                rows += net.lp - first_row
    return rows


@pytest.mark.parametrize("name", sorted(POISON_CASES))
def test_rows_behind_the_context_are_not_read(emu, name):
    kw, batch, lp = POISON_CASES[name]
    cfg, net, oracle, host, eng, rep = _case(emu, kw, batch, lp)
    eps, starts = host.sample_indices(eng.batch)
    eng.set_indices(eps, starts)
    eng.forward_backward(rep)
    first = eng.grad.clone()
    assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0
    L = cfg.history_len
    assert poison_padding_rows(emu, net, eng, (L + 3) // 4 * 4) > 0
    assert bool(torch.isnan(eng.grd).any()) and bool(torch.isnan(eng.act).any())
    eng.grad.zero_()
    _wgrad(eng)
    assert bool(torch.isfinite(eng.grad).all())
    assert torch.equal(eng.grad, first)


@pytest.mark.parametrize("name", sorted(POISON_CASES))
def test_weight_gradients_vs_oracle(emu, name):
    kw, batch, lp = POISON_CASES[name]
    cfg, net, oracle, host, eng, rep = _case(emu, kw, batch, lp)
    check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1)


def test_bag_network_contracts_every_row(emu):
    """Bag entries fill the records' rows past the context: every step of every unit stays in the product."""
    kw, batch, lp = BAG_CASE
    cfg, net, oracle, host, eng, rep = _case(emu, kw, batch, lp)
    check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1)
    eps, starts = host.sample_indices(eng.batch)
    eng.set_indices(eps, starts)
    rng = np.random.Generator(np.random.PCG64(77))
    eng.set_bag(rng.random((batch, cfg.bag_size, cfg.obs_dim), dtype=np.float32), rng.integers(0, cfg.num_actions, (batch, cfg.bag_size, 1)))
    eng.forward_backward(rep)
    first = eng.grad.clone()
    assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0
    eng.grad.zero_()
    _wgrad(eng)
    assert torch.equal(eng.grad, first)
