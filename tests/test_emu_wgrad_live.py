"""The one-launch weight gradients (dtqn_wgrad_direct_kernel) at the shapes where a walk over the token axis can go wrong -- a context that
leaves two live rows in a sequence's last 16-token block, one that ends inside a 4-token step, one without padding rows, one 16-token unit
per sequence; batches at which a wave's last unit is partial; jobs that loop over layers (GRU gates) or run over bag entries.  On the CPU
emulation: one TD update against the oracle (flat gradient within the usual 2e-4 * max|g|, helpers.check_td_updates) and two launches on
the same records bit-identical.  (Written with the live-token walk of round 7, docs/experiments/r07_wgrad_live_tokens.patch, which also
kept the rows behind the context out of the product; it measured slower on the MI355X and is not in the kernel -- DESIGN.md section 3.3.
The kernel as it stands multiplies those rows by the zero gradient rows the backward leaves there, so that property is not asserted.)"""
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
# (network, batch, records' rows lp): a context of 50 in 64-row records leaves two live rows in a sequence's last 16-token block, 49 a partial
# last 4-token step, 64 no padding rows at all, 16 one unit per sequence; batches 2 and 3: fewer units than waves, a partial last round;
# GRU gates: jobs that loop over the layers; a bag: two jobs over bag entries
CASES = {
    "L50-b2": (dict(BASE, history_len=50), 2, 64),
    "L49-b3": (dict(BASE, history_len=49), 3, 64),
    "L64-b2": (dict(BASE, history_len=64), 2, 64),
    "L16-b3": (dict(BASE, history_len=16), 3, 16),
    "L50-b3": (dict(BASE, history_len=50), 3, 64),
    "gru-L20-b3": (dict(BASE, history_len=20, gate="gru"), 3, 32),
    "bag-L20-b2": (dict(BASE, history_len=20, bag_size=5), 2, 64),
}


def _case(emu, name):
    kw, batch, lp = CASES[name]
    cfg = O.NetCfg(**kw)
    L = cfg.history_len
    net, oracle, host, eng, rep = make_td_case(emu, cfg, seed=7, batch=batch, T=L + 20, n_eps=6, mask=-5)
    assert net.lp == lp and emu.dtqn_td_wgrad_is_direct(ctypes.byref(net), batch) == 1
    assert not emu.dtqn_td_wgrad_is_fused(ctypes.byref(net), ctypes.byref(eng.td))
    return cfg, net, oracle, host, eng, rep


@pytest.mark.parametrize("name", sorted(CASES))
def test_weight_gradients_vs_oracle(emu, name):
    cfg, net, oracle, host, eng, rep = _case(emu, name)
    check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1)


def _wgrad(eng):
    s = eng._stream()
    assert eng.lib.dtqn_td_wgrad(eng._net_ref, eng._td_ref, s) == 0
    assert eng.lib.dtqn_td_reduce(eng._net_ref, eng._td_ref, s) == 0


@pytest.mark.parametrize("name", ["L50-b2", "L49-b3", "gru-L20-b3", "bag-L20-b2"])
def test_two_launches_on_the_same_records_are_bit_identical(emu, name):
    """A fixed order of the sums: the second launch writes the same bits, also into a gradient buffer that was cleared in between."""
    cfg, net, oracle, host, eng, rep = _case(emu, name)
    Bn = eng.batch
    eps, starts = host.sample_indices(Bn)
    eng.set_indices(eps, starts)
    if cfg.bag_size > 0:
        rng = np.random.Generator(np.random.PCG64(77))
        eng.set_bag(rng.random((Bn, cfg.bag_size, cfg.obs_dim), dtype=np.float32), rng.integers(0, cfg.num_actions, (Bn, cfg.bag_size, 1)))
    eng.forward_backward(rep)
    first = eng.grad.clone()
    assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0
    _wgrad(eng)
    assert torch.equal(eng.grad, first)
    eng.grad.zero_()
    _wgrad(eng)
    assert torch.equal(eng.grad, first)
