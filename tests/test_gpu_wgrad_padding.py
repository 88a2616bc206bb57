"""-m gpu: the one-launch weight gradients (dtqn_wgrad_direct_kernel) on the MI355X do not touch the rows behind the context -- the device
half of tests/test_emu_wgrad_padding.py.  After one forward_backward, NaN is written into rows [round-up-4(L), lp) of every X and every dY
operand of every job; a second weight-gradient launch must reproduce the first gradient bit for bit, finite throughout.  Plus one update
against the oracle at each shape.  The smallest shapes that reach each walk: a context of 50 at batch 2 (64-row records, one live step in
a sequence's last unit), 40 at batch 3 (a two-step unit and waves without any live step), 20 at batch 3 (32-row records, two units per
sequence).  The metric batch is covered by tests/test_gpu_wgrad_live.py."""
import ctypes

import pytest
import torch

from oracle import dtqn_oracle as O

from helpers import make_td_case, check_td_updates
from test_emu_wgrad_padding import poison_padding_rows

pytestmark = pytest.mark.gpu

CASES = [(50, 2, 64), (40, 3, 64), (20, 3, 32)]


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


def _case(lib, ctx, batch, lp):
    cfg = O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=ctx)
    net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=7, batch=batch, T=ctx + 20, n_eps=batch + 8, mask=-5, device="cuda", test_lib=False)
    assert net.lp == lp and lib.dtqn_td_wgrad_is_direct(ctypes.byref(net), batch) == 1
    assert not lib.dtqn_td_wgrad_is_fused(ctypes.byref(net), ctypes.byref(eng.td))
    return cfg, net, oracle, host, eng, rep


@pytest.mark.parametrize("ctx,batch,lp", CASES)
def test_rows_behind_the_context_are_not_read(lib, ctx, batch, lp):
    cfg, net, oracle, host, eng, rep = _case(lib, ctx, batch, lp)
    eps, starts = host.sample_indices(eng.batch)
    eng.set_indices(eps, starts)
    eng.forward_backward(rep)
    torch.cuda.synchronize()
    first = eng.grad.clone()
    assert bool(torch.isfinite(first).all()) and float(first.abs().max()) > 0
    assert poison_padding_rows(lib, net, eng, (ctx + 3) // 4 * 4) > 0
    eng.grad.zero_()
    torch.cuda.synchronize()
    s = eng._stream()
    assert lib.dtqn_td_wgrad(eng._net_ref, eng._td_ref, s) == 0
    assert lib.dtqn_td_reduce(eng._net_ref, eng._td_ref, s) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(eng.grad).all())
    assert torch.equal(eng.grad, first)


@pytest.mark.parametrize("ctx,batch,lp", CASES)
def test_weight_gradients_vs_oracle(lib, ctx, batch, lp):
    cfg, net, oracle, host, eng, rep = _case(lib, ctx, batch, lp)
    check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1)
