"""-m gpu: the one-launch weight gradients (dtqn_wgrad_direct_kernel) on the MI355X against the oracle at the token-axis edge shapes of
tests/test_emu_wgrad_live.py: a context of 50 (two live rows in a sequence's last 16-token block) at batch 2, a context of 49 (ends inside a
4-token step) at batch 3 -- fewer units than waves -- and the metric shapes (BASELINE config 1) at batch 32.  One update each."""
import ctypes

import pytest

from oracle import dtqn_oracle as O

from helpers import make_td_case, check_td_updates

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("ctx,batch", [(50, 2), (49, 3), (50, 32)])
def test_weight_gradients_vs_oracle(lib, ctx, batch):
    cfg = O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=ctx)
    net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=7, batch=batch, T=ctx + 20, n_eps=batch + 8, mask=-5, device="cuda", test_lib=False)
    assert net.lp == 64 and lib.dtqn_td_wgrad_is_direct(ctypes.byref(net), batch) == 1
    assert not lib.dtqn_td_wgrad_is_fused(ctypes.byref(net), ctypes.byref(eng.td))
    check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1)
