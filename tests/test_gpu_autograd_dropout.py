"""-m gpu: train-mode dropout in the differentiable forward on the MI355X -- Q, parameter and observation gradients against the oracle
under the engine's keep masks (the cases of tests/autograd_dropout_helpers.py), the mask semantics of DTQN.set_dropout_seed, and a
torch.optim.Adam loop on the module."""
import math

import numpy as np
import pytest
import torch

from oracle import dtqn_oracle as O

from autograd_dropout_helpers import BATCH, CASES, SEED, STEP, check_dropout_parity, flat_grad, hip_grads_drop
from autograd_helpers import hip_grads, make_inputs, make_module

pytestmark = pytest.mark.gpu

# a context past 64 rows runs on the row-block kernels by itself; the tests below feed it prefixes of 20 and 13 rows
ROWBLOCK = dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=2, history_len=70, action_dim=4, dropout=0.1)


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    torch.cuda.set_device(0)
    return engine.get_lib()


def test_the_refused_call_runs_and_the_seed_surface_exists(lib):
    from dtqn_amd.networks.dtqn import DTQN
    m = DTQN(3, 3, 8, 0, 64, 8, 2, 50, dropout=0.1, autograd=True).to("cuda")
    o, a = torch.rand(2, 50, 3, device="cuda"), torch.zeros(2, 50, 1, dtype=torch.long, device="cuda")
    m(o, a, _train_dropout=(1, 2)).sum().backward()
    g = flat_grad(m)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    m.set_dropout_seed(1)
    m(o, a).sum().backward()
    assert m._drop_step == 1


@pytest.mark.parametrize("name", list(CASES))
def test_parity_under_the_engines_mask_on_device(lib, name):
    kw, n = CASES[name]
    cfg = O.NetCfg(**kw)
    params = O.init_params(cfg, seed=3, perturb=True)
    m = make_module(None, cfg, params, device="cuda")
    obs, act, bag, w = make_inputs(cfg, BATCH, n, seed=5)
    q = check_dropout_parity(m, cfg, params, obs, act, bag, w, device="cuda")[0]
    # the no-grad forward draws the same masks for the same keys
    kwb = {} if bag is None else dict(bag_obss=torch.as_tensor(bag[0], device="cuda"), bag_actions=torch.as_tensor(bag[1], device="cuda"))
    with torch.no_grad():
        q_ng = m(torch.as_tensor(obs, device="cuda"), torch.as_tensor(act, device="cuda"), _train_dropout=(SEED, STEP), **kwb).cpu().numpy()
    assert np.array_equal(q_ng, q)


def rowblock_module(**over):
    cfg = O.NetCfg(**{**ROWBLOCK, **over})
    params = O.init_params(cfg, seed=3, perturb=True)
    m = make_module(None, cfg, params, device="cuda")
    assert m.net.tiled == 1
    return cfg, params, m


def test_mask_semantics_on_device(lib):
    cfg, params, m = rowblock_module()
    obs, act, _, w = make_inputs(cfg, BATCH, 20, seed=5)
    a = hip_grads_drop(m, obs, act, None, w, (SEED, STEP), device="cuda")
    b = hip_grads_drop(m, obs, act, None, w, (SEED, STEP), device="cuda")
    c = hip_grads_drop(m, obs, act, None, w, (SEED, STEP + 1), device="cuda")
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and not np.array_equal(x, z)
    # the module's own counter, two forwards before one backward
    obs2, act2, _, w2 = make_inputs(cfg, BATCH, 13, seed=6)
    g2 = hip_grads_drop(m, obs2, act2, None, w2, (SEED, STEP + 1), device="cuda")[1]
    m.train()
    m.set_dropout_seed(SEED, STEP)
    m.zero_grad(set_to_none=True)
    t = lambda x: torch.as_tensor(x, device="cuda")
    qa, qb = m(t(obs), t(act)), m(t(obs2), t(act2))
    assert np.array_equal(qa.detach().cpu().numpy(), a[0])
    ((qa * t(w)).sum() + (qb * t(w2)).sum()).backward()
    assert np.array_equal(flat_grad(m), a[1] + g2)
    # eval(), and no seed: the forward of the same weights at dropout 0
    plain = make_module(None, O.NetCfg(**{**ROWBLOCK, "dropout": 0.0}), params, device="cuda")
    ref = hip_grads(plain, obs, act, None, w, device="cuda")
    m.eval()
    ev = hip_grads(m, obs, act, None, w, device="cuda")
    m.train()
    m.set_dropout_seed(None)
    never = hip_grads(m, obs, act, None, w, device="cuda")
    for got in (ev, never):
        for x, y in zip(got, ref):
            assert np.array_equal(x, y)


def test_keep_rate_on_device(lib):
    from dtqn_amd.networks.dtqn import _GradRunner
    p, Bn, n = 0.1, 8, 50
    cfg = O.NetCfg(obs_dim=4, num_actions=4, inner_embed_size=128, num_heads=8, num_layers=1, history_len=50, dropout=p)
    m = make_module(None, cfg, O.init_params(cfg, seed=3, perturb=True), device="cuda")
    obs, act, _, _ = make_inputs(cfg, Bn, n, seed=9)
    runner = _GradRunner(m, torch.as_tensor(obs, device="cuda"), torch.as_tensor(act, device="cuda"), None, None, (SEED, STEP))
    runner.forward()
    net = runner.net
    rec = runner.ws.cpu().numpy()[:Bn * net.act_stride].reshape(Bn, net.act_stride)
    off = net.ao_layer0 + net.al_u1                 # x0 = dropout(embedding + position): a dropped element is exactly 0
    x0 = rec[:, off:off + net.lp * net.d_model].reshape(Bn, net.lp, net.d_model)[:, :n]
    kept, total = int(np.count_nonzero(x0)), x0.size
    assert total == Bn * n * 128 and abs(kept - total * (1 - p)) <= 4 * math.sqrt(total * p * (1 - p)), (kept, total)


def test_optimiser_loop_on_device(lib):
    """20 steps of torch.optim.Adam with clip_grad_norm_ on a train-mode module with its own dropout counter: the loss stays finite,
    theta moves, and a second run from the same seeds ends at identical theta."""
    def run():
        cfg, _, m = rowblock_module()
        m.train()
        m.set_dropout_seed(SEED)
        theta0 = m.flat.detach().clone()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        obs, act, _, w = make_inputs(cfg, 8, 20, seed=5)
        o, a, target = (torch.as_tensor(x, device="cuda") for x in (obs, act, w))
        for _ in range(20):
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.smooth_l1_loss(m(o, a), target)
            assert torch.isfinite(loss)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0, error_if_nonfinite=True)
            opt.step()
        assert m._drop_step == 20 and not torch.equal(m.flat, theta0) and torch.isfinite(m.flat).all()
        return m.flat.detach().cpu().clone()
    assert torch.equal(run(), run())
