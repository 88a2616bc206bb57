"""Train-mode dropout in the differentiable forward (dtqn_forward_train_drop + dtqn_backward_dq_drop, DTQN.set_dropout_seed) on the CPU
emulation of the HIP sources: parity with the oracle under the engine's keep masks, consistency with the fused TD update, the mask
semantics of the module surface, and the bits of the two entry points that keep their signatures.

Whole-sequence shapes: a forward with dropout takes Q from the row-block twin too (the kernels that write the records the backward
reads), so Q and the gradient come from one set of masks; test_whole_sequence_shape_takes_q_from_the_twin_under_dropout pins that."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from dtqn_amd import _binding as B
from dtqn_amd.networks.dtqn import DTQN, _GradRunner
from oracle import dtqn_oracle as O

from autograd_dropout_helpers import BATCH, CASES, SEED, STEP, check_dropout_parity, flat_grad, hip_grads_drop
from autograd_helpers import hip_grads, make_inputs, make_module
from helpers import make_td_case, oracle_batch, ptr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# a context past 64 rows runs on the row-block kernels by itself; the tests below feed it prefixes of 20 and 13 rows
ROWBLOCK = dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=2, history_len=70, action_dim=4, dropout=0.1)


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


def test_the_refused_call_runs_and_the_seed_surface_exists(emu):
    m = DTQN(3, 3, 8, 0, 64, 8, 2, 50, dropout=0.1, autograd=True, _test_lib=emu)
    m._allow_cpu = True
    o, a = torch.rand(2, 50, 3), torch.zeros(2, 50, 1, dtype=torch.long)
    m(o, a, _train_dropout=(1, 2)).sum().backward()
    g = flat_grad(m)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    assert m.set_dropout_seed(1) is m
    m(o, a).sum().backward()
    assert m._drop_step == 1


@pytest.mark.parametrize("name", list(CASES))
def test_parity_under_the_engines_mask(emu, name):
    kw, n = CASES[name]
    cfg = O.NetCfg(**kw)
    params = O.init_params(cfg, seed=3, perturb=True)
    m = make_module(emu, cfg, params)
    if name.startswith("cfg1") or name == "d128_h8":
        assert m.net.tiled == 0                     # shapes of the whole-sequence family: records and Q on the row-block twin
    obs, act, bag, w = make_inputs(cfg, BATCH, n, seed=5)
    check_dropout_parity(m, cfg, params, obs, act, bag, w)


def test_whole_sequence_shape_takes_q_from_the_twin_under_dropout(emu):
    kw, n = CASES["cfg1"]
    cfg = O.NetCfg(**kw)
    m = make_module(emu, cfg, O.init_params(cfg, seed=3, perturb=True))
    obs, act, _, _ = make_inputs(cfg, BATCH, n, seed=5)
    o, a = np.ascontiguousarray(obs), np.ascontiguousarray(act.reshape(BATCH, n), dtype=np.uint8)
    twin = m._grad_net()
    assert twin is not m.net and twin.tiled == 1 and twin.dropout == m.net.dropout
    ws = np.zeros(emu.dtqn_grad_workspace_floats(ctypes.byref(twin), BATCH, n), np.float32)
    q_twin = np.zeros((BATCH, n, cfg.num_actions), np.float32)
    assert emu.dtqn_forward_train_drop(ctypes.byref(twin), ptr(m.flat.numpy()), ptr(o), ptr(a), None, None, BATCH, n, ptr(q_twin), ptr(ws),
                                       SEED, STEP, None) == 0
    q = m(torch.tensor(obs, requires_grad=True), torch.as_tensor(act), _train_dropout=(SEED, STEP))
    assert np.array_equal(q.detach().numpy(), q_twin)
    with torch.no_grad():
        assert np.array_equal(m(torch.as_tensor(obs), torch.as_tensor(act), _train_dropout=(SEED, STEP)).numpy(), q_twin)


# ------------------------------------------------------------------------------------------ consistency with the fused TD update
def td_and_autograd_gradients(emu, kw, run):
    cfg = O.NetCfg(**kw)
    net, oracle, host, eng, rep = make_td_case(emu, cfg, seed=23, batch=run["batch"], T=run["T"], n_eps=run.get("n_eps", 6), mask=-5)
    eng.td.dropout_seed = SEED
    Bn, L, A, hist, gamma = eng.batch, cfg.history_len, cfg.num_actions, cfg.history_len, np.float32(0.99)
    eps, starts = host.sample_indices(Bn)
    eng.set_indices(eps, starts)
    eng.forward_backward(rep)
    step = int(eng.step_counter[1].item())
    tnet = eng.net
    q3 = torch.from_numpy(eng.q3.numpy().reshape(3, Bn, tnet.lp, tnet.ap)[:, :, :L, :A].copy())
    batch = oracle_batch(host, eps, starts, cfg.discrete)
    m = make_module(emu, cfg, oracle.pol)
    assert np.array_equal(m.flat.numpy(), eng.theta_pol.numpy())
    q = m(batch.obss, batch.actions, _train_dropout=(SEED, step))
    # tl_loss_kernel (td_loss_wave): y = r + (1 - done) * (Q_tgt(o')[argmax Q_pol(o')] * gamma); dQ[a] = 2 (Q[a] - y) / (B * history)
    with torch.no_grad():
        amax = torch.argmax(q3[1], dim=2, keepdim=True)
        qt = q3[2].gather(2, amax)
        y = batch.rewards + (1.0 - batch.dones.float()) * (qt * float(gamma))
        diff = q.detach().gather(2, batch.actions) - y
        inv_count = np.float32(1.0) / (np.float32(Bn) * np.float32(hist))
        dq = torch.zeros_like(q).scatter_(2, batch.actions, 2.0 * diff * float(inv_count))
        dq[:, :L - hist] = 0.0
    m.zero_grad(set_to_none=True)
    q.backward(dq)
    return eng, q.detach().numpy(), q3[0].numpy(), flat_grad(m), eng.grad.numpy()[:tnet.n_trainable].copy()


@pytest.mark.parametrize("kw,run", [
    (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=70, dropout=0.1), dict(batch=3, T=90)),
    (dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=2, num_layers=2, history_len=70, gate="gru", dropout=0.2), dict(batch=3, T=90)),
    (dict(obs_dim=4, num_actions=4, inner_embed_size=128, num_heads=8, num_layers=1, history_len=70, dropout=0.1), dict(batch=2, T=80, n_eps=10)),
])
def test_gradient_equals_the_td_updates_on_row_block_nets(emu, kw, run):
    eng, q, q_td, got, ref = td_and_autograd_gradients(emu, kw, run)
    assert eng.net.tiled == 1
    assert np.array_equal(q, q_td)                  # the training third of the update and this forward: same masks, same kernels
    assert np.abs(ref).max() > 0 and np.array_equal(got, ref)


def test_gradient_matches_the_td_updates_on_a_whole_sequence_shape(emu):
    kw = dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, history_len=50, dropout=0.1)
    eng, q, q_td, got, ref = td_and_autograd_gradients(emu, kw, dict(batch=2, T=60, n_eps=10))
    assert eng.net.tiled == 0                       # the update ran the whole-sequence kernels, the module their row-block twin
    assert np.abs(q - q_td).max() <= 1e-4 * max(1.0, float(np.abs(q_td).max()))
    assert np.abs(got - ref).max() <= 2e-4 * np.abs(ref).max(), np.abs(got - ref).max() / np.abs(ref).max()


# ------------------------------------------------------------------------------------------ mask semantics
def rowblock_module(emu, **over):
    cfg = O.NetCfg(**{**ROWBLOCK, **over})
    params = O.init_params(cfg, seed=3, perturb=True)
    m = make_module(emu, cfg, params)
    assert m.net.tiled == 1
    return cfg, params, m


def test_same_keys_same_bits_and_consecutive_forwards_differ(emu):
    cfg, _, m = rowblock_module(emu)
    obs, act, _, w = make_inputs(cfg, BATCH, 20, seed=5)
    a = hip_grads_drop(m, obs, act, None, w, (SEED, STEP))
    b = hip_grads_drop(m, obs, act, None, w, (SEED, STEP))
    c = hip_grads_drop(m, obs, act, None, w, (SEED, STEP + 1))
    d = hip_grads_drop(m, obs, act, None, w, (SEED + 1, STEP))
    for x, y, z, u in zip(a, b, c, d):
        assert np.array_equal(x, y) and not np.array_equal(x, z) and not np.array_equal(x, u)
    m.train()
    m.set_dropout_seed(SEED, STEP)
    q0, g0, d0 = hip_grads(m, obs, act, None, w)
    q1, g1, d1 = hip_grads(m, obs, act, None, w)
    assert m._drop_step == STEP + 2
    assert np.array_equal(q0, a[0]) and np.array_equal(g0, a[1]) and np.array_equal(d0, a[2])
    assert np.array_equal(q1, c[0]) and np.array_equal(g1, c[1]) and np.array_equal(d1, c[2])
    # the same seed and the same calls again: the same bits
    m.set_dropout_seed(SEED, STEP)
    again = hip_grads(m, obs, act, None, w), hip_grads(m, obs, act, None, w)
    for x, y in zip(again[0] + again[1], (q0, g0, d0, q1, g1, d1)):
        assert np.array_equal(x, y)


def test_two_forwards_one_backward(emu):
    """Each forward's backward recomputes the masks of its own (seed, step), whatever ran in between."""
    cfg, _, m = rowblock_module(emu)
    obs1, act1, _, w1 = make_inputs(cfg, BATCH, 20, seed=5)
    obs2, act2, _, w2 = make_inputs(cfg, BATCH, 13, seed=6)
    _, g1, _ = hip_grads_drop(m, obs1, act1, None, w1, (SEED, 0))
    _, g2, _ = hip_grads_drop(m, obs2, act2, None, w2, (SEED, 1))
    m.train()
    m.set_dropout_seed(SEED)
    m.zero_grad(set_to_none=True)
    qa = m(torch.as_tensor(obs1), torch.as_tensor(act1))
    qb = m(torch.as_tensor(obs2), torch.as_tensor(act2))
    assert qa.grad_fn.dropout_keys == (SEED, 0) and qb.grad_fn.dropout_keys == (SEED, 1)
    ((qa * torch.as_tensor(w1)).sum() + (qb * torch.as_tensor(w2)).sum()).backward()
    assert np.array_equal(flat_grad(m), g1 + g2)


@pytest.mark.parametrize("over", [dict(), dict(bag_size=5), dict(gate="gru")])
def test_no_keys_means_no_dropout_bit_for_bit(emu, over):
    """eval(), and a train-mode module on which set_dropout_seed was never called: the forward of the same weights at dropout 0."""
    cfg, params, m = rowblock_module(emu, **over)
    plain = make_module(emu, O.NetCfg(**{**ROWBLOCK, **over, "dropout": 0.0}), params)
    obs, act, bag, w = make_inputs(cfg, BATCH, 20, seed=5)
    ref = hip_grads(plain, obs, act, bag, w)
    kwb = {} if bag is None else dict(bag_obss=torch.as_tensor(bag[0]), bag_actions=torch.as_tensor(bag[1]))
    m.train()
    never = hip_grads(m, obs, act, bag, w)
    m.set_dropout_seed(SEED)
    m.eval()
    ev = hip_grads(m, obs, act, bag, w)
    assert m._drop_step == 0                        # eval forwards leave the counter alone
    with torch.no_grad():
        q_ng = m(torch.as_tensor(obs), torch.as_tensor(act), **kwb).numpy()
    m.train()
    m.set_dropout_seed(None)
    off = hip_grads(m, obs, act, bag, w)
    for got in (never, ev, off):
        for x, y in zip(got, ref):
            assert np.array_equal(x, y)
    assert np.array_equal(q_ng, ref[0])
    m.set_dropout_seed(SEED)
    assert not np.array_equal(hip_grads(m, obs, act, bag, w)[0], ref[0])


@pytest.mark.parametrize("over", [dict(), dict(bag_size=5), dict(identity=True)])
def test_differentiable_and_no_grad_forward_draw_the_same_masks(emu, over):
    cfg, _, m = rowblock_module(emu, **over)
    obs, act, bag, w = make_inputs(cfg, BATCH, 20, seed=5)
    kwb = {} if bag is None else dict(bag_obss=torch.as_tensor(bag[0]), bag_actions=torch.as_tensor(bag[1]))
    q = hip_grads_drop(m, obs, act, bag, w, (SEED, STEP))[0]
    with torch.no_grad():
        q_ng = m(torch.as_tensor(obs), torch.as_tensor(act), _train_dropout=(SEED, STEP), **kwb)
        assert q_ng.grad_fn is None and np.array_equal(q_ng.numpy(), q)
        # the module's own counter: call k of either path draws the masks of step k
        m.train()
        m.set_dropout_seed(SEED, STEP - 1)
        first = m(torch.as_tensor(obs), torch.as_tensor(act), **kwb).numpy()
        second = m(torch.as_tensor(obs), torch.as_tensor(act), **kwb).numpy()
    assert not np.array_equal(first, q) and np.array_equal(second, q)


def embedding_keep_count(m, cfg, Bn, n, keys):
    """Kept / all elements of x0 = dropout(embedding + position) in the records of one forward (a dropped element is exactly 0)."""
    obs, act, _, _ = make_inputs(cfg, Bn, n, seed=9)
    runner = _GradRunner(m, torch.as_tensor(obs), torch.as_tensor(act), None, None, keys)
    runner.forward()
    net = runner.net
    rec = runner.ws.cpu().numpy()[:Bn * net.act_stride].reshape(Bn, net.act_stride)
    off = net.ao_layer0 + net.al_u1                 # post-LN layers read their input, x0, from u1 of layer 0
    x0 = rec[:, off:off + net.lp * net.d_model].reshape(Bn, net.lp, net.d_model)
    return int(np.count_nonzero(x0[:, :n])), Bn * n * net.d_model


def test_keep_rate(emu):
    p = 0.1
    cfg = O.NetCfg(obs_dim=4, num_actions=4, inner_embed_size=128, num_heads=8, num_layers=1, history_len=50, dropout=p)
    m = make_module(emu, cfg, O.init_params(cfg, seed=3, perturb=True))
    kept, total = embedding_keep_count(m, cfg, 8, 50, (SEED, STEP))
    sigma = math.sqrt(total * p * (1 - p))
    assert total == 8 * 50 * 128 and abs(kept - total * (1 - p)) <= 4 * sigma, (kept, total)
    assert embedding_keep_count(m, cfg, 8, 50, None)[0] == total


def test_optimiser_loop(emu):
    """Adam + clip_grad_norm_ on the module with its own dropout counter: finite, moves theta, and a second run repeats it."""
    def run():
        cfg, _, m = rowblock_module(emu, num_layers=1)
        m.train()
        m.set_dropout_seed(SEED)
        theta0 = m.flat.detach().clone()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        obs, act, _, w = make_inputs(cfg, BATCH, 20, seed=5)
        target = torch.as_tensor(w)
        for _ in range(5):
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.smooth_l1_loss(m(torch.as_tensor(obs), torch.as_tensor(act)), target)
            assert torch.isfinite(loss)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(m.parameters(), 1.0, error_if_nonfinite=True)
            opt.step()
        assert m._drop_step == 5 and not torch.equal(m.flat, theta0)
        return m.flat.detach().clone()
    assert torch.equal(run(), run())


# ------------------------------------------------------------------------------------------ the entry points that keep their signatures
def test_plain_entry_points_give_the_parents_bits(emu):
    """dtqn_forward_train / dtqn_backward_dq, now calls of the _drop forms with the masks off, against Q, grad and dobs dumped from
    the commit before them on this emulation (tests/golden/autograd_parent_bits.npz; a dropout = 0.1 network, so "off" is what is
    tested), and the _drop forms with step -1."""
    z = np.load(os.path.join(GOLDEN, "autograd_parent_bits.npz"))
    cfg = O.NetCfg(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=70, action_dim=4, dropout=0.1)
    Bn, n = 2, 33
    m = make_module(emu, cfg, O.init_params(cfg, seed=3, perturb=True))
    net = m.net
    obs, act, _, w = make_inputs(cfg, Bn, n, seed=5)
    o, a = np.ascontiguousarray(obs, dtype=np.float32), np.ascontiguousarray(act.reshape(Bn, n), dtype=np.uint8)
    theta, w = m.flat.numpy(), np.ascontiguousarray(w)
    size = emu.dtqn_grad_workspace_floats(ctypes.byref(net), Bn, n)

    def run(fwd, bwd):
        ws = np.zeros(size, np.float32)
        q = np.zeros((Bn, n, cfg.num_actions), np.float32)
        g, dobs = np.full(net.n_trainable, np.nan, np.float32), np.full(o.shape, np.nan, np.float32)
        assert fwd(ws, q) == 0 and bwd(ws, g, dobs) == 0
        return q, g, dobs
    nb = ctypes.byref(net)
    plain = run(lambda ws, q: emu.dtqn_forward_train(nb, ptr(theta), ptr(o), ptr(a), None, None, Bn, n, ptr(q), ptr(ws), None),
                lambda ws, g, d: emu.dtqn_backward_dq(nb, ptr(theta), ptr(o), ptr(a), None, None, Bn, n, ptr(w), ptr(ws), ptr(g), ptr(d), None))
    off = run(lambda ws, q: emu.dtqn_forward_train_drop(nb, ptr(theta), ptr(o), ptr(a), None, None, Bn, n, ptr(q), ptr(ws), SEED, -1, None),
              lambda ws, g, d: emu.dtqn_backward_dq_drop(nb, ptr(theta), ptr(o), ptr(a), None, None, Bn, n, ptr(w), ptr(ws), ptr(g), ptr(d),
                                                         SEED, -1, None))
    on = run(lambda ws, q: emu.dtqn_forward_train_drop(nb, ptr(theta), ptr(o), ptr(a), None, None, Bn, n, ptr(q), ptr(ws), SEED, 0, None),
             lambda ws, g, d: emu.dtqn_backward_dq_drop(nb, ptr(theta), ptr(o), ptr(a), None, None, Bn, n, ptr(w), ptr(ws), ptr(g), ptr(d),
                                                        SEED, 0, None))
    for got in (plain, off):
        assert np.array_equal(got[0], z["q"]) and np.array_equal(got[1], z["grad"]) and np.array_equal(got[2], z["dobs"])
    assert not np.array_equal(on[0], z["q"]) and np.isfinite(on[1]).all() and np.isfinite(on[2]).all()
    assert emu.dtqn_abi_version() == B.DEFINES["DTQN_ABI_VERSION"] == 21


def test_pad_rows_take_no_part_under_dropout(emu):
    """A prefix of n < L rows under dropout: NaN in every activation / gradient record of the workspace, pad rows n .. LP - 1
    included, changes no bit of Q, grad or dobs.  (That the live rows' masks are right, the embedding mask on dobs included, is the
    cfg1_prefix parity case: the oracle masks the embedding before anything reads it.)"""
    kw, n = CASES["cfg1_prefix"]
    cfg = O.NetCfg(**kw)
    m = make_module(emu, cfg, O.init_params(cfg, seed=3, perturb=True))
    net = m._grad_net()
    obs, act, _, w = make_inputs(cfg, BATCH, n, seed=5)
    o, a = np.ascontiguousarray(obs), np.ascontiguousarray(act.reshape(BATCH, n), dtype=np.uint8)
    theta, w = m.flat.numpy(), np.ascontiguousarray(w)
    size = emu.dtqn_grad_workspace_floats(ctypes.byref(net), BATCH, n)

    def run(ws):
        q = np.zeros((BATCH, n, cfg.num_actions), np.float32)
        g, dobs = np.zeros(net.n_trainable, np.float32), np.full(o.shape, np.nan, np.float32)
        assert emu.dtqn_forward_train_drop(ctypes.byref(net), ptr(theta), ptr(o), None, None, None, BATCH, n, ptr(q), ptr(ws), SEED, STEP, None) == 0
        assert emu.dtqn_backward_dq_drop(ctypes.byref(net), ptr(theta), ptr(o), None, None, None, BATCH, n, ptr(w), ptr(ws), ptr(g), ptr(dobs),
                                         SEED, STEP, None) == 0
        return q, g, dobs
    clean = run(np.zeros(size, np.float32))
    ws = np.zeros(size, np.float32)
    ws[:BATCH * (net.act_stride + net.grd_stride)] = np.nan
    for x, y in zip(clean, run(ws)):
        assert np.isfinite(x).all() and np.array_equal(x, y)
