"""The differentiable forward (DTQN(..., autograd=True), dtqn_forward_train + dtqn_backward_dq) on the CPU emulation of the HIP sources:
parameter and observation gradients of a loss written in torch against torch.autograd through the oracle's forward, Q against the
no-grad forward bit for bit, determinism, and one TD step of the reference written in plain torch on the module."""
import ctypes

import numpy as np
import pytest
import torch

from dtqn_amd import _binding as B
from oracle import dtqn_oracle as O

from autograd_helpers import check_against_oracle, hip_grads, make_inputs, make_module
from helpers import flat_from_params, ptr


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


# (network, batch, rows)
CASES = {
    "cfg1_twin": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50), 2, 50),
    "action_embedding": (dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=70, action_dim=4), 2, 70),
    "discrete": (dict(obs_dim=6, num_actions=5, inner_embed_size=64, num_heads=2, num_layers=1, history_len=12, discrete=True, vocab_sizes=9,
                      action_dim=8), 3, 12),
    "gru": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=4, num_layers=2, history_len=20, gate="gru"), 2, 20),
    "identity": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=4, num_layers=2, history_len=70, identity=True), 2, 70),
    "pos_sin": (dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=70, action_dim=4, pos="sin"), 2, 70),
    "pos_none": (dict(obs_dim=4, num_actions=3, inner_embed_size=128, num_heads=8, num_layers=1, history_len=70, pos="none"), 2, 70),
    "padded_48_6": (dict(obs_dim=3, num_actions=3, inner_embed_size=48, num_heads=6, num_layers=2, history_len=20, pos="sin"), 2, 20),
    "padded_96_1": (dict(obs_dim=3, num_actions=3, inner_embed_size=96, num_heads=1, num_layers=1, history_len=40), 2, 40),
    "bag": (dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=20, action_dim=4, bag_size=4), 2, 20),
    "kblock_d128_h1": (dict(obs_dim=4, num_actions=4, inner_embed_size=128, num_heads=1, num_layers=1, history_len=140), 1, 140),
    "prefix": (dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=70, action_dim=4), 2, 33),
    "prefix_one_row": (dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=20, action_dim=4), 3, 1),
    "prefix_bag": (dict(obs_dim=5, num_actions=3, inner_embed_size=64, num_heads=2, num_layers=1, history_len=20, discrete=True, vocab_sizes=7,
                        action_dim=4, bag_size=3), 2, 9),
}


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_match_the_oracle(emu, name):
    kw, Bn, n = CASES[name]
    cfg = O.NetCfg(**kw)
    params = O.init_params(cfg, seed=3, perturb=True)
    m = make_module(emu, cfg, params)
    obs, act, bag, w = make_inputs(cfg, Bn, n, seed=5)
    q, _, _ = check_against_oracle(m, cfg, params, obs, act, bag, w)
    # the differentiable forward returns what the no-grad forward returns, bit for bit
    kwb = {} if bag is None else dict(bag_obss=torch.as_tensor(bag[0]), bag_actions=torch.as_tensor(bag[1]))
    with torch.no_grad():
        q0 = m(torch.as_tensor(obs), torch.as_tensor(act), **kwb)
    assert np.array_equal(q, q0.numpy())


def test_off_by_default(emu):
    cfg = O.NetCfg(**CASES["action_embedding"][0])
    params = O.init_params(cfg, seed=3, perturb=True)
    m = make_module(emu, cfg, params, autograd=False)
    obs, act, _, _ = make_inputs(cfg, 2, 10, seed=1)
    q = m(torch.as_tensor(obs), torch.as_tensor(act))
    assert q.grad_fn is None and not q.requires_grad
    m.set_autograd(True)
    q1 = m(torch.as_tensor(obs), torch.as_tensor(act))
    assert q1.grad_fn is not None and np.array_equal(q.numpy(), q1.detach().numpy())
    with torch.no_grad():                                   # grad mode off: today's path
        assert m(torch.as_tensor(obs), torch.as_tensor(act)).grad_fn is None
    m.set_autograd(False)
    assert m(torch.as_tensor(obs), torch.as_tensor(act)).grad_fn is None


def test_frozen_parameters_and_constant_obs_give_no_graph(emu):
    cfg = O.NetCfg(**CASES["gru"][0])
    m = make_module(emu, cfg, O.init_params(cfg, seed=3, perturb=True))
    for p in m.parameters():
        p.requires_grad_(False)
    obs, act, _, _ = make_inputs(cfg, 2, 8, seed=1)
    assert m(torch.as_tensor(obs), torch.as_tensor(act)).grad_fn is None
    # only the observations ask for a gradient
    o = torch.tensor(obs, requires_grad=True)
    m(o, torch.as_tensor(act)).sum().backward()
    assert o.grad is not None and torch.isfinite(o.grad).all()


def test_image_networks_are_refused(emu):
    from dtqn_amd.networks.dtqn import DTQN
    m = DTQN((1, 24, 24), 3, 8, 0, 64, 8, 1, 4, autograd=True, _test_lib=emu)
    m._allow_cpu = True
    with pytest.raises(NotImplementedError, match="image"):
        m(torch.zeros(1, 2, 1, 24, 24, dtype=torch.uint8), torch.zeros(1, 2, 1, dtype=torch.long))


@pytest.mark.parametrize("name", ["gru", "padded_48_6", "bag"])
def test_deterministic(emu, name):
    kw, Bn, n = CASES[name]
    cfg = O.NetCfg(**kw)
    m = make_module(emu, cfg, O.init_params(cfg, seed=3, perturb=True))
    obs, act, bag, w = make_inputs(cfg, Bn, n, seed=5)
    a = hip_grads(m, obs, act, bag, w)
    b = hip_grads(m, obs, act, bag, w)
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(x, y)


def test_graph_survives_other_forwards_and_shorter_prefixes(emu):
    """A forward + backward at seq = L, then at seq = L / 2 on the same module (whose records go to a new workspace), and a graph whose
    backward runs after another forward."""
    kw, Bn, L = CASES["action_embedding"]
    cfg = O.NetCfg(**kw)
    params = O.init_params(cfg, seed=3, perturb=True)
    m = make_module(emu, cfg, params)
    for n in (L, L // 2):
        obs, act, bag, w = make_inputs(cfg, Bn, n, seed=n)
        check_against_oracle(m, cfg, params, obs, act, bag, w)
    obs1, act1, _, w1 = make_inputs(cfg, Bn, L, seed=1)
    obs2, act2, _, w2 = make_inputs(cfg, Bn, L // 2, seed=2)
    ref = hip_grads(m, obs1, act1, None, w1)[1]
    m.zero_grad(set_to_none=True)
    q1 = m(torch.as_tensor(obs1), torch.as_tensor(act1))
    q2 = m(torch.as_tensor(obs2), torch.as_tensor(act2))
    (q1 * torch.as_tensor(w1)).sum().backward()
    got = np.zeros(m.net.n_trainable, dtype=np.float32)
    for p, off in m._grad_params(with_offsets=True):
        got[off:off + p.numel()] = p.grad.reshape(-1).numpy()
    assert np.array_equal(got, ref)
    del q2


def test_pad_rows_take_no_part_whatever_the_workspace_holds(emu):
    """dtqn_backward_dq on a prefix of n rows: the records of rows n .. LP - 1 come from this forward, whatever the workspace held
    before (another call's records, or NaN in every record of the act / grd regions)."""
    kw, Bn, n = CASES["prefix"]
    cfg = O.NetCfg(**kw)
    params = O.init_params(cfg, seed=3, perturb=True)
    m = make_module(emu, cfg, params)
    net = m.net
    obs, act, _, w = make_inputs(cfg, Bn, n, seed=5)
    o = np.ascontiguousarray(obs, dtype=np.float32)
    a = np.ascontiguousarray(act.reshape(Bn, n), dtype=np.uint8)
    theta = m.flat.numpy()

    def run(ws):
        q = np.zeros((Bn, n, cfg.num_actions), np.float32)
        assert emu.dtqn_forward_train(ctypes.byref(net), ptr(theta), ptr(o), ptr(a), None, None, Bn, n, ptr(q), ptr(ws), None) == 0
        g = np.full(net.n_trainable, np.nan, np.float32)
        dobs = np.full(o.shape, np.nan, np.float32)
        assert emu.dtqn_backward_dq(ctypes.byref(net), ptr(theta), ptr(o), ptr(a), None, None, Bn, n, ptr(np.ascontiguousarray(w)), ptr(ws),
                                    ptr(g), ptr(dobs), None) == 0
        return q, g, dobs

    size = emu.dtqn_grad_workspace_floats(ctypes.byref(net), Bn, n)
    assert size > 0
    clean = run(np.zeros(size, np.float32))
    # a workspace a full-length call has used
    ws = np.zeros(size, np.float32)
    ol, al, _, wl = make_inputs(cfg, Bn, cfg.history_len, seed=9)
    ql = np.zeros((Bn, cfg.history_len, cfg.num_actions), np.float32)
    gl = np.zeros(net.n_trainable, np.float32)
    ol, al = np.ascontiguousarray(ol), np.ascontiguousarray(al.reshape(Bn, -1), dtype=np.uint8)
    assert emu.dtqn_forward_train(ctypes.byref(net), ptr(theta), ptr(ol), ptr(al), None, None, Bn, cfg.history_len, ptr(ql), ptr(ws), None) == 0
    assert emu.dtqn_backward_dq(ctypes.byref(net), ptr(theta), ptr(ol), ptr(al), None, None, Bn, cfg.history_len, ptr(np.ascontiguousarray(wl)),
                                ptr(ws), ptr(gl), None, None) == 0
    reused = run(ws)
    # NaN in every activation / gradient record
    ws = np.zeros(size, np.float32)
    ws[:Bn * (net.act_stride + net.grd_stride)] = np.nan
    poisoned = run(ws)
    for r in (reused, poisoned):
        for x, y in zip(clean, r):
            assert np.array_equal(x, y)
    # ... and the result is the oracle's
    _, grads, dobs_ref = __import__("autograd_helpers").oracle_grads(cfg, params, obs, act, None, w)
    ref = flat_from_params(net, grads, O.trainable_keys(cfg))
    assert np.abs(clean[1] - ref).max() <= 2e-4 * np.abs(ref).max()
    assert np.abs(clean[2] - dobs_ref).max() <= 2e-4 * np.abs(dobs_ref).max()


def test_c_abi_refusals(emu):
    from helpers import net_from_cfg
    ws_net = net_from_cfg(emu, O.NetCfg(**CASES["cfg1_twin"][0]))
    assert ws_net.tiled == 0 and emu.dtqn_grad_workspace_floats(ctypes.byref(ws_net), 2, 10) == 0
    x = np.zeros(16, np.float32)
    assert emu.dtqn_forward_train(ctypes.byref(ws_net), ptr(x), ptr(x), None, None, None, 1, 1, ptr(x), ptr(x), None) == B.DEFINES["DTQN_ERR_CONFIG"]
    net = net_from_cfg(emu, O.NetCfg(**CASES["prefix"][0]))
    assert emu.dtqn_grad_workspace_floats(ctypes.byref(net), 2, net.ctx_len + 1) == 0
    assert emu.dtqn_forward_train(ctypes.byref(net), ptr(x), ptr(x), ptr(x), None, None, 1, net.ctx_len + 1, ptr(x), ptr(x), None) == \
        B.DEFINES["DTQN_ERR_ARG"]


def test_reference_td_step_in_plain_torch(emu):
    """DtqnAgent.train() (dtqn/agents/dtqn.py:215-265) written in torch on the module: gather, double-DQN target under no_grad, MSE over
    the last `history` rows, backward, clip_grad_norm_, torch.optim.Adam -- against the oracle's gradients and first Adam step."""
    cfg = O.NetCfg(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=2, history_len=20, action_dim=4)
    pol = O.init_params(cfg, seed=3, perturb=True)
    tgt = O.init_params(cfg, seed=4, perturb=True)
    Bn, L, hist, gamma, lr = 3, cfg.history_len, 7, 0.99, 3e-4
    rng = np.random.default_rng(11)
    obs = torch.as_tensor(rng.uniform(-1, 1, (Bn, L + 1, cfg.obs_dim)).astype(np.float32))
    acts = torch.as_tensor(rng.integers(0, cfg.num_actions, (Bn, L + 1, 1)))
    batch = O.Batch(obss=obs[:, :L], actions=acts[:, :L], rewards=torch.as_tensor(rng.uniform(-1, 1, (Bn, L, 1)).astype(np.float32)),
                    next_obss=obs[:, 1:], next_actions=acts[:, 1:], dones=torch.as_tensor(rng.integers(0, 2, (Bn, L, 1))))
    policy = make_module(emu, cfg, pol)
    target = make_module(emu, cfg, tgt, autograd=False)
    opt = torch.optim.Adam(policy.parameters(), lr=lr)
    # dtqn/agents/dtqn.py:215-265
    q_values = policy(batch.obss, batch.actions)
    q_values = q_values.gather(2, batch.actions).squeeze()
    with torch.no_grad():
        argmax = torch.argmax(policy(batch.next_obss, batch.next_actions), dim=2).unsqueeze(-1)
        next_obs_q_values = target(batch.next_obss, batch.next_actions).gather(2, argmax).squeeze()
        targets = batch.rewards.squeeze() + (1 - batch.dones.squeeze()) * (next_obs_q_values * gamma)
    q_values = q_values[:, -hist:]
    targets = targets[:, -hist:]
    loss = torch.nn.functional.mse_loss(q_values, targets)
    opt.zero_grad(set_to_none=True)
    loss.backward()
    norm = torch.nn.utils.clip_grad_norm_(policy.parameters(), 1.0, error_if_nonfinite=True)
    got = np.zeros(policy.net.n_trainable, np.float32)
    for p, off in policy._grad_params(with_offsets=True):
        got[off:off + p.numel()] = p.grad.reshape(-1).numpy()
    pre = policy.flat.detach().clone().numpy()[:policy.net.n_trainable]
    opt.step()
    post = policy.flat.detach().numpy()[:policy.net.n_trainable]
    # the oracle
    grads, out = O.td_gradients(pol, tgt, cfg, batch, gamma, hist)
    keys = O.trainable_keys(cfg)
    ref = flat_from_params(policy.net, grads, keys)
    ref_norm, coef = O.clip_coef(grads)
    assert abs(float(norm) - ref_norm) <= 2e-4 * ref_norm
    assert np.abs(got / coef - ref).max() <= 2e-4 * np.abs(ref).max()     # p.grad is the clipped gradient
    assert abs(loss.item() - out[0].item()) <= 1e-4 * max(1.0, abs(out[0].item()))
    pol_after = {k: v.clone() for k, v in pol.items()}
    O.adam_step(pol_after, {k: g * coef for k, g in grads.items()}, O.AdamState(keys, pol_after), lr)
    ref_post = flat_from_params(policy.net, pol_after, keys)
    solid = np.abs(ref) >= 1e-3 * np.abs(ref).max()
    assert np.abs(post - ref_post)[solid].max() <= 2e-6
    assert np.abs(post - pre).max() <= 1.001 * lr
