"""-m gpu: the differentiable forward (DTQN(..., autograd=True)) on the MI355X -- parameter / observation gradients of a loss written in
torch against the oracle at BASELINE config 1-5 shapes, full per-GPU batches at config 3 / 5 shapes, and the gradient of the reference's
TD loss written in torch against the fused TD update's own gradient on the same windows."""
import numpy as np
import pytest
import torch

from oracle import dtqn_oracle as O

from autograd_helpers import check_against_oracle, hip_grads, make_inputs, make_module
from helpers import make_td_case, oracle_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    torch.cuda.set_device(0)
    return engine.get_lib()


CFG = {
    1: dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50),
    3: dict(obs_dim=10, num_actions=10, inner_embed_size=128, num_heads=8, num_layers=2, history_len=50, discrete=True, vocab_sizes=9),
    4: dict(obs_dim=6, num_actions=6, inner_embed_size=128, num_heads=8, num_layers=2, history_len=128, discrete=True, vocab_sizes=12),
    5: dict(obs_dim=1, num_actions=5, inner_embed_size=256, num_heads=8, num_layers=2, history_len=256, discrete=True, vocab_sizes=22),
}

# (name, network, batch, rows): reduced batches
CASES = [
    ("cfg1", CFG[1], 4, 50),
    ("cfg1_prefix", CFG[1], 3, 17),
    ("cfg2_continuous_action_embedding", dict(CFG[1], action_dim=8, pos="sin"), 4, 50),
    ("cfg3", CFG[3], 4, 50),
    ("cfg3_continuous", dict(CFG[3], discrete=False, vocab_sizes=0), 4, 50),
    ("cfg4", CFG[4], 2, 128),
    ("cfg4_prefix", CFG[4], 2, 77),
    ("cfg5", CFG[5], 2, 256),
    ("d256_h8_L512", dict(CFG[5], history_len=512), 1, 512),
    ("gru_identity", dict(CFG[1], gate="gru", identity=True, action_dim=8), 3, 50),
    ("padded_48_6", dict(obs_dim=3, num_actions=3, inner_embed_size=48, num_heads=6, num_layers=2, history_len=20), 3, 20),
    ("bag", dict(CFG[1], bag_size=6, action_dim=4), 3, 50),
]


@pytest.mark.parametrize("name,kw,Bn,n", CASES, ids=[c[0] for c in CASES])
def test_gradients_match_the_oracle_on_device(lib, name, kw, Bn, n):
    cfg = O.NetCfg(**kw)
    params = O.init_params(cfg, seed=3, perturb=True)
    if cfg.inner_embed_size >= 256:
        # d_model 256 at std-0.2 weights puts |Q| in the thousands and fp32 rounding flips ReLUs whose pre-activation sits at the kink
        # (the gradient is discontinuous there): matrices at a quarter of that scale, biases / LayerNorms / positions still perturbed
        params = {k: (v * 0.25 if v.dim() == 2 and not k.endswith(("attn_mask", "position_encoding")) else v) for k, v in params.items()}
    m = make_module(None, cfg, params, device="cuda")
    obs, act, bag, w = make_inputs(cfg, Bn, n, seed=5)
    q, _, _ = check_against_oracle(m, cfg, params, obs, act, bag, w, device="cuda")
    kwb = {} if bag is None else dict(bag_obss=torch.as_tensor(bag[0], device="cuda"), bag_actions=torch.as_tensor(bag[1], device="cuda"))
    with torch.no_grad():
        q0 = m(torch.as_tensor(obs, device="cuda"), torch.as_tensor(act, device="cuda"), **kwb).cpu().numpy()
    assert np.array_equal(q, q0)


@pytest.mark.parametrize("c,Bn", [(3, 512), (5, 32)])
def test_full_batch_is_finite_and_deterministic(lib, c, Bn):
    cfg = O.NetCfg(**CFG[c])
    m = make_module(None, cfg, O.init_params(cfg, seed=3, perturb=False), device="cuda")
    obs, act, bag, w = make_inputs(cfg, Bn, cfg.history_len, seed=5)
    a = hip_grads(m, obs, act, bag, w, device="cuda")
    b = hip_grads(m, obs, act, bag, w, device="cuda")
    assert np.isfinite(a[1]).all() and np.abs(a[1]).max() > 0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("c,Bn", [(1, 8), (4, 4)])
def test_torch_td_loss_matches_the_fused_update(lib, c, Bn):
    """The windows one fused TD update drew, fed to the reference's loss written in torch on the module (dtqn/agents/dtqn.py:215-256):
    the autograd gradient is the update's own td.grad."""
    cfg = O.NetCfg(**CFG[c])
    L = cfg.history_len
    mask = cfg.vocab_sizes - 1 if cfg.discrete else -5
    net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=7, batch=Bn, T=L + 40, n_eps=12, mask=mask, device="cuda", test_lib=False)
    eps, starts = host.sample_indices(Bn)
    eng.set_indices(eps, starts)
    eng.forward_backward(rep)
    fused = eng.grad.cpu().numpy()[:net.n_trainable].copy()
    batch = oracle_batch(host, eps, starts, cfg.discrete)
    pol = make_module(None, cfg, oracle.pol, device="cuda")
    tgt = make_module(None, cfg, oracle.tgt, device="cuda", autograd=False)
    with torch.no_grad():
        pol.flat[:net.n_trainable].copy_(eng.theta_pol[:net.n_trainable])
        tgt.flat[:net.n_trainable].copy_(eng.theta_tgt[:net.n_trainable])
    dev = torch.device("cuda")
    obss, actions = batch.obss.to(dev), batch.actions.to(dev)
    next_obss, next_actions = batch.next_obss.to(dev), batch.next_actions.to(dev)
    rewards, dones = batch.rewards.to(dev), batch.dones.to(dev)
    q_values = pol(obss, actions).gather(2, actions).squeeze()
    with torch.no_grad():
        argmax = torch.argmax(pol(next_obss, next_actions), dim=2).unsqueeze(-1)
        next_q = tgt(next_obss, next_actions).gather(2, argmax).squeeze()
        targets = rewards.squeeze() + (1 - dones.squeeze()) * (next_q * oracle.gamma)
    hist = oracle.history
    loss = torch.nn.functional.mse_loss(q_values[:, -hist:], targets[:, -hist:])
    pol.zero_grad(set_to_none=True)
    loss.backward()
    got = np.zeros(net.n_trainable, np.float32)
    for p, off in pol._grad_params(with_offsets=True):
        got[off:off + p.numel()] = p.grad.reshape(-1).cpu().numpy()
    assert np.abs(got - fused).max() <= 2e-4 * np.abs(fused).max(), (np.abs(got - fused).max(), np.abs(fused).max())
