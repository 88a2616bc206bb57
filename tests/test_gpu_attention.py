"""-m gpu: attention capture (DTQN(..., capture_attention=True), tl_alpha_kernel / tl_bag_alpha_kernel) on the MI355X -- the reference's
own weights (G13), torch.nn.MultiheadAttention's head-averaged weights built from the oracle's parameters at config 5 shapes (key-blocked
at L = 256 / 512), d_model 256 with head width 128, head width 4 and a bag network, and the agent's acting forward."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import dtqn_oracle as O

from attention_helpers import capture_module, captured, check_weights, g13, g13_case, g13_names, tensors
from autograd_helpers import make_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    torch.cuda.set_device(0)
    return engine.get_lib()


@pytest.fixture(scope="module")
def z():
    with g13() as f:
        yield {k: f[k] for k in f.files}


@pytest.mark.parametrize("name", g13_names())
def test_weights_match_the_reference_on_device(lib, z, name):
    cfg, params, inputs, q_ref, ref_alphas, ref_bag = g13_case(z, name)
    m = capture_module(None, cfg, params, device="cuda")
    q = m(**tensors(inputs, "cuda"))
    assert np.abs(q.cpu().numpy() - q_ref).max() <= 1e-4 * max(1.0, float(np.abs(q_ref).max()))
    alphas, bag = captured(m)
    check_weights(alphas, bag, ref_alphas, ref_bag, f64=(cfg, params, inputs))
    assert all(layer.alpha.device.type == "cuda" for layer in m.transformer_layers)
    m.set_capture_attention(False)
    assert torch.equal(q, m(**tensors(inputs, "cuda")))
    m.set_capture_attention(True)
    m(**tensors(inputs, "cuda"))
    again, bag2 = captured(m)
    assert all(np.array_equal(a, b) for a, b in zip(alphas, again))
    assert bag is None or np.array_equal(bag, bag2)


def mha_weights(cfg, params, obs, act, bag):
    """Every layer's torch.nn.MultiheadAttention(batch_first=True) weights with average_attn_weights=True, and the bag attention's, on
    the attention inputs of the oracle's forward (CPU, float32)."""
    alphas, bagw = [], []
    orig_mha, orig_cross = O.mha, O.cross_attention

    def module(D, H, w_in, b_in, w_out, b_out):
        mod = nn.MultiheadAttention(D, H, batch_first=True)
        with torch.no_grad():
            mod.in_proj_weight.copy_(w_in); mod.in_proj_bias.copy_(b_in)
            mod.out_proj.weight.copy_(w_out); mod.out_proj.bias.copy_(b_out)
        return mod.eval()

    def mha(x, w_in, b_in, w_out, b_out, H, *args, **kw):
        n = x.shape[1]
        _, w = module(x.shape[-1], H, w_in, b_in, w_out, b_out)(x, x, x, attn_mask=O.causal_mask(n), average_attn_weights=True)
        alphas.append(w.detach().numpy())
        return orig_mha(x, w_in, b_in, w_out, b_out, H, *args, **kw)

    def cross(x, mem, w_in, b_in, w_out, b_out, H, *args, **kw):
        _, w = module(x.shape[-1], H, w_in, b_in, w_out, b_out)(x, mem, mem)
        bagw.append(w.detach().numpy())
        return orig_cross(x, mem, w_in, b_in, w_out, b_out, H, *args, **kw)

    O.mha, O.cross_attention = mha, cross
    try:
        kw = {}
        if bag is not None:
            kw = dict(bag_obss=torch.as_tensor(bag[0]).long() if cfg.discrete else torch.as_tensor(bag[0]), bag_actions=torch.as_tensor(bag[1]))
        with torch.no_grad():
            O.forward(params, cfg, torch.as_tensor(obs).long() if cfg.discrete else torch.as_tensor(obs), torch.as_tensor(act), **kw)
    finally:
        O.mha, O.cross_attention = orig_mha, orig_cross
    return alphas, (bagw[0] if bagw else None)


CFG5 = dict(obs_dim=1, num_actions=5, inner_embed_size=256, num_heads=8, num_layers=2, history_len=256, discrete=True, vocab_sizes=22)
# (name, network, batch, rows)
MHA_CASES = [
    ("cfg5_L256", CFG5, 2, 256),
    ("cfg5_L512", dict(CFG5, history_len=512), 2, 512),
    ("cfg5_L512_prefix", dict(CFG5, history_len=512), 2, 333),
    ("d256_hd128", dict(obs_dim=4, num_actions=3, inner_embed_size=256, num_heads=2, num_layers=1, history_len=200), 2, 200),
    ("hd4", dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=16, num_layers=2, history_len=70), 3, 70),
    ("bag", dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50, action_dim=4, bag_size=6), 3, 50),
]


@pytest.mark.parametrize("name,kw,Bn,n", MHA_CASES, ids=[c[0] for c in MHA_CASES])
def test_weights_match_multihead_attention(lib, name, kw, Bn, n):
    cfg = O.NetCfg(**kw)
    params = O.init_params(cfg, seed=11, perturb=True)
    if cfg.inner_embed_size >= 256:      # (as tests/test_gpu_autograd.py: matrices at a quarter of the perturbed scale at d_model 256)
        params = {k: (v * 0.25 if v.dim() == 2 and not k.endswith(("attn_mask", "position_encoding")) else v) for k, v in params.items()}
    obs, act, bag, _ = make_inputs(cfg, Bn, n, seed=7)
    ref_alphas, ref_bag = mha_weights(cfg, params, obs, act, bag)
    m = capture_module(None, cfg, params, device="cuda")
    kwb = {} if bag is None else dict(bag_obss=torch.as_tensor(bag[0], device="cuda"), bag_actions=torch.as_tensor(bag[1], device="cuda"))
    q = m(torch.as_tensor(obs, device="cuda"), torch.as_tensor(act, device="cuda"), **kwb)
    alphas, bagw = captured(m)
    check_weights(alphas, bagw, ref_alphas, ref_bag,
                  f64=(cfg, params, dict(obss=obs, actions=act, **({} if bag is None else dict(bag_obss=bag[0], bag_actions=bag[1])))))
    m.set_capture_attention(False)
    assert torch.equal(q, m(torch.as_tensor(obs, device="cuda"), torch.as_tensor(act, device="cuda"), **kwb))


def test_agent_get_action_captures_the_acting_context(lib):
    from dtqn_amd import envs
    from dtqn_amd.utils.agent_utils import get_agent
    from dtqn_amd.utils.random import set_global_seed
    env = envs.make("DiscreteCarFlag-v0")
    set_global_seed(3, env)
    agent = get_agent("DTQN", [env], 8, 0, 64, 20_000, torch.device("cuda"), 3e-4, 32, 50, -1, 50, 1000, 0.99, 8, 2, 0.0,
                      False, "res", "learned", 0)
    net = agent.policy_network
    net.set_capture_attention(True)
    agent.context_reset(env.reset())
    for step in range(12):
        a = agent.get_action(epsilon=0.0)
        ctx = agent.context
        n = min(ctx.max_length, ctx.timestep + 1)
        alphas = [layer.alpha.clone() for layer in net.transformer_layers]
        assert all(x.shape == (1, n, n) for x in alphas)
        q = net(torch.as_tensor(ctx.obs[None, :n], dtype=agent.obs_tensor_type, device="cuda"),
                torch.as_tensor(ctx.action[None, :n], dtype=torch.long, device="cuda"))
        assert a == int(torch.argmax(q[0, -1]).item())
        assert all(torch.equal(x, layer.alpha) for x, layer in zip(alphas, net.transformer_layers))
        obs, r, done, _ = env.step(a)
        agent.observe(obs, a, r, done)
        if done:
            break
