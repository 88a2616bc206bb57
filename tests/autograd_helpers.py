"""Shared by the autograd tests (tests/test_emu_autograd.py on the CPU emulation, tests/test_gpu_autograd.py on the device): a
DTQN module with oracle weights and the differentiable forward on, random inputs, and the oracle's gradients of the same loss."""
import numpy as np
import torch

from dtqn_amd.networks.dtqn import DTQN
from oracle import dtqn_oracle as O

from grad_f64_helpers import check_gradient_f64
from helpers import flat_from_params, pack_theta, padding_mask, relu_masks
from q_f64_helpers import check_forward_f64


def make_module(lib, cfg: O.NetCfg, params, device="cpu", autograd=True) -> DTQN:
    m = DTQN(cfg.obs_dim, cfg.num_actions, cfg.embed_per_obs_dim, cfg.action_dim, cfg.inner_embed_size, cfg.num_heads, cfg.num_layers,
             cfg.history_len, dropout=cfg.dropout, gate=cfg.gate, identity=cfg.identity, pos=cfg.pos, discrete=cfg.discrete,
             vocab_sizes=cfg.vocab_sizes if cfg.discrete else None, bag_size=cfg.bag_size, autograd=autograd, _test_lib=lib)
    if device == "cpu":
        m._allow_cpu = True
    else:
        m = m.to(device)
    with torch.no_grad():
        m.flat.copy_(torch.from_numpy(pack_theta(m.net, params)))
    return m


def make_inputs(cfg: O.NetCfg, Bn: int, n: int, seed: int):
    """obss (float, or integer tokens as float), actions [B, n, 1], bag (or None), loss weights w [B, n, A]."""
    rng = np.random.default_rng(seed)
    if cfg.discrete:
        obs = rng.integers(0, cfg.vocab_sizes, size=(Bn, n, cfg.obs_dim)).astype(np.float32)
    else:
        obs = rng.uniform(-1, 1, size=(Bn, n, cfg.obs_dim)).astype(np.float32)
    act = rng.integers(0, cfg.num_actions, size=(Bn, n, 1))
    bag = None
    if cfg.bag_size > 0:
        bo = rng.integers(0, cfg.vocab_sizes, size=(Bn, cfg.bag_size, cfg.obs_dim)).astype(np.float32) if cfg.discrete \
            else rng.uniform(-1, 1, size=(Bn, cfg.bag_size, cfg.obs_dim)).astype(np.float32)
        bag = (bo, rng.integers(0, cfg.num_actions, size=(Bn, cfg.bag_size, 1)))
    w = rng.standard_normal((Bn, n, cfg.num_actions)).astype(np.float32)
    return obs, act, bag, w


def forward_masks(q, num_layers: int, width: int):
    """The ReLU activation patterns in the records of the differentiable forward that produced q (read before its backward, which
    releases them): what helpers.engine_probe reads from a TD engine, for the oracle evaluations conditional on them."""
    r = q.grad_fn.runner
    act = r.ws[:r.Bn * r.net.act_stride].cpu().numpy().reshape(r.Bn, r.net.act_stride)
    return relu_masks(O.NetCfg(obs_dim=0, num_actions=0, inner_embed_size=width, num_layers=num_layers), r.net, act, r.n)


def hip_grads(m: DTQN, obs, act, bag, w, device="cpu", masks_out=None):
    """q, flat parameter gradient (engine layout, trainable region) and obss.grad (None for tokens) of loss = (q * w).sum().
    masks_out: a list that receives the forward's ReLU patterns (forward_masks)."""
    o = torch.tensor(obs, device=device, requires_grad=not m.discrete)
    a = torch.as_tensor(act, device=device)
    kw = {}
    if bag is not None:
        kw = dict(bag_obss=torch.as_tensor(bag[0], device=device), bag_actions=torch.as_tensor(bag[1], device=device))
    m.zero_grad(set_to_none=True)
    q = m(o, a, **kw)
    assert q.requires_grad and q.grad_fn is not None
    if masks_out is not None:
        masks_out.extend(forward_masks(q, m.net.num_layers, m.net.d_real or m.net.d_model))
    (q * torch.as_tensor(w, device=device)).sum().backward()
    flat = torch.zeros(m.net.n_trainable, dtype=torch.float32)
    for p, off in m._grad_params(with_offsets=True):
        flat[off:off + p.numel()] = p.grad.detach().reshape(-1).cpu()
    return q.detach().cpu().numpy(), flat.numpy(), (None if o.grad is None else o.grad.cpu().numpy())


def oracle_grads(cfg: O.NetCfg, params, obs, act, bag, w, probe=None, dtype=torch.float32):
    """The same loss through oracle.forward and torch.autograd.grad: q, {canonical key: grad}, d loss / d obss (continuous).
    probe: {"masks": [...]} evaluates it under another implementation's ReLU patterns (the list is consumed); dtype float64: the
    float32 parameters and inputs widened exactly, every operation in double."""
    keys = O.trainable_keys(cfg)
    params = {k: v.to(dtype) if v.dtype == torch.float32 else v for k, v in params.items()}
    leaves = {k: params[k].detach().clone().requires_grad_(True) for k in keys}
    p2 = {k: leaves.get(O.canonical_key(cfg, k), params[k]) for k in O.state_dict_keys(cfg)}
    o = torch.tensor(obs, dtype=dtype, requires_grad=True) if not cfg.discrete else torch.as_tensor(obs).long()
    kw = {}
    if bag is not None:
        kw = dict(bag_obss=torch.as_tensor(bag[0]).long() if cfg.discrete else torch.as_tensor(bag[0], dtype=dtype),
                  bag_actions=torch.as_tensor(bag[1]))
    q = O.forward(p2, cfg, o, torch.as_tensor(act), probe, **kw)
    loss = (q * torch.as_tensor(w).to(dtype)).sum()
    wrt = [leaves[k] for k in keys] + ([o] if not cfg.discrete else [])
    g = torch.autograd.grad(loss, wrt)
    grads = dict(zip(keys, g))
    return q.detach().numpy(), grads, (g[-1].numpy() if not cfg.discrete else None)


def check_against_oracle(m: DTQN, cfg, params, obs, act, bag, w, device="cpu", rtol=2e-4):
    masks = []
    q, got, dobs = hip_grads(m, obs, act, bag, w, device, masks_out=masks)
    q_ref, grads, dobs_ref = oracle_grads(cfg, params, obs, act, bag, w)
    qmax = float(np.abs(q_ref).max())
    assert np.abs(q - q_ref).max() <= 1e-4 * max(1.0, qmax), (np.abs(q - q_ref).max(), qmax)
    check_forward_f64(cfg, params, obs, act, q, bag=bag, what="differentiable forward")      # ... and row by row against float64
    ref = flat_from_params(m.net, grads, O.trainable_keys(cfg))
    err = np.abs(got - ref).max()
    assert err <= rtol * np.abs(ref).max(), (err, np.abs(ref).max())
    pad = padding_mask(m.net)
    if pad.any():                           # width-padded network: no gradient in the padding
        assert not got[pad].any()
    if dobs_ref is not None:
        assert dobs is not None
        derr = np.abs(dobs - dobs_ref).max()
        assert derr <= rtol * np.abs(dobs_ref).max(), (derr, np.abs(dobs_ref).max())
    check_f64_under_masks(cfg, m.net, got, masks, qmax, lambda probe, dtype: oracle_grads(cfg, params, obs, act, bag, w, probe, dtype)[1])
    return q, got, dobs


def check_f64_under_masks(cfg, net, got, masks, qmax, grads_of, what=None):
    """The float64 gradient check (grad_f64_helpers.py) of a differentiable forward: grads_of(probe, dtype) evaluates the oracle under
    the kernels' own ReLU patterns, once in fp32 (the yardstick) and once in float64; the patterns may differ from the oracle's own
    only where check_td_updates lets them (a few units, at pre-activations within rounding of the kink)."""
    import time
    from grad_f64_helpers import TOTALS
    t0 = time.perf_counter()
    p32, p64 = {"masks": list(masks)}, {"masks": list(masks)}
    g32, g64 = grads_of(p32, torch.float32), grads_of(p64, torch.float64)
    TOTALS[0] += time.perf_counter() - t0
    TOTALS[1] += 1
    assert not p32["masks"] and not p64["masks"], "oracle consumed fewer ReLU masks than the forward saved"
    n_relu = sum(int(x.numel()) for x in masks)
    for p in (p32, p64):
        assert p.get("relu_flips", 0) <= max(2, n_relu // 20000), p
        assert p.get("max_flip_preact", 0.0) <= 2e-5 * max(1.0, qmax), p
    return check_gradient_f64(cfg, net, got, g64, g32, what=what)
