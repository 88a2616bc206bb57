"""Shared by the train-mode dropout tests of the differentiable forward (tests/test_emu_autograd_dropout.py on the CPU emulation,
tests/test_gpu_autograd_dropout.py on the device): the parity cases, the oracle's gradients of a loss under the engine's keep masks
(oracle.DropSpec, the host restatement of dtqn_device.hpp drop_keep), and the flat gradient of a module."""
import numpy as np
import torch

from oracle import dtqn_oracle as O

from autograd_helpers import check_f64_under_masks, forward_masks, hip_grads
from helpers import flat_from_params, padding_mask

SEED, STEP = 12345, 7

# (network, rows); every case runs B = 3 sequences
CASES = {
    "cfg1": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50, dropout=0.1), 50),
    "cfg1_prefix": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50, dropout=0.1), 17),
    "d128_h8": (dict(obs_dim=4, num_actions=4, inner_embed_size=128, num_heads=8, num_layers=2, history_len=50, dropout=0.1), 50),
    "gru": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=4, num_layers=2, history_len=20, gate="gru", dropout=0.1), 20),
    "identity": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=4, num_layers=2, history_len=70, identity=True,
                      dropout=0.1), 70),
    "discrete_p50": (dict(obs_dim=6, num_actions=5, inner_embed_size=64, num_heads=2, num_layers=1, history_len=12, discrete=True,
                          vocab_sizes=9, action_dim=8, dropout=0.5), 12),
    "bag5": (dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=20, action_dim=4, bag_size=5,
                  dropout=0.1), 20),
}
BATCH = 3


def oracle_grads_drop(cfg: O.NetCfg, params, obs, act, bag, w, drop, probe=None, dtype=torch.float32):
    """loss = (Q * w).sum() through oracle.forward under the keep masks of `drop`: q, {canonical key: grad}, d loss / d obss.
    dtype float64: the float32 parameters and inputs widened exactly, every operation in double."""
    keys = O.trainable_keys(cfg)
    params = {k: v.to(dtype) if v.dtype == torch.float32 else v for k, v in params.items()}
    leaves = {k: params[k].detach().clone().requires_grad_(True) for k in keys}
    p2 = {k: leaves.get(O.canonical_key(cfg, k), params[k]) for k in O.state_dict_keys(cfg)}
    o = torch.tensor(obs, dtype=dtype, requires_grad=True) if not cfg.discrete else torch.as_tensor(obs).long()
    kw = {}
    if bag is not None:
        kw = dict(bag_obss=torch.as_tensor(bag[0]).long() if cfg.discrete else torch.as_tensor(bag[0], dtype=dtype),
                  bag_actions=torch.as_tensor(bag[1]))
    q = O.forward(p2, cfg, o, torch.as_tensor(act), probe, drop, **kw)
    loss = (q * torch.as_tensor(w).to(dtype)).sum()
    wrt = [leaves[k] for k in keys] + ([o] if not cfg.discrete else [])
    g = torch.autograd.grad(loss, wrt)
    return q.detach().numpy(), dict(zip(keys, g)), (g[-1].numpy() if not cfg.discrete else None)


def flat_grad(m) -> np.ndarray:
    flat = torch.zeros(m.net.n_trainable, dtype=torch.float32)
    for p, off in m._grad_params(with_offsets=True):
        if p.grad is not None:
            flat[off:off + p.numel()] = p.grad.detach().reshape(-1).cpu()
    return flat.numpy()


def hip_grads_drop(m, obs, act, bag, w, keys, device="cpu", masks_out=None):
    """autograd_helpers.hip_grads with the forward given the keep-mask keys (seed, step)."""
    o = torch.tensor(obs, device=device, requires_grad=not m.discrete)
    kw = dict(_train_dropout=keys)
    if bag is not None:
        kw.update(bag_obss=torch.as_tensor(bag[0], device=device), bag_actions=torch.as_tensor(bag[1], device=device))
    m.zero_grad(set_to_none=True)
    q = m(o, torch.as_tensor(act, device=device), **kw)
    assert q.requires_grad and q.grad_fn is not None
    if masks_out is not None:
        masks_out.extend(forward_masks(q, m.net.num_layers, m.net.d_real or m.net.d_model))
    (q * torch.as_tensor(w, device=device)).sum().backward()
    return q.detach().cpu().numpy(), flat_grad(m), (None if o.grad is None else o.grad.cpu().numpy())


def check_dropout_parity(m, cfg, params, obs, act, bag, w, device="cpu", report=None):
    """Q, every parameter's gradient and obss.grad against the oracle under the masks of (SEED, STEP); the tolerances of
    autograd_helpers.check_against_oracle, every element compared (none is set aside for a ReLU kink).  The masks matter: without
    them the oracle's Q is somewhere else."""
    masks = []
    q, got, dobs = hip_grads_drop(m, obs, act, bag, w, (SEED, STEP), device, masks_out=masks)
    drop = O.DropSpec(cfg.dropout, SEED, STEP, 0)
    q_ref, grads, dobs_ref = oracle_grads_drop(cfg, params, obs, act, bag, w, drop)
    q_plain = oracle_grads_drop(cfg, params, obs, act, bag, w, None)[0]
    qmax = float(np.abs(q_ref).max())
    ref = flat_from_params(m.net, grads, O.trainable_keys(cfg))
    figures = {"q_err": float(np.abs(q - q_ref).max()), "q_max": qmax, "grad_err_over_max": float(np.abs(got - ref).max() / np.abs(ref).max())}
    if dobs_ref is not None:
        figures["dobs_err_over_max"] = float(np.abs(dobs - dobs_ref).max() / np.abs(dobs_ref).max())
    print("dropout parity", figures)
    if report is not None:
        report.update(figures)
    assert np.abs(q_plain - q_ref).max() > 1e-2 * max(1.0, qmax)
    assert figures["q_err"] <= 1e-4 * max(1.0, qmax), figures
    assert figures["grad_err_over_max"] <= 2e-4, figures
    pad = padding_mask(m.net)
    if pad.any():
        assert not got[pad].any()
    if dobs_ref is not None:
        assert dobs is not None and figures["dobs_err_over_max"] <= 2e-4, figures
    check_f64_under_masks(cfg, m.net, got, masks, qmax,
                          lambda probe, dtype: oracle_grads_drop(cfg, params, obs, act, bag, w, drop, probe, dtype)[1])
    return q, got, dobs


__all__ = ["CASES", "BATCH", "SEED", "STEP", "oracle_grads_drop", "flat_grad", "hip_grads_drop", "check_dropout_parity", "hip_grads"]
