"""Shared by the attention-capture tests (tests/test_emu_attention.py on the CPU emulation, tests/test_gpu_attention.py on the device):
the G13 fixture (the reference DTQN's own attention weights, tests/golden/make_golden_attention.py) and a DTQN module with its weights."""
import json
import os

import numpy as np
import torch

from oracle import dtqn_oracle as O

from autograd_helpers import make_module
from q_f64_helpers import check_q_f64, widen

G13 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "G13_attention.npz")


def g13():
    return np.load(G13)


def g13_names():
    with np.load(G13) as z:
        return json.loads(str(z["names"]))


def g13_case(z, name):
    """cfg, params, module inputs (obss as float32, like the module's other tests), Q, [alpha per layer], attn_weights (or None)."""
    cfg = O.NetCfg(**json.loads(str(z[f"{name}_cfg"])))
    meta = json.loads(str(z[f"{name}_meta"]))
    params = O.init_params(cfg, seed=meta["seed"], perturb=True)
    ref = float(z[f"{name}_checksum"])
    assert abs(O.param_checksum(params) - ref) <= 1e-9 * max(1.0, abs(ref)), "weight generator drifted"
    inputs = dict(obss=z[f"{name}_obs"].astype(np.float32), actions=z[f"{name}_act"])
    if cfg.bag_size > 0:
        inputs.update(bag_obss=z[f"{name}_bag_obs"].astype(np.float32), bag_actions=z[f"{name}_bag_act"])
    alphas = [z[f"{name}_alpha{l}"] for l in range(cfg.num_layers)]
    bag = z[f"{name}_attn_weights"] if cfg.bag_size > 0 else None
    return cfg, params, inputs, z[f"{name}_q"], alphas, bag


def tensors(inputs, device="cpu"):
    return {k: torch.as_tensor(v, device=device) for k, v in inputs.items()}


def capture_module(lib, cfg, params, device="cpu", autograd=False):
    m = make_module(lib, cfg, params, device=device, autograd=autograd)
    m.set_capture_attention(True)
    m.eval()
    return m


def captured(m):
    """[alpha of every layer] as numpy, and attn_weights (None without a bag)."""
    alphas = [layer.alpha.detach().cpu().numpy() for layer in m.transformer_layers]
    bag = m.attn_weights.detach().cpu().numpy() if m.bag_size > 0 else None
    return alphas, bag


def oracle_weights(cfg, params, inputs, wide=False):
    """O.attention_weights on module inputs (g13_case / make_inputs: obss as float32, tokens included): ([alpha per layer], bag weights or
    None) as numpy; wide: the float32 parameters, positions table and inputs widened exactly, every operation in float64."""
    integer = cfg.discrete and cfg.image is None
    as_obs = lambda a: torch.as_tensor(np.asarray(a)).long() if integer else torch.as_tensor(np.asarray(a, dtype=np.float32))
    w = widen if wide else (lambda t: t)
    kw = {}
    if cfg.bag_size > 0:
        kw = dict(bag_obss=w(as_obs(inputs["bag_obss"])), bag_actions=torch.as_tensor(np.asarray(inputs["bag_actions"])).long())
    with torch.no_grad():
        alphas, bag = O.attention_weights({k: w(v) for k, v in params.items()}, cfg, w(as_obs(inputs["obss"])),
                                          torch.as_tensor(np.asarray(inputs["actions"])).long(), **kw)
    return [a.numpy() for a in alphas], (None if bag is None else bag.numpy())


def check_weights(alphas, bag, ref_alphas, ref_bag, atol=1e-5, f64=None):
    """f64 = (cfg, params, inputs): the captured weights are also held, row by row at scale 1 (a row sums to 1), within margin * D32 of the
    oracle's float64 softmax, D32 from its fp32 evaluation (q_f64_helpers.check_q_f64); the fp32 oracle weights themselves have to be the
    reference weights handed in."""
    if f64 is not None:
        a32, b32 = oracle_weights(*f64)
        a64, b64 = oracle_weights(*f64, wide=True)
        for l, (a, r32, r64, ref) in enumerate(zip(alphas, a32, a64, ref_alphas)):
            assert np.abs(r32 - ref).max() <= atol, ("oracle.attention_weights is not the reference's alpha", l, np.abs(r32 - ref).max())
            check_q_f64(a, r64, r32, what=("alpha", l), scale=1.0)
        if ref_bag is not None:
            assert np.abs(b32 - ref_bag).max() <= atol, ("oracle.attention_weights is not the reference's bag weights", np.abs(b32 - ref_bag).max())
            check_q_f64(bag, b64, b32, what="bag weights", scale=1.0)
    assert len(alphas) == len(ref_alphas)
    for l, (a, r) in enumerate(zip(alphas, ref_alphas)):
        assert a.shape == r.shape, (l, a.shape, r.shape)
        err = np.abs(a - r).max()
        assert err <= atol, (l, err)
        n = a.shape[-1]
        assert not a[:, np.triu_indices(n, 1)[0], np.triu_indices(n, 1)[1]].any(), "nonzero weight above the diagonal"
        assert np.abs(a.sum(-1) - 1.0).max() <= 1e-5
    if ref_bag is not None:
        assert bag is not None and bag.shape == ref_bag.shape
        assert np.abs(bag - ref_bag).max() <= atol, np.abs(bag - ref_bag).max()
        assert np.abs(bag.sum(-1) - 1.0).max() <= 1e-5
