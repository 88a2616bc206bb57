#!/usr/bin/env python3
"""Generate tests/golden/G13_attention.npz by running THE REFERENCE ITSELF: the attention weights its DTQN leaves on the module after
a forward (TransformerLayer.alpha, transformer.py:46,64-70,88-94; DTQN.attn_weights with a bag, dtqn.py:211).

Runs only in the build container (needs the reference checkout, read-only), through make_golden.py's stubs and loaders.  Eval mode,
CPU.  Only DATA is written: per case the constructor arguments, the weight seed and checksum (oracle.dtqn_oracle.init_params, as in
every other fixture: both sides regenerate the weights from the seed), the inputs, Q, every layer's alpha [B, n, n] and, with a bag,
attn_weights [B, n, bag_size].

Usage:  python tests/golden/make_golden_attention.py            (writes next to this file)
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_golden as MG                                             # noqa: E402  (stubs + the reference's modules)
from oracle import dtqn_oracle as O                                  # noqa: E402

# (name, network, batch, rows)
CASES = [
    ("cfg1", O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50), 2, 50),
    ("prefix", O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50), 2, 17),
    ("gru_identity", O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=4, num_layers=2, history_len=20, gate="gru",
                              identity=True), 2, 20),
    ("pos_sin", O.NetCfg(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=30, pos="sin"), 2, 30),
    ("discrete_action", O.NetCfg(obs_dim=4, num_actions=5, inner_embed_size=64, num_heads=4, num_layers=1, history_len=16, discrete=True,
                                 vocab_sizes=9, action_dim=8), 2, 16),
    ("padded_48_6", O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=48, num_heads=6, num_layers=2, history_len=20), 2, 20),
    ("bag4", O.NetCfg(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=20, action_dim=4,
                      bag_size=4), 2, 20),
    ("d128_h2_L300", O.NetCfg(obs_dim=4, num_actions=3, inner_embed_size=128, num_heads=2, num_layers=1, history_len=300), 1, 300),
]


def gen_G13():
    out = {"stamp": json.dumps(MG.STAMP), "names": json.dumps([c[0] for c in CASES])}
    for i, (name, cfg, Bn, n) in enumerate(CASES):
        seed = 130 + i
        params = O.init_params(cfg, seed=seed, perturb=True)
        net = MG.make_ref_net(cfg, params)
        net.eval()
        rng = np.random.Generator(np.random.PCG64(seed + 1000))
        draw = lambda *shape: (rng.integers(0, cfg.vocab_sizes, size=shape).astype(np.int64) if cfg.discrete
                               else rng.uniform(-1, 1, size=shape).astype(np.float32))
        obs = draw(Bn, n, cfg.obs_dim)
        act = rng.integers(0, cfg.num_actions, size=(Bn, n, 1))
        args = [torch.as_tensor(obs), torch.as_tensor(act)]
        if cfg.bag_size > 0:
            bag_obs, bag_act = draw(Bn, cfg.bag_size, cfg.obs_dim), rng.integers(0, cfg.num_actions, size=(Bn, cfg.bag_size, 1))
            args += [torch.as_tensor(bag_obs), torch.as_tensor(bag_act)]
            out.update({f"{name}_bag_obs": bag_obs, f"{name}_bag_act": bag_act})
        with torch.no_grad():
            q = net(*args).numpy()
        out.update({f"{name}_cfg": json.dumps(cfg.to_json()), f"{name}_meta": json.dumps({"seed": seed, "B": Bn, "n": n}),
                    f"{name}_checksum": MG.checksum(params), f"{name}_obs": obs, f"{name}_act": act, f"{name}_q": q})
        for l, layer in enumerate(net.transformer_layers):
            out[f"{name}_alpha{l}"] = layer.alpha.detach().numpy().astype(np.float32)
        if cfg.bag_size > 0:
            out[f"{name}_attn_weights"] = net.attn_weights.detach().numpy().astype(np.float32)
            assert net.bag_attn_weights is None
        print(name, {k: v.shape for k, v in out.items() if k.startswith(name) and isinstance(v, np.ndarray) and v.ndim > 1})
    np.savez_compressed(os.path.join(HERE, "G13_attention.npz"), **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    gen_G13()
