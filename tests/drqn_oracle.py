"""CPU oracle of the DRQN baseline (dtqn/networks/drqn.py, dtqn/agents/drqn.py): the network with explicit gate arithmetic, the
packed and the step forward, and one agent update including clip and Adam, in plain torch.  Callable in float32 and float64.

Parameters travel as a dict keyed like the reference's state_dict:
    obs_embed.observation_embedding.{weight,bias}                      (continuous observations)
    obs_embed.observation_embedding.{0.weight,2.weight,2.bias}         (discrete observations)
    lstm.{weight_ih_l0,weight_hh_l0,bias_ih_l0,bias_hh_l0}, ffn.{0,2}.{weight,bias}
"""
from typing import Dict, Optional

import numpy as np
import torch

KEYS_CONT = ["obs_embed.observation_embedding.weight", "obs_embed.observation_embedding.bias"]
KEYS_DISC = ["obs_embed.observation_embedding.0.weight", "obs_embed.observation_embedding.2.weight", "obs_embed.observation_embedding.2.bias"]
KEYS_TAIL = ["ffn.0.weight", "ffn.0.bias", "ffn.2.weight", "ffn.2.bias",
             "lstm.weight_ih_l0", "lstm.weight_hh_l0", "lstm.bias_ih_l0", "lstm.bias_hh_l0"]


def keys(discrete: bool):
    return (KEYS_DISC if discrete else KEYS_CONT) + KEYS_TAIL


def shapes(obs_dim, num_actions, embed_per_obs, d, discrete, vocab):
    out = {}
    if discrete:
        out[KEYS_DISC[0]] = (vocab, embed_per_obs)
        out[KEYS_DISC[1]] = (d, obs_dim * embed_per_obs)
        out[KEYS_DISC[2]] = (d,)
    else:
        out[KEYS_CONT[0]] = (d, obs_dim)
        out[KEYS_CONT[1]] = (d,)
    out.update({"ffn.0.weight": (d, d), "ffn.0.bias": (d,), "ffn.2.weight": (num_actions, d), "ffn.2.bias": (num_actions,),
                "lstm.weight_ih_l0": (4 * d, d), "lstm.weight_hh_l0": (4 * d, d), "lstm.bias_ih_l0": (4 * d,), "lstm.bias_hh_l0": (4 * d,)})
    return out


def random_params(rng: np.random.Generator, obs_dim, num_actions, embed_per_obs, d, discrete, vocab=0, scale=1.0) -> Dict[str, np.ndarray]:
    """Test parameters: weights large enough that every gate leaves its linear range (nothing to do with the module's initialisation)."""
    out = {}
    for k, shp in shapes(obs_dim, num_actions, embed_per_obs, d, discrete, vocab).items():
        fan = shp[-1] if len(shp) > 1 else d
        s = scale / np.sqrt(fan) if len(shp) > 1 else 0.1 * scale
        if k.endswith("0.weight") and discrete and k.startswith("obs_embed"):
            s = scale
        out[k] = (rng.standard_normal(shp) * s).astype(np.float32)
    return out


def to_torch(params: Dict[str, np.ndarray], dtype=torch.float32, grad=False) -> Dict[str, torch.Tensor]:
    return {k: torch.tensor(np.asarray(v), dtype=dtype).requires_grad_(grad) for k, v in params.items()}


def embed(p, obs: torch.Tensor, discrete: bool) -> torch.Tensor:
    """obs [B, n, O] -> [B, n, D]"""
    if discrete:
        e = p[KEYS_DISC[0]][obs.long()]                           # [B, n, O, e]
        e = e.reshape(*e.shape[:-2], -1)
        return e @ p[KEYS_DISC[1]].T + p[KEYS_DISC[2]]
    return obs.to(p[KEYS_CONT[0]].dtype) @ p[KEYS_CONT[0]].T + p[KEYS_CONT[1]]


def lstm(p, x: torch.Tensor, lengths: Optional[torch.Tensor], h0=None, c0=None):
    """torch.nn.LSTM (one layer, batch_first) on x [B, n, D] with explicit gates i | f | g | o.  lengths [B] (packed-sequence mode): output
    rows at or beyond lengths[b] are 0 and the state stops at the last live row.  Returns out [B, n, D], h_n [B, D], c_n [B, D]."""
    B, n, D = x.shape
    w_ih, w_hh, b_ih, b_hh = p["lstm.weight_ih_l0"], p["lstm.weight_hh_l0"], p["lstm.bias_ih_l0"], p["lstm.bias_hh_l0"]
    h = torch.zeros(B, D, dtype=x.dtype) if h0 is None else h0.to(x.dtype)
    c = torch.zeros(B, D, dtype=x.dtype) if c0 is None else c0.to(x.dtype)
    outs = []
    for t in range(n):
        g = x[:, t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh
        i, f, gg, o = torch.sigmoid(g[:, :D]), torch.sigmoid(g[:, D:2 * D]), torch.tanh(g[:, 2 * D:3 * D]), torch.sigmoid(g[:, 3 * D:])
        c_new = f * c + i * gg
        h_new = o * torch.tanh(c_new)
        if lengths is None:
            h, c = h_new, c_new
            outs.append(h_new)
        else:
            live = (t < lengths).to(x.dtype).unsqueeze(1)
            h = live * h_new + (1 - live) * h
            c = live * c_new + (1 - live) * c
            outs.append(live * h_new)
    return torch.stack(outs, dim=1), h, c


def head(p, y: torch.Tensor) -> torch.Tensor:
    return torch.relu(y @ p["ffn.0.weight"].T + p["ffn.0.bias"]) @ p["ffn.2.weight"].T + p["ffn.2.bias"]


def forward(p, obs, discrete: bool, lengths=None, h0=None, c0=None):
    """DRQN.forward: Q [B, n, A], (h_n [B, D], c_n [B, D]).  lengths: packed-sequence mode; h0 / c0: step mode."""
    if lengths is not None:
        lengths = torch.as_tensor(np.asarray(lengths)).reshape(-1).long()
    out, h, c = lstm(p, embed(p, obs, discrete), lengths, h0, c0)
    return head(p, out), (h, c)


def head_of_zero(p) -> torch.Tensor:
    d = p["ffn.0.bias"].shape[0]
    return head(p, torch.zeros(d, dtype=p["ffn.0.bias"].dtype))


def gradients(params: Dict[str, np.ndarray], obs, lengths, dq, discrete: bool, dtype=torch.float32):
    """(Q, {key: d sum(Q * dq) / d param}) of the packed forward."""
    p = to_torch(params, dtype, grad=True)
    o = torch.as_tensor(np.asarray(obs))
    q, _ = forward(p, o if discrete else o.to(dtype), discrete, lengths)
    (q * torch.as_tensor(np.asarray(dq)).to(dtype)).sum().backward()
    return q.detach(), {k: v.grad.detach() for k, v in p.items()}


STAT_NAMES = ["td_error", "grad_norm", "qvalue_max", "qvalue_mean", "qvalue_min", "target_max", "target_mean", "target_min"]


class Learner:
    """DrqnAgent.train (drqn.py:114-210) on a batch handed in: three packed forwards, double-DQN target, MSE over the last `history`
    columns (padding rows included), clip_grad_norm_, Adam (torch.optim.Adam's defaults), hard target copy every `tuf` updates."""

    def __init__(self, params: Dict[str, np.ndarray], discrete: bool, gamma=0.99, history=50, lr=3e-4, clip=1.0, tuf=10_000, dtype=torch.float32):
        self.dtype, self.discrete = dtype, discrete
        self.policy = to_torch(params, dtype)
        self.target = {k: v.clone() for k, v in self.policy.items()}
        self.gamma, self.history, self.lr, self.clip, self.tuf = gamma, history, lr, clip, tuf
        self.m = {k: torch.zeros_like(v) for k, v in self.policy.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.policy.items()}
        self.steps = 0
        self.grads = None

    def update(self, obss, actions, rewards, next_obss, dones, lengths) -> Dict[str, float]:
        dt = self.dtype
        as_obs = (lambda a: torch.as_tensor(np.asarray(a)).long()) if self.discrete else (lambda a: torch.as_tensor(np.asarray(a)).to(dt))
        obss, next_obss = as_obs(obss), as_obs(next_obss)
        actions = torch.as_tensor(np.asarray(actions)).long()
        rewards = torch.as_tensor(np.asarray(rewards)).to(dt).squeeze(-1)
        dones = torch.as_tensor(np.asarray(dones)).to(dt).squeeze(-1)
        p = {k: v.clone().requires_grad_(True) for k, v in self.policy.items()}
        q_all, _ = forward(p, obss, self.discrete, lengths)
        q = q_all.gather(2, actions).squeeze(-1)
        with torch.no_grad():
            argmax = torch.argmax(forward(self.policy, next_obss, self.discrete, lengths)[0], dim=2).unsqueeze(-1)
            nq = forward(self.target, next_obss, self.discrete, lengths)[0].gather(2, argmax).squeeze(-1)
            targets = rewards + (1 - dones) * (nq * self.gamma)
        q, targets = q[:, -self.history:], targets[:, -self.history:]
        loss = ((q - targets) ** 2).mean()
        loss.backward()
        grads = {k: v.grad.detach() for k, v in p.items()}
        self.grads = {k: g.clone() for k, g in grads.items()}
        norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values())).to(dt)
        if not bool(torch.isfinite(norm)):
            raise RuntimeError("non-finite gradient norm")
        coef = torch.clamp(self.clip / (norm + 1e-6), max=1.0)
        self.steps += 1
        b1, b2, eps = 0.9, 0.999, 1e-8
        bc1, bc2 = 1 - b1 ** self.steps, 1 - b2 ** self.steps
        for k in self.policy:
            g = grads[k] * coef
            self.m[k] = b1 * self.m[k] + (1 - b1) * g
            self.v[k] = b2 * self.v[k] + (1 - b2) * g * g
            denom = self.v[k].sqrt() / np.sqrt(bc2) + eps
            self.policy[k] = self.policy[k] - (self.lr / bc1) * self.m[k] / denom
        if self.steps % self.tuf == 0:
            self.target = {k: v.clone() for k, v in self.policy.items()}
        qd, td = q.detach(), targets
        return {"td_error": float(loss.detach()), "grad_norm": float(norm), "qvalue_max": float(qd.max()), "qvalue_mean": float(qd.mean()),
                "qvalue_min": float(qd.min()), "target_max": float(td.max()), "target_mean": float(td.mean()), "target_min": float(td.min())}
