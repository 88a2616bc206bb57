#!/usr/bin/env python3
"""Generate tests/golden/G13_drqn.npz by running the reference's DRQN and DrqnAgent themselves.

Runs only where the reference checkout is available (make_golden.py's REF), never on the GPU machine.  The reference's modules are
imported unmodified behind make_golden.py's stub modules (`gym`, `wandb`, `pyglet`).  Only DATA is written: parameters, inputs,
lengths and what the reference computed from them, as arrays and short strings.

Tiny sizes: D 16, L 6, B 3, lengths 1, 4 and 6, A 3; a continuous case (O = 3) and a discrete one (O = 4, V = 5, e = 8).  Per case
    param/<key>                 parameters (drqn_oracle.random_params, loaded with load_state_dict)
    obs, lengths                inputs of the packed forward;  q_packed, h_packed, c_packed its outputs
    q_step, h_step, c_step      a three-step chain in step mode on the first three rows (state carried from zeros)
    batch<k>/...                three update batches (obss, actions, rewards, next_obss, next_actions, dones, lengths)
    stats                       [3][8] the eight running statistics' newest entries after each update (drqn_oracle.STAT_NAMES order)
    grad1/<key>                 the gradients left on the parameters by update 1 (after clip_grad_norm_)
    after1/<key>, after3/<key>  policy parameters after one and three updates;  target3/<key> the target network after three (tuf = 2)
    episode_obs, episode_actions, episode_next_draw     a seeded ten-step epsilon-greedy episode (epsilon 0.5) and the next draw of the
                                exploration stream after it

Usage:  python tests/golden/make_golden_drqn.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG                                            # noqa: E402  (installs the stubs, puts the reference on sys.path)
from dtqn.networks.drqn import DRQN as RefDRQN                      # noqa: E402
from dtqn.agents.drqn import DrqnAgent as RefDrqnAgent              # noqa: E402
import utils.random as ref_random                                   # noqa: E402

import drqn_oracle as O                                              # noqa: E402

D, L, B, A, E = 16, 6, 3, 3, 8
LENGTHS = np.array([1, 4, 6], dtype=np.int64)
HISTORY, TUF, LR, GAMMA = 4, 2, 3e-4, 0.99
CASES = {"cont": dict(obs_dim=3, discrete=False, vocab=0), "disc": dict(obs_dim=4, discrete=True, vocab=5)}


def draw_obs(rng, shape, case):
    if case["discrete"]:
        return rng.integers(0, case["vocab"], size=shape).astype(np.int64)
    return rng.uniform(-1, 1, size=shape).astype(np.float32)


def make_batch(rng, case):
    obs = draw_obs(rng, (B, L + 1, case["obs_dim"]), case)
    acts = rng.integers(0, A, size=(B, L + 1, 1)).astype(np.int64)
    lens = rng.permutation(LENGTHS).reshape(B, 1)
    return dict(obss=obs[:, :-1], actions=acts[:, :-1], rewards=rng.choice(np.array([0, 0, 1, -1], dtype=np.float32), size=(B, L, 1)),
                next_obss=obs[:, 1:], next_actions=acts[:, 1:], dones=rng.random((B, L, 1)) < 0.2, lengths=lens)


def make_case(name, case, seed):
    rng = np.random.default_rng(seed)
    out = {}
    params = O.random_params(rng, case["obs_dim"], A, E, D, case["discrete"], case["vocab"])

    def factory():
        net = RefDRQN(case["obs_dim"], A, E, 0, D, case["discrete"], obs_vocab_size=case["vocab"] if case["discrete"] else None)
        assert list(net.state_dict().keys()) == O.keys(case["discrete"]), list(net.state_dict().keys())
        net.load_state_dict({k: torch.tensor(v) for k, v in params.items()})
        return net

    for k, v in params.items():
        out[f"param/{k}"] = v
    net = factory()
    obs = draw_obs(rng, (B, L, case["obs_dim"]), case)
    out["obs"], out["lengths"] = obs, LENGTHS
    with torch.no_grad():
        q, (h, c) = net(torch.as_tensor(obs), None, episode_lengths=torch.as_tensor(LENGTHS))
        out["q_packed"], out["h_packed"], out["c_packed"] = q.numpy(), h.numpy(), c.numpy()
        hid = (torch.zeros(1, B, D), torch.zeros(1, B, D))
        qs = []
        for t in range(3):
            qt, hid = net(torch.as_tensor(obs[:, t:t + 1]), None, hidden_states=hid)
            qs.append(qt.numpy())
        out["q_step"], out["h_step"], out["c_step"] = np.concatenate(qs, axis=1), hid[0].numpy(), hid[1].numpy()

    mask = case["vocab"] - 1 if case["discrete"] else -5
    agent = RefDrqnAgent(factory, 10 * 12, torch.device("cpu"), case["obs_dim"], 12, mask, A, case["discrete"], learning_rate=LR,
                         batch_size=B, context_len=L, gamma=GAMMA, target_update_frequency=TUF, embed_size=D, history=HISTORY)
    # a seeded ten-step epsilon-greedy episode on the fresh policy
    ref_random.RNG.rng = np.random.Generator(np.random.PCG64(seed=seed + 100))
    ep_obs = draw_obs(rng, (11, case["obs_dim"]), case)
    agent.eval_on()
    agent.context_reset(ep_obs[0])
    actions = []
    for t in range(10):
        a = int(agent.get_action(epsilon=0.5))
        actions.append(a)
        agent.observe(ep_obs[t + 1], a, 0.0, False)
    agent.eval_off()
    out["episode_obs"], out["episode_actions"] = ep_obs, np.array(actions, dtype=np.int64)
    out["episode_next_draw"] = np.array(ref_random.RNG.rng.random())
    # three updates on three handed-in batches
    batches = [make_batch(rng, case) for _ in range(3)]
    agent.replay_buffer.can_sample = lambda n: True
    stats = []
    for k, b in enumerate(batches):
        for key, v in b.items():
            out[f"batch{k}/{key}"] = v
        agent.replay_buffer.sample = lambda n, b=b: (b["obss"], b["actions"], b["rewards"], b["next_obss"], b["next_actions"], b["dones"], b["lengths"])
        agent.train()
        stats.append([agent.td_errors.q[-1], agent.grad_norms.q[-1], agent.qvalue_max.q[-1], agent.qvalue_mean.q[-1], agent.qvalue_min.q[-1],
                      agent.target_max.q[-1], agent.target_mean.q[-1], agent.target_min.q[-1]])
        if k == 0:
            for key, p in agent.policy_network.named_parameters():
                out[f"grad1/{key}"] = p.grad.detach().numpy().copy()
            for key, v in agent.policy_network.state_dict().items():
                out[f"after1/{key}"] = v.numpy().copy()
    out["stats"] = np.array(stats, dtype=np.float64)
    for key, v in agent.policy_network.state_dict().items():
        out[f"after3/{key}"] = v.numpy().copy()
    for key, v in agent.target_network.state_dict().items():
        out[f"target3/{key}"] = v.numpy().copy()
    assert agent.num_train_steps == 3
    return {f"{name}/{k}": v for k, v in out.items()}


def main():
    data = {"stamp": np.array(f"torch {torch.__version__} numpy {np.__version__} | D {D} L {L} B {B} A {A} history {HISTORY} tuf {TUF} lr {LR} gamma {GAMMA}")}
    for i, (name, case) in enumerate(CASES.items()):
        data.update(make_case(name, case, 1300 + i))
    path = os.path.join(HERE, "G13_drqn.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes,", len(data), "arrays")


if __name__ == "__main__":
    main()
