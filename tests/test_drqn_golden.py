"""tests/drqn_oracle.py against what the reference's own DRQN and DrqnAgent computed (tests/golden/G13_drqn.npz, written by
tests/golden/make_golden_drqn.py): the packed forward, a step-mode chain, three agent updates and a seeded episode, to 1e-6."""
import os

import numpy as np
import pytest
import torch

import drqn_oracle as O

TOL = 1e-6
HISTORY, TUF, LR, GAMMA = 4, 2, 3e-4, 0.99


@pytest.fixture(scope="module")
def g13(golden_dir):
    path = os.path.join(golden_dir, "G13_drqn.npz")
    assert os.path.getsize(path) < 1 << 20
    data = np.load(path, allow_pickle=False)
    assert all(data[k].dtype.kind in "fiub" or data[k].dtype.kind == "U" for k in data.files)        # arrays and short strings only
    return data


def case_of(g13, name):
    pre = name + "/"
    return {k[len(pre):]: g13[k] for k in g13.files if k.startswith(pre)}


def close(a, b, tol=TOL):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and float(np.abs(a - b).max(initial=0.0)) <= tol * max(1.0, float(np.abs(b).max(initial=0.0)))


@pytest.mark.parametrize("name,discrete", [("cont", False), ("disc", True)])
def test_oracle_forward_matches_the_reference(g13, name, discrete):
    c = case_of(g13, name)
    params = {k[len("param/"):]: v for k, v in c.items() if k.startswith("param/")}
    assert list(params) == O.keys(discrete)
    assert c["lengths"].tolist() == [1, 4, 6] and c["obs"].shape[:2] == (3, 6)
    p = O.to_torch(params)
    obs = torch.as_tensor(c["obs"])
    q, (h, cc) = O.forward(p, obs, discrete, c["lengths"])
    assert close(q, c["q_packed"]) and close(h, c["h_packed"][0]) and close(cc, c["c_packed"][0])
    hs = cs = torch.zeros(3, 16)
    qs = []
    for t in range(3):
        qt, (hs, cs) = O.forward(p, obs[:, t:t + 1], discrete, None, hs, cs)
        qs.append(qt)
    assert close(torch.cat(qs, dim=1), c["q_step"]) and close(hs, c["h_step"][0]) and close(cs, c["c_step"][0])
    # the float64 evaluation agrees with the reference's float32 one to float32 rounding
    q64, _ = O.forward(O.to_torch(params, torch.float64), obs if discrete else obs.double(), discrete, c["lengths"])
    assert close(q64, c["q_packed"], 1e-5)


@pytest.mark.parametrize("name,discrete", [("cont", False), ("disc", True)])
def test_oracle_learner_matches_the_reference_agent(g13, name, discrete):
    c = case_of(g13, name)
    params = {k[len("param/"):]: v for k, v in c.items() if k.startswith("param/")}
    learner = O.Learner(params, discrete, gamma=GAMMA, history=HISTORY, lr=LR, tuf=TUF)
    for k in range(3):
        b = {key[len(f"batch{k}/"):]: v for key, v in c.items() if key.startswith(f"batch{k}/")}
        stats = learner.update(b["obss"], b["actions"], b["rewards"], b["next_obss"], b["dones"], b["lengths"])
        assert close([stats[n] for n in O.STAT_NAMES], c["stats"][k]), (k, stats, c["stats"][k])
        if k == 0:
            coef = min(1.0, 1.0 / (stats["grad_norm"] + 1e-6))                 # the fixture holds the gradients after clip_grad_norm_
            for key in params:
                assert close(learner.grads[key] * coef, c[f"grad1/{key}"]), key
                assert close(learner.policy[key], c[f"after1/{key}"]), key
    for key in params:
        assert close(learner.policy[key], c[f"after3/{key}"]), key
        assert close(learner.target[key], c[f"target3/{key}"]), key
    assert not all(np.array_equal(c[f"after3/{key}"], c[f"target3/{key}"]) for key in params)        # copied at update 2, not at 3


@pytest.mark.parametrize("name,discrete", [("cont", False), ("disc", True)])
def test_oracle_episode_matches_the_reference_agent(g13, name, discrete):
    """drqn.py:84-112: the network steps first, epsilon is drawn after; Context.reset draws the padding actions."""
    c = case_of(g13, name)
    params = {k[len("param/"):]: v for k, v in c.items() if k.startswith("param/")}
    p = O.to_torch(params)
    seed = {"cont": 1300, "disc": 1301}[name] + 100
    rng = np.random.Generator(np.random.PCG64(seed=seed))
    rng.integers(3, size=(6, 1))
    h = cc = torch.zeros(1, 16)
    actions = []
    ep = c["episode_obs"]
    for t in range(10):
        q, (h, cc) = O.forward(p, torch.as_tensor(ep[t]).reshape(1, 1, -1), discrete, None, h, cc)
        actions.append(int(rng.integers(3)) if rng.random() < 0.5 else int(torch.argmax(q)))
    assert actions == c["episode_actions"].tolist()
    assert rng.random() == float(c["episode_next_draw"])
