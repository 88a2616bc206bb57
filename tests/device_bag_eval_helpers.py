"""Shared by test_emu_device_bag_eval.py (HIP emulation on the CPU) and test_gpu_device_bag_eval.py (MI355X): the device-resident greedy
evaluation of a bag network (dtqn_deval_begin_bag / dtqn_deval_step_bag, dtqn_amd.agents.device_bag_eval.DeviceBagEvaluator) against a
host Context + Bag per environment and DtqnAgent._bag_forward, and the candidate forward on a shared trunk
(dtqn_forward_bag_candidates) against dtqn_forward_bag on the tiled inputs.

Shapes, those of device_bag_helpers.py: d_model 64 / 8 heads / 1 layer, context L = 6, bag K = 2, N = 3 environments, a step cap of 12
-- a window slides from step 6 on, steps 6-7 append, steps 8-11 choose among K + 1 = 3 candidates, step 12 truncates -- and 7 episodes,
so that the environments go idle at different times (environment 0 plays three, the others two).  The Q head is x 100, the networks are
the `scaled` ones (the bag moves Q).

The host never draws or decides: after every vector step the device state is read back and each environment's host Context + Bag replay
what the device did.  Step parity (check_step_parity) with the network seeds of PARITY_SEED, counted on the emulation by the host
reference alone (`seen` of EvalReplay):
  car    (seed 11) 84 environment steps: 42 evictions = 14 appends + 28 choices (26 decisive, 8 kept the bag), 7 bags cleared (all 7
         episodes truncated), 35 steps without an eviction, 24 steps of idle environments
  mem    (seed 11) 66 environment steps: 24 evictions = 12 appends + 12 choices (8 decisive, 5 kept), 7 cleared (3 truncated, 4 ended
         by the environment), 35 without an eviction, 27 idle
  tiger  (seed 13: a network whose greedy action is mostly "listen") 68 environment steps: 26 evictions = 14 appends + 12 choices (12
         decisive), 7 cleared (3 truncated, 4 doors opened), 35 without an eviction, 28 idle"""
import ctypes
import glob

import numpy as np
import torch

from oracle import dtqn_oracle as O

import device_bag_helpers as BH
from autograd_helpers import make_module
from device_bag_helpers import CAP, ENV_ID, K, L, N, PAIRS, Replay, f32_bits, make_agent, q_tol
from device_eval_helpers import _agent_snapshot, _assert_same, run_formulas

EPISODES = 7
PARITY_SEED = {"car": 11, "mem": 11, "tiger": 13}
LDS_BYTES = 160 * 1024


def make_evaluator(agent, kind="car", n=N, seed=5, cap=CAP, max_episodes=8):
    from dtqn_amd.agents.device_bag_eval import DeviceBagEvaluator
    return DeviceBagEvaluator(agent, ENV_ID[kind], n, seed, max_episode_steps=cap, num_pairs=PAIRS if kind == "mem" else None,
                              max_episodes=max_episodes)


# ------------------------------------------------------------------------------------------ 1. candidate forward on caller arrays
def bag_attn_lds(ctx, bag, hd):
    """dtqn_limits.h dtqn_bag_attn_lds at the full context: tl_bag_mfma(net) is this request exceeding a workgroup's 160 KB."""
    return (2 * bag * hd + ctx * bag) * 4


def smallest_mfma_bag(ctx, hd):
    bag = next(b for b in range(1, ctx + 1) if bag_attn_lds(ctx, b, hd) > LDS_BYTES)
    assert bag_attn_lds(ctx, bag - 1, hd) <= LDS_BYTES < bag_attn_lds(ctx, bag, hd)
    return bag


_BASE = dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=1, history_len=L, bag_size=K)
CANDIDATE_CASES = {
    "base": (dict(_BASE), N, K + 1),
    "gru": (dict(_BASE, gate="gru"), N, K + 1),
    "identity": (dict(_BASE, identity=True), N, K + 1),
    "a-embed-4": (dict(_BASE, action_dim=4), N, K + 1),
    "d128-2-layers": (dict(_BASE, inner_embed_size=128, num_layers=2), N, K + 1),
    # the smallest bag of a 200-row context at head width 8 whose resident request does not fit: the tl_bag_attn_mfma_* path
    "mfma-bag": (dict(_BASE, history_len=200, bag_size=smallest_mfma_bag(200, 8)), 2, 2),
}


def check_candidate_forward(lib, device, case, capfd, monkeypatch):
    """dtqn_forward_bag_candidates on n_ctx contexts x n_cand bags against dtqn_forward_bag on the n_ctx n_cand tiled sequences."""
    kw, n_ctx, n_cand = CANDIDATE_CASES[case]
    cfg = O.NetCfg(**kw)
    m = make_module(lib if device == "cpu" else None, cfg, O.init_params(cfg, seed=4, perturb=True), device=device, autograd=False)
    m.eval()
    net, Lc, Kc, A = m.net, cfg.history_len, cfg.bag_size, cfg.num_actions
    mfma = bag_attn_lds(Lc, Kc, cfg.inner_embed_size // cfg.num_heads) > LDS_BYTES
    assert mfma == (case == "mfma-bag")
    rng = np.random.default_rng(6)
    obs = rng.uniform(-1, 1, size=(n_ctx, Lc, cfg.obs_dim)).astype(np.float32)
    act = rng.integers(0, A, size=(n_ctx, Lc)).astype(np.uint8)
    cand_obs = rng.uniform(-1, 1, size=(n_ctx, n_cand, Kc, cfg.obs_dim)).astype(np.float32)
    cand_act = rng.integers(0, A, size=(n_ctx, n_cand, Kc)).astype(np.uint8)
    dev = lambda a: torch.as_tensor(a, device=device)
    S = n_ctx * n_cand
    with torch.no_grad():
        ref = m(dev(np.repeat(obs, n_cand, axis=0)), dev(np.repeat(act, n_cand, axis=0)[..., None].astype(np.int64)),
                bag_obss=dev(cand_obs.reshape(S, Kc, -1)), bag_actions=dev(cand_act.reshape(S, Kc, 1).astype(np.int64))).cpu().numpy()
    need = m._lib.dtqn_bag_candidates_workspace_floats(ctypes.byref(net), n_ctx, n_cand)
    assert need == (n_ctx + S) * (m._lib.dtqn_forward_workspace_floats(ctypes.byref(net), 1)) > 0
    ws = torch.zeros(need, dtype=torch.float32, device=device)
    q = torch.full((n_ctx, n_cand, Lc, A), float("nan"), dtype=torch.float32, device=device)
    t = [dev(obs), dev(act), dev(cand_obs), dev(cand_act)]
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(device)).cuda_stream) if device != "cpu" else None
    monkeypatch.setenv("DTQN_TL_TRACE", "1")
    capfd.readouterr()
    rc = m._lib.dtqn_forward_bag_candidates(ctypes.byref(net), p(m.flat), p(t[0]), p(t[1]) if cfg.action_dim > 0 else None, p(t[2]),
                                            p(t[3]) if cfg.action_dim > 0 else None, n_ctx, n_cand, Lc, p(q), p(ws), stream)
    got = q.cpu().numpy().reshape(S, Lc, A)
    err = capfd.readouterr().err
    monkeypatch.delenv("DTQN_TL_TRACE")
    assert rc == 0
    rpb = net.lp // 64
    # the trunk ran on n_ctx sequences, the tail on n_ctx n_cand: the broadcast, and the bag attention of the family the bound names
    assert f"tl_launch tl_bcast_kernel grid={S * rpb},1,1" in err, err
    assert ("tl_bag_attn_mfma_kernel<" in err) == mfma and ("tl_launch tl_bag_attn_kernel" in err) == (not mfma), err
    assert ("tl_launch tl_copy_kernel" in err) == bool(cfg.identity), err
    attn = [ln for ln in err.splitlines() if "tl_launch" in ln and "attn" in ln and "bag" not in ln]
    assert len(attn) == cfg.num_layers and all(f"grid={n_ctx}," in ln for ln in attn), attn
    tol, diff = q_tol(ref), float(np.abs(got - ref).max())
    print(f"candidate forward [{case}] largest difference {diff:.3e} (tolerance {tol:.3e}), bit-equal: {got.tobytes() == ref.tobytes()}")
    assert np.isfinite(got).all() and diff <= tol, (case, diff, tol)
    # unsupported shapes: no workspace, and the entry refuses
    assert m._lib.dtqn_bag_candidates_workspace_floats(ctypes.byref(net), 0, n_cand) == 0
    assert m._lib.dtqn_bag_candidates_workspace_floats(ctypes.byref(net), n_ctx, 0) == 0
    assert m._lib.dtqn_forward_bag_candidates(ctypes.byref(net), p(m.flat), p(t[0]), p(t[1]), p(t[2]), p(t[3]), n_ctx, n_cand, Lc - 1, p(q), p(ws),
                                              stream) != 0


# ------------------------------------------------------------------------------------------ 2. step parity
class EvalReplay(Replay):
    """device_bag_helpers.Replay on the evaluator's state: N host Context + Bag pairs that replay the device one vector step at a time.
    On top of the bags' bookkeeping: the action is the first arg-max of Q WITH the bag, a finished episode clears the bag whatever the
    next episode is, an idle environment's bag, position and candidates are left alone."""

    def __init__(self, agent, ev, episodes=EPISODES, key=3):
        ev.begin(episodes, key=key)
        super().__init__(agent, ev)
        self.playing = [int(e) for e in self.st.episode]
        self.seen.update(idle_env=0, truncated=0, greedy_checked=0)
        self.choices = {}                                 # (episode, step within it) -> (candidate kept, the bag after)

    def step(self):
        agent, ev, before = self.agent, self.actor, self.st
        Kb = agent.bag.size
        live = [e >= 0 for e in self.playing]
        q_ref = [self.host_q_last(i) if live[i] else None for i in range(self.n)]
        q_bare = [self.host_q_last(i, cleared=True) if live[i] else None for i in range(self.n)]
        ev.step()
        st = self.st = ev.get_state()
        q_dev = ev.q_rows()
        self.seen["steps"] += 1
        for i in range(self.n):
            where = (self.seen["steps"], i)
            assert st.bag.choosing[i] == 0, where
            if not live[i]:                                        # idle: no step, and nothing of its bag state moves
                assert st.last[i, 0] == -1 and st.last[i, 6] == -1 and st.episode[i] == -1 and st.bag.choice[i] == -1, where
                assert st.bag.obs[i].tobytes() == before.bag.obs[i].tobytes() and st.bag.actions[i].tobytes() == before.bag.actions[i].tobytes(), where
                assert st.bag.pos[i] == before.bag.pos[i] and st.bag.cand_obs[i].tobytes() == before.bag.cand_obs[i].tobytes(), where
                assert st.bag.scores[i].tobytes() == before.bag.scores[i].tobytes(), where
                self.seen["idle_env"] += 1
                continue
            # the greedy action is taken from Q with the bag
            tol = q_tol(q_ref[i])
            assert np.isfinite(q_dev[i]).all() and np.abs(q_dev[i] - q_ref[i]).max() <= tol, (where, q_dev[i], q_ref[i], tol)
            action, done, stored = int(st.last[i, 0]), bool(st.last[i, 2]), bool(st.last[i, 3])
            assert action == int(np.argmax(q_dev[i])) and st.last[i, 6] == self.playing[i], (where, action, q_dev[i])
            top = np.sort(q_ref[i])[::-1]
            if top[0] - top[1] > 2 * tol:
                assert action == int(np.argmax(q_ref[i])), (where, action, q_ref[i])
                self.seen["greedy_checked"] += 1
            if self.bags[i].pos > 0:
                self.seen["q_checked"] += 1
                self.seen["q_moved"] += bool(np.abs(q_dev[i] - q_bare[i]).max() > tol)
            t = int(before.elapsed[i]) + 1
            obs, reward = np.array(st.obs_new[i], copy=True), float(st.reward[i])
            if done:                                               # the bag ends up cleared, whether the environment plays on or goes idle
                assert (st.bag.obs[i] == np.float32(agent.obs_mask)).all() and not st.bag.actions[i].any(), where
                assert st.bag.pos[i] == 0 and st.bag.choice[i] == -1, where
                self.seen["cleared"] += 1
                self.seen["truncated"] += bool(st.last[i, 4])
                self.playing[i] = int(st.episode[i])
                if self.playing[i] >= 0:
                    self._begin(i, st)
                else:
                    self.bags[i].reset()
                continue
            ev_obs, ev_act = self.ctx[i].add_transition(obs, action, reward, stored)
            if ev_obs is None:                                     # nothing evicted, no reset: the bag bytes stay
                assert st.bag.choice[i] == -1 and st.bag.obs[i].tobytes() == before.bag.obs[i].tobytes(), where
                assert st.bag.actions[i].tobytes() == before.bag.actions[i].tobytes() and st.bag.pos[i] == before.bag.pos[i], where
                self.seen["idle"] += 1
                continue
            self.seen["evicted"] += 1
            ev_act = int(np.asarray(ev_act).reshape(-1)[0])
            assert f32_bits(before.block.obs[i, 0]).tobytes() == f32_bits(ev_obs).tobytes() and ev_act == action, where
            bag = self.bags[i]
            if bag.add(ev_obs, ev_act):
                assert st.bag.choice[i] == -1, where
                self._assert_bag(i, st, where)
                self.seen["appends"] += 1
                continue
            C = Kb + 1
            cand_obss, cand_actions = np.tile(bag.obss, (C, 1, 1)), np.tile(bag.actions, (C, 1, 1))
            for c in range(Kb):
                cand_obss[c, c], cand_actions[c, c] = ev_obs, ev_act
            assert f32_bits(st.bag.cand_obs[i]).tobytes() == f32_bits(cand_obss).tobytes(), where
            assert st.bag.cand_actions[i].tobytes() == cand_actions.astype(np.uint8).reshape(-1).tobytes(), where
            ctx = self.ctx[i]
            with torch.no_grad():
                q = agent._bag_forward(np.tile(ctx.obs, (C, 1, 1)), np.tile(ctx.action, (C, 1, 1)), cand_obss, cand_actions)
                host = BH._to_np(torch.mean(torch.max(q, 2)[0], 1))
            tol = q_tol(BH._to_np(q))
            dev = st.bag.scores[i]
            print("choice", where, "device scores", dev, "host scores", host, "tolerance", tol)
            assert np.isfinite(dev).all() and np.abs(dev - host).max() <= tol, (where, dev, host, tol)
            keep = int(st.bag.choice[i])
            assert keep == int(np.argmax(dev)), (where, keep, dev)            # the first arg-max of the device's own scores
            assert host[keep] >= host.max() - 2 * tol, (where, keep, host, tol)
            best = int(np.argmax(host))
            same = lambda c: cand_obss[c].tobytes() == cand_obss[best].tobytes() and cand_actions[c].tobytes() == cand_actions[best].tobytes()
            decisive = all(same(c) for c in range(C) if host[c] >= host.max() - 2 * tol)
            bag.obss, bag.actions = cand_obss[keep], cand_actions[keep]     # the host follows the device's choice
            self._assert_bag(i, st, where)
            if decisive:
                assert f32_bits(st.bag.obs[i]).tobytes() == f32_bits(cand_obss[best]).tobytes(), where
                assert st.bag.actions[i].tobytes() == cand_actions[best].astype(np.uint8).reshape(-1).tobytes(), where
            self.seen["choices"] += 1
            self.seen["kept"] += keep == Kb
            self.seen["decisive"] += decisive
            self.choices[(self.playing[i], t)] = (keep, st.bag.obs[i].tobytes(), st.bag.actions[i].tobytes())
        c = st.bag.counters
        assert (int(c[0]), int(c[1]), int(c[2]), int(c[3])) == tuple(self.seen[k] for k in ("appends", "choices", "kept", "cleared")), (c, self.seen)
        return st


def check_step_parity(lib, device, kind):
    agent = make_agent(lib, device, kind, scaled=True, seed=PARITY_SEED[kind])
    ev = make_evaluator(agent, kind)
    rep = EvalReplay(agent, ev)
    k = 0
    while any(e >= 0 for e in rep.playing):
        assert k < 3 * CAP, "more vector steps than ceil(7 / 3) episodes of `cap` steps"
        # the host's switch: false before vector step L + K - 1 since the begin
        assert ev._may_choose() == (k >= L + K - 1), (k, ev._to_choice)
        rep.step()
        k += 1
    seen = rep.seen
    print(kind, seen)
    got = ev.poll()
    assert got["finished"] == EPISODES and got["live"] == 0 and got["env_steps"] == seen["evicted"] + seen["idle"] + seen["cleared"], (got, seen)
    # every phase: windows that did not slide, evictions appended and chosen, bags cleared by an episode end, idle environments
    for phase in ("idle", "evicted", "appends", "choices", "cleared", "idle_env", "q_checked", "greedy_checked"):
        assert seen[phase] >= 1, (phase, seen)
    assert seen["evicted"] == seen["appends"] + seen["choices"] and seen["cleared"] == EPISODES, seen
    assert 2 * seen["decisive"] >= seen["choices"], f"{seen['decisive']} of {seen['choices']} choices were decisive"
    assert seen["q_moved"] >= 1, seen
    assert ev.bag_counters() == {k_: int(seen[k_]) for k_ in ("appends", "choices", "kept", "cleared")}
    assert ev.choice_steps == max(0, ev.vector_steps - (L + K - 1)) and ev.vector_steps == k
    # steps past the end: nobody wakes up, no bag moves
    raw = ev.get_state().bag.raw.tobytes()
    ev.step()
    assert ev.get_state().bag.raw.tobytes() == raw


def check_may_choose(lib, device):
    """Never under a cap below L + K; after set_state recomputed from `elapsed` and `bag.pos`."""
    agent = make_agent(lib, device, "car", scaled=True)
    short = make_evaluator(agent, "car", cap=L + K - 1)
    short.begin(2, key=1)
    for _ in range(2 * (L + K)):
        assert not short._may_choose()
        short.step()
    assert short.choice_steps == 0 and short.bag_counters()["choices"] == 0
    ev = make_evaluator(agent, "car")
    ev.begin(3, key=1)
    ev.step()
    st = ev.get_state()
    assert ev._to_choice == L + K - 1
    st.elapsed[1], st.bag.pos[1] = L - 1, K                      # environment 1: slides at the next step onto a full bag
    st.block.lens[1] = L
    ev.set_state(st)
    assert ev._to_choice == 1 and ev._may_choose()
    ev.step()
    st = ev.get_state()
    assert st.bag.choice[1] in range(K + 1) and st.bag.choice[0] == -1 and st.bag.counters[1] == 1, (st.bag.choice, st.bag.counters)


# ------------------------------------------------------------------------------------------ 3. episodes do not depend on N
def _play(ev, episodes, key):
    """An evaluation stepped by hand -> per-episode results, every action and every bag choice by (episode, step within it)."""
    ev.begin(episodes, key=key)
    st = ev.get_state()
    actions, choices = {}, {}
    bound = -(-episodes // ev.n) * ev.cap
    for _ in range(bound):
        before = st
        ev.step()
        st = ev.get_state()
        for i in range(ev.n):
            e = int(st.last[i, 6])
            if e < 0:
                continue
            t = int(before.elapsed[i]) + 1
            actions[(e, t)] = int(st.last[i, 0])
            if st.bag.choice[i] >= 0:
                choices[(e, t)] = (int(st.bag.choice[i]), st.bag.obs[i].tobytes(), st.bag.actions[i].tobytes())
        if st.counters[0] == episodes:
            break
    assert st.counters[0] == episodes and st.counters[5] == 0, st.counters
    res = st.results[:episodes]
    return [(float(r["ret"]), int(r["length"]), int(r["success"])) for r in res], actions, choices


def check_independent_of_n(lib, device, kind="car"):
    agent = make_agent(lib, device, kind, scaled=True)
    ref = None
    for n in (1, 2, 3):
        ev = make_evaluator(agent, kind, n=n)
        got = _play(ev, EPISODES, key=9)
        assert len(got[2]) >= EPISODES, (n, len(got[2]))          # bag choices were made
        if ref is None:
            ref = got
        assert got[0] == ref[0] and got[1] == ref[1] and got[2] == ref[2], n
        triple = ev.evaluate(EPISODES, key=9)                     # the same episodes through evaluate(): the quota is exact
        res = ev.results()
        assert len(res.returns) == EPISODES and ev.poll()["finished"] == EPISODES and ev.poll()["live"] == 0
        assert [(float(r), int(l_), int(s)) for r, l_, s in zip(res.returns, res.lengths, res.successes)] == ref[0], n
        assert triple == run_formulas(res.returns.tolist(), res.lengths.tolist(), res.successes.tolist()), triple
        assert np.array_equal(res.envs, np.arange(EPISODES) % n)
    ev.evaluate(2)
    first = ev.key
    ev.evaluate(2)
    assert ev.key != first and first > 9                         # keys never repeat, explicit ones included


# ------------------------------------------------------------------------------------------ 4. nothing else moves
def _bag_snapshot(agent):
    return agent.bag.obss.tobytes(), np.asarray(agent.bag.actions).tobytes(), agent.bag.pos


def check_nothing_else_moves(lib, device, steps=24):
    from dtqn_amd.agents.device_bag import DeviceBagVectorActor
    from device_rollout_helpers import replay_arrays
    agent = make_agent(lib, device, "car", scaled=True)
    agent.eval_on()
    agent.context_reset(np.array([0.1, 0.0, 0.0]))
    agent.eval_off()
    agent.context_reset(np.array([-0.1, 0.0, 0.0]))
    agent.bag.add(np.array([0.3, 0.0, 0.0]), 1)
    ev = make_evaluator(agent, "car")
    before, bag_before = _agent_snapshot(agent), _bag_snapshot(agent)
    ev.evaluate(EPISODES)
    ev.evaluate(2, key=1)
    assert ev.bag_counters()["choices"] > 0
    _assert_same(before, _agent_snapshot(agent))
    assert bag_before == _bag_snapshot(agent)
    # a device rollout of the same network, parameters frozen: the same replay and bag bytes with evaluations between its steps and without
    out = []
    for interleave in (False, True):
        ag = make_agent(lib, device, "car", scaled=True)
        actor = DeviceBagVectorActor(ag, ENV_ID["car"], N, 5, max_episode_steps=CAP)
        ev2 = make_evaluator(ag, "car")
        for k in range(steps):
            actor.step_all(0.3)
            if interleave and k % 5 == 2:
                ev2.evaluate(3)
        got = actor.sync()
        assert got["committed"] >= 3
        out.append((replay_arrays(ag.replay_buffer), got, list(ag.replay_buffer.pos), ag._actor_calls, actor.get_state().bag.raw.tobytes()))
    (ra, ga, pa, da, ba), (rb_, gb, pb, db, bb) = out
    assert ga == gb and pa == pb and da == db and ba == bb
    for key in ra:
        assert ra[key].tobytes() == rb_[key].tobytes(), key


# ------------------------------------------------------------------------------------------ 5. dropout
def check_dropout_is_off(lib, device):
    plain, drop = make_agent(lib, device, "car", scaled=True), make_agent(lib, device, "car", scaled=True, dropout=0.1)
    assert drop.policy_network.dropout_p == 0.1 and plain.policy_network.dropout_p == 0.0
    drop.policy_network.load_state_dict({k: v.clone() for k, v in plain.policy_network.state_dict().items()})
    assert drop.engine.theta_pol.cpu().numpy().tobytes() == plain.engine.theta_pol.cpu().numpy().tobytes()
    assert drop.train_mode.name == "TRAIN"
    out = []
    for agent in (plain, drop):
        ev = make_evaluator(agent, "car")
        triple = ev.evaluate(EPISODES, key=4)
        st = ev.get_state()
        assert st.bag.counters[1] > 0
        out.append((triple, st.results.tobytes(), ev.q_rows().tobytes(), st.bag.raw.tobytes()))
    assert out[0] == out[1]


# ------------------------------------------------------------------------------------------ 6. run.py
def check_run_py(lib, device, monkeypatch, tmp_path):
    import pytest
    import run as runpy
    from dtqn_amd.agents import device_bag_eval
    from device_rollout_helpers import _patch_emu
    _patch_emu(lib, monkeypatch)
    monkeypatch.chdir(tmp_path)
    made = []
    init = device_bag_eval.DeviceBagEvaluator.__init__

    def recording_init(self, *a, **k):
        init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(device_bag_eval.DeviceBagEvaluator, "__init__", recording_init)
    common = ("--envs DiscreteCarFlag-v0 --sampler device --in-embed 64 --context 6 --batch 2 --num-steps 24 --prepopulate 60 "
              "--max-episode-steps 12 --history 6 --heads 8 --layers 1 --buf-size 240 --eval-frequency 12 --eval-episodes 2 --disable-wandb "
              f"--device {device}")
    assert runpy.get_args(common.split()).device_bag_eval_envs == 0
    agent = runpy.run_experiment(runpy.get_args((common + " --bag-size 2 --device-envs 3 --device-bag-eval-envs 2 --project-name bageval").split()))
    assert agent.num_train_steps == 24 and len(made) == 1
    ev = made[0]
    files = glob.glob(str(tmp_path / "policies" / "bageval" / "**" / "*_results.csv"), recursive=True)
    assert len(files) == 1
    rows = open(files[0], newline="").read().splitlines()
    assert len(rows) == 3 and [r.split(",")[1] for r in rows[1:]] == ["0", "12"]
    for row in rows[1:]:
        assert all(np.isfinite(float(v)) for v in row.split(","))
    bags = ev.bag_counters()
    assert ev.n == 2 and ev.key == 1 and ev.poll()["finished"] == 2, (ev.key, ev.poll())          # the evaluator played both evaluations
    assert bags["appends"] > 0 and bags["cleared"] >= 4 and ev.vector_steps > 0, (bags, ev.vector_steps)
    refused = ((" --bag-size 2 --device-bag-eval-envs 2 --eval-envs 2", ValueError), (" --bag-size 2 --device-bag-eval-envs 2 --device-eval-envs 2", ValueError),
               (" --device-bag-eval-envs 2", ValueError), (" --bag-size 2 --device-bag-eval-envs -1", ValueError))
    for extra, exc in refused:
        with pytest.raises(exc):
            runpy.run_experiment(runpy.get_args((common + extra + " --project-name refused").split()))
    with pytest.raises(NotImplementedError, match="--device-bag-eval-envs"):       # the bag-less evaluator names the switch
        runpy.run_experiment(runpy.get_args((common + " --bag-size 2 --device-eval-envs 2 --project-name refused").split()))
    monkeypatch.setattr(runpy.ddp, "init_from_env", lambda *a, **k: (0, 2, 0))
    with pytest.raises(NotImplementedError):
        runpy.run_experiment(runpy.get_args((common + " --bag-size 2 --device-bag-eval-envs 2 --project-name refused").split()))


# ------------------------------------------------------------------------------------------ 7. refusals
def check_refusals(lib, device):
    import pytest
    from dtqn_amd import _binding as B
    from dtqn_amd.agents.device_bag_eval import DeviceBagEvaluator
    from dtqn_amd.agents.device_eval import DeviceEvaluator
    import device_rollout_helpers as R
    CONFIG, ARG = B.DEFINES["DTQN_ERR_CONFIG"], B.DEFINES["DTQN_ERR_ARG"]
    plain = R.make_agent(lib, device, "car")
    with pytest.raises(ValueError):                               # an agent without a bag
        DeviceBagEvaluator(plain, ENV_ID["car"], N, 0, max_episode_steps=CAP)
    agent = make_agent(lib, device, "car")
    with pytest.raises(NotImplementedError):                      # everything DeviceEvaluator refuses
        DeviceBagEvaluator(agent, "CartPole-v1", N, 0)
    with pytest.raises(ValueError):
        DeviceBagEvaluator(agent, ENV_ID["car"], 0, 0, max_episode_steps=CAP)
    with pytest.raises(NotImplementedError):                      # DeviceEvaluator keeps refusing bag agents
        DeviceEvaluator(agent, ENV_ID["car"], N, 0, max_episode_steps=CAP)
    ev = make_evaluator(agent)
    lib_, net = ev._lib_args()
    stream, theta = agent.engine._stream(), agent._theta_p
    begin = lambda net_=net, e=ev._ev_ref, bag=ev._bag_ref, episodes=2: lib_.dtqn_deval_begin_bag(net_, e, bag, 1, episodes, stream)
    step = lambda net_=net, e=ev._ev_ref, bag=ev._bag_ref, cur=0, n_max=1, episodes=2, th=theta: lib_.dtqn_deval_step_bag(
        net_, th, e, bag, 1, 0, cur, n_max, episodes, 0, stream)
    assert begin() == 0 and step() == 0
    assert begin(bag=None) == ARG and step(bag=None) == ARG       # a NULL bag descriptor
    ev.bag_desc.n_envs = N + 1
    assert begin() == ARG and step() == ARG                       # the bag descriptor and the evaluation's disagree
    ev.bag_desc.n_envs = N
    q_cand = ev.bag_desc.q_cand
    ev.bag_desc.q_cand = None
    assert step() == ARG
    ev.bag_desc.q_cand = q_cand
    assert step(cur=2) == ARG and step(cur=-1) == ARG
    assert step(n_max=0) == ARG and step(n_max=L + 1) == ARG
    assert begin(episodes=-1) == ARG and begin(episodes=ev.max_episodes + 1) == ARG
    assert step(episodes=-1) == ARG and step(episodes=ev.max_episodes + 1) == ARG
    assert begin() == 0 and step() == 0
    # a network without a bag: DTQN_ERR_CONFIG, whatever the bag descriptor says
    from device_eval_helpers import make_evaluator as make_plain_evaluator
    other = make_plain_evaluator(plain, "car")
    lib2, net2 = other._lib_args()
    assert lib2.dtqn_deval_begin_bag(net2, other._ev_ref, ev._bag_ref, 1, 2, plain.engine._stream()) == CONFIG
    assert lib2.dtqn_deval_step_bag(net2, plain._theta_p, other._ev_ref, ev._bag_ref, 1, 0, 0, 1, 2, 0, plain.engine._stream()) == CONFIG
    # the evaluation's own entry points still refuse a bag network
    assert lib_.dtqn_deval_begin(net, ev._ev_ref, 1, 2, stream) == CONFIG
    assert lib_.dtqn_deval_step(net, theta, ev._ev_ref, 1, 0, 0, 1, 2, stream) == CONFIG
