"""Shared by test_emu_device_bag.py (HIP emulation on the CPU) and test_gpu_device_bag.py (MI355X): the device-resident rollout of a
bag network (csrc/dtqn_devbag.hip, dtqn_amd.agents.device_bag.DeviceBagVectorActor) against a host Context + Bag per environment and
DtqnAgent._bag_forward.

Shapes, the smallest that can still go wrong: d_model 64 / 8 heads / 1 layer, context L = 6, bag K = 2, N = 3 environments, a step
cap of 12 -- a window slides from step 6 on, steps 6-7 append, steps 8-11 choose among K + 1 = 3 candidates, step 12 truncates.

The host never draws or decides: after every vector step both device states are read back and each environment's host Context + Bag
replay what the device did (its action, its new observation, its choice).  What is compared is the bag bookkeeping and the scores."""
import numpy as np
import torch

from device_rollout_helpers import f32_bits

N, E, L, K, CAP, PAIRS = 3, 5, 6, 2, 12, 2
ENV_ID = {"car": "DiscreteCarFlag-v0", "mem": "Memory-5-v0", "tiger": "POMDP-tiger-episodic-v0"}


def host_env(kind):
    from dtqn_amd import envs
    from dtqn_amd.envs import CarFlag, Memory, TimeLimit
    if kind == "car":
        return TimeLimit(CarFlag(discrete=True), CAP)
    if kind == "mem":
        return TimeLimit(Memory(num_pairs=PAIRS), CAP)
    return envs.make(ENV_ID["tiger"], max_episode_steps=CAP)


def make_agent(lib, device, kind="car", a_embed=0, scaled=False, bag_size=K, dropout=0.0, seed=11, q_scale=100.0):
    """An agent as run.py builds it for the small environment; lib: the emulation library (agent on the CPU) or None.  scaled: a
    network in which the bag moves Q (fresh weights leave candidate gaps of 0 .. 5e-6 against a tolerance of 3e-4): bag_attention
    weights x 30, observation embedding weights x 10, on top of the Q head x 100 every test here uses."""
    from dtqn_amd.networks.dtqn import DTQN
    from dtqn_amd.utils import agent_utils
    from dtqn_amd.utils.random import set_global_seed
    env = host_env(kind)
    set_global_seed(seed, env)
    orig = agent_utils.MODEL_MAP["DTQN"]
    if lib is not None:
        def emu_dtqn(*a, **k):
            m = DTQN(*a, _test_lib=lib, **k)
            m._allow_cpu = True
            return m
        agent_utils.MODEL_MAP["DTQN"] = emu_dtqn
    try:
        agent = agent_utils.get_agent("DTQN", [env], 8, a_embed, 64, E * CAP, device, 3e-4, 2, L, CAP, L, 1000, 0.99, 8, 1, dropout, False, "res",
                                      "learned", bag_size, sampler="device", sample_seed=seed)
    finally:
        agent_utils.MODEL_MAP["DTQN"] = orig
    sd = {k: v.clone() for k, v in agent.policy_network.state_dict().items()}
    sd["ffn.2.weight"] = sd["ffn.2.weight"] * q_scale
    if scaled:
        for k in sd:
            if k.startswith("bag_attention") and k.endswith("weight"):
                sd[k] = sd[k] * 30.0
            if k.startswith("obs_embedding") and k.endswith("weight"):
                sd[k] = sd[k] * 10.0
    agent.policy_network.load_state_dict(sd)
    agent.target_update()
    assert agent.replay_buffer.max_size == E and agent.replay_buffer.max_episode_steps == CAP
    return agent


def make_actor(agent, kind="car", n=N, seed=5):
    from dtqn_amd.agents.device_bag import DeviceBagVectorActor
    return DeviceBagVectorActor(agent, ENV_ID[kind], n, seed, max_episode_steps=CAP, num_pairs=PAIRS if kind == "mem" else None)


def q_tol(*qs):
    """The project's Q tolerance: 1e-4 max(1, |Q|max).  A mean of row maxima is bounded by it."""
    return 1e-4 * max(1.0, max(float(np.abs(np.asarray(q)).max()) for q in qs))


def _to_np(q):
    return q.detach().cpu().numpy() if isinstance(q, torch.Tensor) else np.asarray(q)


class Replay:
    """N host Context + Bag pairs that replay the device, one vector step at a time; every step is checked in full (the evicted pair,
    append, clear, idle, candidates, scores, choice) and counted in `seen`."""

    def __init__(self, agent, actor, check_q=False):
        from dtqn_amd.utils.bag import Bag
        from dtqn_amd.utils.context import Context
        self.agent, self.actor, self.check_q = agent, actor, check_q
        self.n = actor.n
        mk = lambda: Context(L, agent.obs_mask, agent.num_actions, agent.env_obs_length, discrete=agent.is_discrete_env)
        self.ctx = [mk() for _ in range(self.n)]
        self.bags = [Bag(agent.bag.size, agent.obs_mask, agent.env_obs_length, discrete=agent.is_discrete_env) for _ in range(self.n)]
        self.st = actor.get_state()
        for i in range(self.n):
            self._begin(i, self.st)
        self.seen = dict(steps=0, evicted=0, appends=0, choices=0, kept=0, cleared=0, idle=0, decisive=0, ragged=0, q_checked=0, q_moved=0)
        self.by_env = [dict(appends=0, choices=0) for _ in range(self.n)]
        self.episodes = [[np.array(self.st.block.obs[i, 0], copy=True)] for i in range(self.n)]
        self.finished = []                                # (first observation, [(obs, action, reward, stored done)]) in commit order

    def _begin(self, i, st):
        self.ctx[i].reset(np.array(st.block.obs[i, 0], copy=True))
        self.ctx[i].action[0, 0] = st.block.actions[i, 0]          # the padding action of row 0 is a draw of the device's
        self.bags[i].reset()

    def _bag_bits(self, bag):
        return f32_bits(bag.obss).tobytes(), np.asarray(bag.actions, dtype=np.uint8).reshape(-1).tobytes()

    def _assert_bag(self, i, st, where):
        obs, act = self._bag_bits(self.bags[i])
        assert f32_bits(st.bag.obs[i]).tobytes() == obs and st.bag.actions[i].tobytes() == act, (where, i, st.bag.obs[i], self.bags[i].obss)
        assert st.bag.pos[i] == self.bags[i].pos, (where, i, st.bag.pos, self.bags[i].pos)

    def host_q_last(self, i, cleared=False):
        """Q of the last live row of environment i's context with its bag (or a cleared one), through the module forward."""
        ctx, bag = self.ctx[i], self.bags[i]
        n = min(L, ctx.timestep + 1)
        obss, acts = bag.make_empty_bag() if cleared else (bag.obss, bag.actions)
        with torch.no_grad():
            q = self.agent._bag_forward(ctx.obs[None, :n], ctx.action[None, :n], obss[None], acts[None])
        return _to_np(q)[0, -1]

    def step(self, forced=None, epsilon=1.0, store=False):
        agent, actor, before = self.agent, self.actor, self.st
        Kb = agent.bag.size
        if self.check_q and epsilon < 1.0:
            q_ref = [self.host_q_last(i) for i in range(self.n)]
            q_bare = [self.host_q_last(i, cleared=True) for i in range(self.n)]
            self.seen["ragged"] += len(set(int(v) for v in before.block.lens)) > 1
        actor.set_forced(forced)
        actor.step_all(epsilon, store=store)
        st = self.st = actor.get_state()
        self.seen["steps"] += 1
        if self.check_q and epsilon < 1.0:
            q_dev = actor.q_rows()
            for i in range(self.n):
                tol = q_tol(q_ref[i])
                assert np.isfinite(q_dev[i]).all() and np.abs(q_dev[i] - q_ref[i]).max() <= tol, (i, q_dev[i], q_ref[i], tol)
                if self.bags[i].pos > 0:
                    self.seen["q_checked"] += 1
                    self.seen["q_moved"] += bool(np.abs(q_dev[i] - q_bare[i]).max() > tol)
        for i in range(self.n):
            where = (self.seen["steps"], i)
            action, done, stored = int(st.last[i, 0]), bool(st.last[i, 2]), bool(st.last[i, 3])
            t = int(before.elapsed[i]) + 1
            obs = np.array(st.stage_obs[i, t], copy=True)
            self.episodes[i].append((obs, action, float(st.reward[i]), stored))
            assert st.bag.choosing[i] == 0, where
            if done:                                               # observe, then context_reset -> bag.reset(): the bag ends up cleared
                self.finished.append(self.episodes[i])
                self._begin(i, st)
                self.episodes[i] = [np.array(st.block.obs[i, 0], copy=True)]
                self._assert_bag(i, st, where)
                assert (st.bag.obs[i] == np.float32(agent.obs_mask)).all() and not st.bag.actions[i].any() and st.bag.choice[i] == -1, where
                self.seen["cleared"] += 1
                continue
            ev_obs, ev_act = self.ctx[i].add_transition(obs, action, float(st.reward[i]), stored)
            if ev_obs is None:                                     # nothing evicted, no reset: the bag bytes stay
                assert st.bag.choice[i] == -1 and st.bag.obs[i].tobytes() == before.bag.obs[i].tobytes(), where
                assert st.bag.actions[i].tobytes() == before.bag.actions[i].tobytes() and st.bag.pos[i] == before.bag.pos[i], where
                self.seen["idle"] += 1
                continue
            # the pair the device takes is Context.add_transition's return value: the observation of row 0 of the block the step read,
            # and -- the returned action is a view of the row the new action is then written to -- this step's action
            self.seen["evicted"] += 1
            ev_act = int(np.asarray(ev_act).reshape(-1)[0])
            assert f32_bits(before.block.obs[i, 0]).tobytes() == f32_bits(ev_obs).tobytes() and ev_act == action, where
            bag = self.bags[i]
            if bag.add(ev_obs, ev_act):
                assert st.bag.choice[i] == -1, where
                self._assert_bag(i, st, where)
                self.seen["appends"] += 1
                self.by_env[i]["appends"] += 1
                continue
            # a choice: the K + 1 candidates as _bag_insert builds them, from the bag before
            C = Kb + 1
            cand_obss, cand_actions = np.tile(bag.obss, (C, 1, 1)), np.tile(bag.actions, (C, 1, 1))
            for c in range(Kb):
                cand_obss[c, c], cand_actions[c, c] = ev_obs, ev_act
            assert f32_bits(st.bag.cand_obs[i]).tobytes() == f32_bits(cand_obss).tobytes(), where
            assert st.bag.cand_actions[i].tobytes() == cand_actions.astype(np.uint8).reshape(-1).tobytes(), where
            ctx = self.ctx[i]
            with torch.no_grad():
                q = agent._bag_forward(np.tile(ctx.obs, (C, 1, 1)), np.tile(ctx.action, (C, 1, 1)), cand_obss, cand_actions)
                host = _to_np(torch.mean(torch.max(q, 2)[0], 1))
            tol = q_tol(_to_np(q))
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
            self.by_env[i]["choices"] += 1
        c = st.bag.counters
        assert (int(c[0]), int(c[1]), int(c[2]), int(c[3])) == tuple(self.seen[k] for k in ("appends", "choices", "kept", "cleared")), (c, self.seen)
        return st


def moving_actions(k, n=N):
    """CarFlag: pushes that change with the step and the environment, so that observations differ from row to row."""
    return [(k // 2 + i) % 3 if (k + i) % 4 else 2 for i in range(n)]


# ------------------------------------------------------------------------------------------ 1. bookkeeping
def check_bookkeeping(lib, device, kind, a_embed=0, steps=30):
    agent = make_agent(lib, device, kind, a_embed=a_embed)
    actor = make_actor(agent, kind)
    rep = Replay(agent, actor)
    rng = np.random.default_rng(3)
    for k in range(steps):
        if kind == "car":
            forced = moving_actions(k)
        elif kind == "tiger":
            forced = [0] * N                                      # listen: the episode runs into the cap
        else:                                                     # Memory: mostly the shown card itself, a miss -- episodes reach the cap
            forced = [int(rep.st.env_i32[i, 0]) if rng.random() < 0.9 else int(rng.integers(0, agent.num_actions)) for i in range(N)]
        rep.step(forced)
    seen = rep.seen
    print(kind, seen)
    assert seen["appends"] >= K * N and seen["cleared"] >= N and seen["idle"] >= L - 1 and seen["evicted"] == seen["appends"] + seen["choices"], seen
    assert seen["choices"] >= 2 * N, seen


# ------------------------------------------------------------------------------------------ 2. / 3. / 4. scores, choice, acting
def check_scores_and_choice(lib, device, steps=36):
    """CarFlag with the scaled weights and actions that move the car: every score against the host forward, every choice the first
    arg-max of the device's scores, and at least half of the choices decisive (then the device's bag is the host's best candidate)."""
    agent = make_agent(lib, device, "car", scaled=True)
    actor = make_actor(agent, "car")
    rep = Replay(agent, actor)
    for k in range(steps):
        rep.step(moving_actions(k))
    seen = rep.seen
    print(seen)
    assert seen["choices"] >= 24, seen
    assert 2 * seen["decisive"] >= seen["choices"], f"{seen['decisive']} of {seen['choices']} choices were decisive"


def check_acting_uses_the_bag(lib, device, steps=14):
    agent = make_agent(lib, device, "car", scaled=True)
    actor = make_actor(agent, "car")
    rep = Replay(agent, actor, check_q=True)
    for k in range(steps):
        rep.step(moving_actions(k), epsilon=0.0)
    seen = rep.seen
    print(seen)
    assert seen["q_checked"] >= 4 * N and seen["q_moved"] == seen["q_checked"], seen


# ------------------------------------------------------------------------------------------ 5. ragged phases
def check_ragged_phases(lib, device):
    """Environment 2 restarts its episode after 5 vector steps (set_state): the others choose at steps 8-11 while it still fills its
    context, and it appends when they truncate."""
    agent = make_agent(lib, device, "car", scaled=True)
    actor = make_actor(agent, "car")
    rep = Replay(agent, actor, check_q=True)
    for k in range(5):
        rep.step(moving_actions(k), epsilon=0.0)
    st = rep.st
    late = 2
    st.elapsed[late], st.ep_ret[late], st.block.lens[late] = 0, 0.0, 1
    st.stage_obs[late, 0] = st.block.obs[late, 0]
    actor.set_state(st)
    rep.st = actor.get_state()
    rep._begin(late, rep.st)
    rep.episodes[late] = [np.array(rep.st.block.obs[late, 0], copy=True)]
    for k in range(5, 12):
        rep.step(moving_actions(k), epsilon=0.0)
    print(rep.by_env, rep.seen)
    assert rep.by_env[0]["choices"] == 4 and rep.by_env[1]["choices"] == 4 and rep.by_env[late]["choices"] == 0, rep.by_env
    assert rep.by_env[late]["appends"] >= 1 and rep.seen["ragged"] >= 1, (rep.by_env, rep.seen)


# ------------------------------------------------------------------------------------------ 6. determinism
def check_determinism(lib, device, steps=24):
    raws = []
    for _ in range(2):
        agent = make_agent(lib, device, "car", scaled=True)
        actor = make_actor(agent, "car", seed=9)
        for _ in range(steps):
            actor.step_all(0.3)
        st = actor.get_state()
        assert st.bag.counters[1] > 0
        raws.append((st.raw.tobytes(), st.bag.raw.tobytes()))
    assert raws[0] == raws[1]


# ------------------------------------------------------------------------------------------ 7. replay and accounting
def check_replay_and_accounting(lib, device, steps=40):
    agent = make_agent(lib, device, "car")
    actor = make_actor(agent, "car")
    rep = Replay(agent, actor)
    for k in range(steps):
        rep.step(moving_actions(k), store=True)
    got = actor.sync()                                            # raises on any counter mismatch
    assert got["committed"] == got["staged"] == len(rep.finished) > E and got["env_steps"] == steps * N, (got, len(rep.finished))
    d = agent.replay_buffer.dev
    obs, act, rew, don, ep_len = (getattr(d, k).cpu().numpy() for k in ("obs", "actions", "rewards", "dones", "ep_len"))
    for e in range(len(rep.finished) - E, len(rep.finished)):     # the episodes the ring still holds
        ep, slot = rep.finished[e], (actor.pos0 + e) % E
        n = len(ep) - 1
        assert ep_len[slot] == n, (e, slot, ep_len, n)
        assert f32_bits(obs[slot, 0]).tobytes() == f32_bits(ep[0]).tobytes()
        for t, (o, a, r, dn) in enumerate(ep[1:]):
            assert f32_bits(obs[slot, t + 1]).tobytes() == f32_bits(o).tobytes() and act[slot, t] == a, (e, t)
            assert rew[slot, t] == np.float32(r) and bool(don[slot, t]) == dn, (e, t)
    assert actor.bag_counters() == {k: int(rep.seen[k]) for k in ("appends", "choices", "kept", "cleared")}


# ------------------------------------------------------------------------------------------ 8. run.py
def check_run_py(lib, device, monkeypatch, tmp_path):
    import run as runpy
    from dtqn_amd.agents import device_bag
    from device_rollout_helpers import _patch_emu
    _patch_emu(lib, monkeypatch)
    monkeypatch.chdir(tmp_path)
    made = []
    init = device_bag.DeviceBagVectorActor.__init__

    def recording_init(self, *a, **k):
        init(self, *a, **k)
        made.append(self)
    monkeypatch.setattr(device_bag.DeviceBagVectorActor, "__init__", recording_init)
    common = ("--envs DiscreteCarFlag-v0 --sampler device --in-embed 64 --context 6 --batch 2 --num-steps 24 --prepopulate 60 "
              "--max-episode-steps 12 --history 6 --heads 8 --layers 1 --buf-size 240 --eval-frequency 12 --eval-episodes 2 --disable-wandb "
              f"--bag-size 2 --device {device}")
    agent = runpy.run_experiment(runpy.get_args((common + " --device-envs 3 --project-name devbag").split()))
    assert agent.num_train_steps == 24 and len(made) == 1           # training updates ran, on the bag actor
    actor = made[0]
    got, bags = actor.counters(), actor.bag_counters()
    assert got["env_steps"] == actor.steps >= 60 + 24 and got["committed"] == got["staged"] >= 3, got
    assert bags["appends"] > 0 and bags["choices"] > 0 and bags["cleared"] > 0 and 0 < actor.choice_steps < actor.vector_steps, (bags, actor.choice_steps)
    rb = agent.replay_buffer
    assert rb.pos[0] >= 3 and rb.pos[1] == 0 and np.array_equal(rb.episode_lengths, rb.dev.ep_len.cpu().numpy())
    import pytest
    with pytest.raises(NotImplementedError):                      # evaluation of a bag run stays on the host
        runpy.run_experiment(runpy.get_args((common + " --device-envs 3 --device-eval-envs 2 --project-name refused").split()))


# ------------------------------------------------------------------------------------------ 9. refusals
def check_refusals(lib, device):
    import ctypes
    import pytest
    from dtqn_amd import _binding as B
    from dtqn_amd.agents.device_bag import DeviceBagVectorActor
    from dtqn_amd.agents.device_rollout import DeviceVectorActor
    import device_rollout_helpers as R
    CONFIG, ARG = B.DEFINES["DTQN_ERR_CONFIG"], B.DEFINES["DTQN_ERR_ARG"]
    plain = R.make_agent(lib, device, "car")
    with pytest.raises(ValueError):                               # an agent without a bag
        DeviceBagVectorActor(plain, ENV_ID["car"], N, 0, max_episode_steps=R.CAR_CAP)
    with pytest.raises(NotImplementedError):                      # dropout
        make_actor(make_agent(lib, device, "car", dropout=0.1))
    agent = make_agent(lib, device, "car")
    with pytest.raises(NotImplementedError):                      # everything DeviceVectorActor refuses
        DeviceBagVectorActor(agent, "CartPole-v1", N, 0)
    with pytest.raises(ValueError):
        DeviceBagVectorActor(agent, ENV_ID["car"], 0, 0, max_episode_steps=CAP)
    image = make_agent(lib, device, "car")
    image.image = (1, 24, 24)
    with pytest.raises(NotImplementedError):
        make_actor(image)
    actor = make_actor(agent)
    lib_, net, rp = actor._lib_args()
    stream = agent.engine._stream()
    step = lambda net_, rp_, ro, bag: lib_.dtqn_rollout_step_bag(net_, agent._theta_p, rp_, ro, bag, 0, 0, 1, 1.0, 0, 0, 0, 0, 0, 0, 0, stream)
    assert step(net, rp, actor._ro_ref, None) == ARG              # a NULL bag descriptor
    assert lib_.dtqn_rollout_reset_bag(net, rp, actor._ro_ref, None, 0, stream) == ARG
    q_cand = actor.bag_desc.q_cand
    actor.bag_desc.q_cand = None
    assert step(net, rp, actor._ro_ref, actor._bag_ref) == ARG    # a NULL q_cand
    actor.bag_desc.q_cand = q_cand
    actor.bag_desc.n_envs = N + 1
    assert step(net, rp, actor._ro_ref, actor._bag_ref) == ARG    # the bag descriptor and the rollout's disagree
    actor.bag_desc.n_envs = N
    assert step(net, rp, actor._ro_ref, actor._bag_ref) == 0
    # a network without a bag: DTQN_ERR_CONFIG, whatever the bag descriptor says
    other = R.make_actor(plain, "car")
    lib2, net2, rp2 = other._lib_args()
    assert lib2.dtqn_rollout_step_bag(net2, plain._theta_p, rp2, other._ro_ref, actor._bag_ref, 0, 0, 1, 1.0, 0, 0, 0, 0, 0, 0, 0,
                                      plain.engine._stream()) == CONFIG
    assert lib2.dtqn_devbag_state_bytes(net2, actor._bag_ref, None) < 0
    # the rollout's own entry points still refuse a bag network (DeviceVectorActor: device_rollout_helpers.check_refusals is the witness)
    assert lib_.dtqn_rollout_step(net, agent._theta_p, rp, actor._ro_ref, 0, 0, 1, 1.0, 0, 0, 0, 0, 0, 0, stream) == CONFIG
    assert lib_.dtqn_rollout_reset(net, rp, actor._ro_ref, 0, stream) == CONFIG
    with pytest.raises(NotImplementedError):
        DeviceVectorActor(agent, ENV_ID["car"], N, 0, max_episode_steps=CAP)
