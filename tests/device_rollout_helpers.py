"""Shared by test_emu_device_rollout.py (HIP emulation on the CPU) and test_gpu_device_rollout.py (MI355X): the device-resident
rollout (csrc/dtqn_rollout.hip, dtqn_amd.agents.device_rollout.DeviceVectorActor) against the host environments, the host Context,
the host ReplayBuffer producer API and dtqn_actor_forward_batch.

Shapes, the smallest that can still go wrong: d_model 64 / 4 heads / 1 layer / context 8 (windows slide after 8 steps), N = 3
environments, a replay of E = 5 slots (the ring wraps), CarFlag with a step cap of 12 (truncation happens), Memory with 2 pairs and a cap
of 6; one row-block network: d_model 128 with the GRU gate, context 8.

The host side never draws: where the device drew (a reset, Memory's next card) the host is given that draw, read back with get_state --
CarFlag by injecting the start state, Memory through a scripted `np_random` that replays the cards."""
import math

import numpy as np
import torch

from helpers import ptr

N, E, L = 3, 5, 8
CAR_CAP, MEM_CAP, MEM_PAIRS = 12, 6, 2
WHOLE = dict(d_model=64, heads=4, layers=1, gate="res")
ROWBLOCK = dict(d_model=128, heads=8, layers=1, gate="gru")
ENV_ID = {"car": "DiscreteCarFlag-v0", "mem": "Memory-5-v0"}


def host_env(kind):
    from dtqn_amd.envs import CarFlag, Memory, TimeLimit
    return TimeLimit(CarFlag(discrete=True), CAR_CAP) if kind == "car" else TimeLimit(Memory(num_pairs=MEM_PAIRS), MEM_CAP)


def make_agent(lib, device, kind, d_model=64, heads=4, layers=1, gate="res", context=L, slots=E, seed=11, batch=2, q_scale=100.0, sampler="device",
               bag_size=0):
    """An agent as run.py builds it (get_agent) for the small environment; kind: "car" / "mem", or the host environment itself (under
    its TimeLimit; pomdp_env_helpers.py passes its model's); lib: the emulation library (agent on the CPU) or None."""
    from dtqn_amd.networks.dtqn import DTQN
    from dtqn_amd.utils import agent_utils
    from dtqn_amd.utils.random import set_global_seed
    env = host_env(kind) if isinstance(kind, str) else kind
    set_global_seed(seed, env)
    cap = env._max_episode_steps
    orig = agent_utils.MODEL_MAP["DTQN"]
    if lib is not None:
        def emu_dtqn(*a, **k):
            m = DTQN(*a, _test_lib=lib, **k)
            m._allow_cpu = True
            return m
        agent_utils.MODEL_MAP["DTQN"] = emu_dtqn
    try:
        agent = agent_utils.get_agent("DTQN", [env], 8, 0, d_model, slots * cap, device, 3e-4, batch, context, cap, context, 1000, 0.99, heads,
                                      layers, 0.0, False, gate, "learned", bag_size, sampler=sampler, sample_seed=seed)
    finally:
        agent_utils.MODEL_MAP["DTQN"] = orig
    if q_scale != 1.0:        # a fresh Q head gives rows of a few 1e-3: a head 100 x as steep, as after training
        sd = {k: v.clone() for k, v in agent.policy_network.state_dict().items()}
        sd["ffn.2.weight"] = sd["ffn.2.weight"] * q_scale
        agent.policy_network.load_state_dict(sd)
        agent.target_update()
    assert agent.replay_buffer.max_size == slots and agent.replay_buffer.max_episode_steps == cap
    return agent


def make_actor(agent, kind, n=N, seed=5):
    from dtqn_amd.agents.device_rollout import DeviceVectorActor
    return DeviceVectorActor(agent, ENV_ID[kind], n, seed, max_episode_steps=CAR_CAP if kind == "car" else MEM_CAP,
                             num_pairs=MEM_PAIRS if kind == "mem" else None)


def f32_bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


class ScriptedRandom:
    """np_random of a host Memory that replays the device's draws: shuffle() deals the device's cards, integers() hands out the
    device's shown cards in order (the rejection loop of memory_cards.py then accepts the first)."""

    def __init__(self):
        self.cards, self.next = None, []

    def shuffle(self, arr):
        arr[:] = self.cards

    def integers(self, *a, **k):
        return self.next.pop(0)          # (IndexError: the host wanted a draw the device did not make)


class HostMirror:
    """N host environments that replay what the device environments do.  begin(i, st): environment i starts the episode the device
    state `st` has just reset to; step(i, action, st_after) -> (obs, reward, done, info) of the host step."""

    def __init__(self, kind, n):
        self.kind, self.envs = kind, [host_env(kind) for _ in range(n)]
        for e in self.envs:
            e.env.np_random = ScriptedRandom()

    def begin(self, i, st):
        env = self.envs[i]
        if self.kind == "car":
            inner = env.env
            env._elapsed_steps = 0
            inner.heaven_position = float(st.env_f64[i, 3])
            inner.hell_position = -inner.heaven_position
            inner.state = np.array([st.env_f64[i, 0], 0, 0.0])          # car_flag.py:36
            assert st.env_f64[i, 1] == 0.0 and st.env_f64[i, 2] == 0.0
            return np.array(inner.state)
        C = 2 * MEM_PAIRS
        rnd = env.env.np_random
        rnd.cards, rnd.next = st.env_i32[i, 1:1 + C].astype(np.int64), [int(st.env_i32[i, 0])]
        assert sorted(rnd.cards.tolist()) == sorted(list(range(1, MEM_PAIRS + 1)) * 2), rnd.cards
        return env.reset()

    def step(self, i, action, st_after):
        env = self.envs[i]
        if self.kind == "mem":
            if st_after.last[i, 4]:       # truncated: the card was drawn and shown, then the reset took the state -- it is the face-up one
                shown = st_after.stage_obs[i, env._elapsed_steps + 1]
                nxt = [int(j) for j in np.nonzero((shown >= 1) & (shown <= MEM_PAIRS))[0]]
                assert len(nxt) == 1, shown
            else:
                nxt = [] if st_after.last[i, 2] else [int(st_after.env_i32[i, 0])]
            env.env.np_random.next = nxt
        out = env.step(int(action))
        if self.kind == "mem":
            assert not env.env.np_random.next, "the device drew a card the host did not ask for"
        return out


def check_step_against_host(kind, i, st, t, obs, reward, done, info, where=""):
    """Device environment i after its step number t (1-based) of the episode: the stored observation (f32 bits), reward, done and the
    stored done against the host's step."""
    truncated = bool(info.get("TimeLimit.truncated", False))
    stored = False if truncated else bool(done)
    assert np.array_equal(f32_bits(st.stage_obs[i, t]), f32_bits(obs)), (where, i, t, st.stage_obs[i, t], obs)
    assert f32_bits(st.reward[i]) == f32_bits(reward), (where, i, t, st.reward[i], reward)
    assert st.stage_rew[i, t - 1] == np.float32(reward) and st.stage_done[i, t - 1] == int(stored), (where, i, t)
    assert (bool(st.last[i, 2]), bool(st.last[i, 3]), bool(st.last[i, 4])) == (bool(done), stored, truncated), (where, i, t, st.last[i], done, info)
    return stored


# ------------------------------------------------------------------------------------------ 1. CarFlag dynamics
def car_scenarios():
    """(position, velocity, heaven side, steps already taken, actions)."""
    lo, hi = 0.5 - 0.2, 0.5 + 0.2
    out = [
        (0.0, 0.0695, 1.0, 0, [2, 2, 2, 1, 0]),                   # the speed clamp at +0.07 ...
        (0.0, -0.0695, -1.0, 0, [0, 0, 0, 1, 2]),                 # ... and at -0.07
        (-1.06, -0.06, 1.0, 0, [0]),                              # the left wall: clamped to -1.1, velocity zeroed; hell (heaven right)
        (-1.06, -0.06, -1.0, 0, [0]),                             # the same wall with heaven on the left
        (0.95, 0.06, 1.0, 0, [2]),                                # reaching heaven: +1
        (0.95, 0.06, -1.0, 0, [2]),                               # reaching hell: -1
        (-0.95, -0.06, -1.0, 3, [0]),                             # heaven on the left: +1
        (0.0, 0.0, 1.0, CAR_CAP - 2, [1, 1]),                     # truncation at the cap: done, stored as not done
        (0.95, 0.06, 1.0, CAR_CAP - 1, [2]),                      # a real end on the cap's step is not a truncation
        (0.31, 0.069, -1.0, 0, [2, 2, 2, 2, 2, 2, 2]),            # through the priest zone and out of it again
    ]
    for side in (1.0, -1.0):                                      # both edges of the priest zone, coasting at rest: on the edge and next to it
        for p in (lo, np.nextafter(lo, -np.inf), hi, np.nextafter(hi, np.inf), np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf)):
            out.append((float(p), 0.0, side, 0, [1, 1]))
    return out


def check_carflag_dynamics(lib, device):
    from dtqn_amd.envs import CarFlag, TimeLimit
    agent = make_agent(lib, device, "car")
    actor = make_actor(agent, "car")
    scen = car_scenarios()
    rng = np.random.default_rng(3)
    for _ in range(6):                                            # and random walks from random states
        scen.append((float(rng.uniform(-0.9, 0.9)), float(rng.uniform(-0.07, 0.07)), float(rng.choice([-1.0, 1.0])), 0,
                     rng.integers(0, 3, size=CAR_CAP).tolist()))
    seen = dict(clamp=0, wall=0, plus=0, minus=0, trunc=0, zone=0)
    for g in range(0, len(scen), N):
        group = scen[g:g + N]
        st = actor.get_state()
        hosts = []
        for i, (p, v, side, e0, _) in enumerate(group):
            st.env_f64[i] = (p, v, 0.0, side)
            st.elapsed[i] = e0
            env = TimeLimit(CarFlag(discrete=True), CAR_CAP)
            env._elapsed_steps = e0
            env.env.heaven_position, env.env.hell_position = side, -side
            env.env.state = np.array([p, v, 0.0])
            hosts.append(env)
        actor.set_state(st)
        alive = [True] * len(group)
        for k in range(max(len(s[4]) for s in group)):
            forced = [1] * N
            for i, s in enumerate(group):
                if alive[i] and k < len(s[4]):
                    forced[i] = s[4][k]
            actor.set_forced(forced)
            actor.step_all(1.0, store=False)
            st = actor.get_state()
            for i, s in enumerate(group):
                if not alive[i] or k >= len(s[4]):
                    alive[i] = False
                    continue
                obs, r, done, info = hosts[i].step(forced[i])
                t = s[3] + k + 1
                assert st.last[i, 0] == forced[i] and st.last[i, 1] == 0
                check_step_against_host("car", i, st, t, obs, r, done, info, where=s)
                if done:
                    alive[i] = False
                    assert st.elapsed[i] == 0 and bool(st.last[i, 5]) == bool(info["is_success"])
                else:
                    assert np.array_equal(st.env_f64[i, :3].view(np.uint64), np.asarray(obs, dtype=np.float64).view(np.uint64)), (s, k)
                    assert st.elapsed[i] == t
                seen["clamp"] += abs(obs[1]) == 0.07
                seen["wall"] += obs[0] == -1.1 and obs[1] == 0
                seen["plus"] += r == 1.0
                seen["minus"] += r == -1.0
                seen["trunc"] += bool(info.get("TimeLimit.truncated", False))
                seen["zone"] += obs[2] != 0
    assert all(v > 0 for v in seen.values()), seen
    actor.set_forced(None)


# ------------------------------------------------------------------------------------------ 2. Memory
def check_memory_dynamics(lib, device, steps=24):
    """Environment 0 always points at the twin (its episodes complete), environment 1 at a card that has left the table whenever there
    is one (else at the shown card itself: a miss), environment 2 alternates; every step of every environment against the host."""
    agent = make_agent(lib, device, "mem")
    actor = make_actor(agent, "mem")
    mirror = HostMirror("mem", N)
    C, removed = 2 * MEM_PAIRS, MEM_PAIRS + 1
    st = actor.get_state()
    for i in range(N):
        obs0 = mirror.begin(i, st)
        assert np.array_equal(f32_bits(st.stage_obs[i, 0]), f32_bits(obs0)) and np.array_equal(f32_bits(st.block.obs[i, 0]), f32_bits(obs0))
    seen = dict(completed=0, onto_removed=0, truncated=0, miss=0)
    for k in range(steps):
        forced = []
        for i in range(N):
            cur, hidden, shown = int(st.env_i32[i, 0]), st.env_i32[i, 1:1 + C], st.env_i32[i, 1 + C:1 + 2 * C]
            twin = [j for j in range(C) if j != cur and hidden[j] == hidden[cur]][0]
            gone = [j for j in range(C) if shown[j] == removed]
            policy = i if i < 2 else 2 + (k % 3)
            if policy in (0, 2):
                a = twin
            elif policy in (1, 3) and gone:
                a = gone[0]
                seen["onto_removed"] += 1
            else:
                a = cur
            forced.append(a)
        actor.set_forced(forced)
        t_before = st.elapsed.copy()
        actor.step_all(1.0, store=False)
        st = actor.get_state()
        for i in range(N):
            obs, r, done, info = mirror.step(i, forced[i], st)
            check_step_against_host("mem", i, st, int(t_before[i]) + 1, obs, r, done, info, where=(k, forced))
            seen["completed"] += bool(info.get("is_success", False))
            seen["truncated"] += bool(info.get("TimeLimit.truncated", False))
            seen["miss"] += r == -1
            assert bool(st.last[i, 5]) == bool(info.get("is_success", False))
            if done:
                obs0 = mirror.begin(i, st)
                assert np.array_equal(f32_bits(st.stage_obs[i, 0]), f32_bits(obs0))
    assert all(v > 0 for v in seen.values()), seen
    # the card that has left the table but still "matches" (memory_cards.py:41-43): its twin is shown while it is marked as removed
    st = actor.get_state()
    for i in range(N):
        hidden = np.array([1, 2, 1, 2], dtype=np.int32)
        shown = np.array([removed, 0, 1, 0], dtype=np.int32)
        st.env_i32[i, 0], st.env_i32[i, 1:1 + C], st.env_i32[i, 1 + C:1 + 2 * C], st.elapsed[i] = 2, hidden, shown, 1
        env = mirror.envs[i]
        env._elapsed_steps, env.env.state, env.env.observation, env.env.current_card = 1, hidden.astype(np.int64), shown.astype(np.float64), 2
    actor.set_state(st)
    actor.set_forced([0] * N)
    actor.step_all(1.0, store=False)
    st = actor.get_state()
    for i in range(N):
        obs, r, done, info = mirror.step(i, 0, st)
        assert r == 0 and not done
        check_step_against_host("mem", i, st, 2, obs, r, done, info, where="removed card matches")
    actor.set_forced(None)


# ------------------------------------------------------------------------------------------ 3. replay parity
def replay_arrays(rb):
    d = rb.dev
    return {k: getattr(d, k).cpu().numpy().copy() for k in ("obs", "actions", "rewards", "dones", "ep_len")}


def check_replay_parity(lib, device, kind, steps=40):
    """`steps` forced-action vector steps with store = 1 against a second ReplayBuffer filled through store_obs / store / flush from
    host re-simulations of the same episodes, committed in the stated slot order (finished episodes of a vector step in environment
    order); then the same number of steps with store = 0 leaves the replay bitwise untouched."""
    from dtqn_amd.buffers.replay_buffer import ReplayBuffer
    agent = make_agent(lib, device, kind)
    actor = make_actor(agent, kind)
    rb = agent.replay_buffer
    cap = rb.max_episode_steps
    rb2 = ReplayBuffer(E * cap, agent.env_obs_length, agent.obs_mask, cap, context_len=L, device=agent.device, lib=agent.engine.lib)
    mirror = HostMirror(kind, N)
    st = actor.get_state()
    episodes = [[mirror.begin(i, st)] for i in range(N)]
    rng = np.random.default_rng(17)
    tally = dict(committed=0, env_steps=0, successes=0, finished=0, length_sum=0, return_sum=0.0)
    returns = [0.0] * N
    for k in range(steps):
        forced = rng.integers(0, agent.num_actions, size=N)
        if kind == "mem":                                         # half of the time the twin, so that episodes complete as well
            C = 2 * MEM_PAIRS
            for i in range(N):
                cur, hidden = int(st.env_i32[i, 0]), st.env_i32[i, 1:1 + C]
                if rng.random() < 0.5:
                    forced[i] = [j for j in range(C) if j != cur and hidden[j] == hidden[cur]][0]
        if kind == "car" and k == 30:
            # random pushes never reach a flag inside the cap: environment 1 is put next to one on both sides, so that a short episode
            # with a real end lands in a slot that held a longer one (a cleansed tail) after the ring has wrapped
            st.env_f64[1, :2] = (0.95, 0.06)
            actor.set_state(st)
            mirror.envs[1].env.state = np.array([0.95, 0.06, st.env_f64[1, 2]])
            forced[1] = 2
        actor.set_forced(forced)
        actor.step_all(1.0)
        st = actor.get_state()
        for i in range(N):
            obs, r, done, info = mirror.step(i, forced[i], st)
            stored = False if info.get("TimeLimit.truncated", False) else done
            episodes[i].append((np.array(obs, copy=True), int(forced[i]), float(r), bool(stored)))
            returns[i] += r
            tally["env_steps"] += 1
            if done:
                ep = episodes[i]
                rb2.store_obs(ep[0])
                for t, (o, a, rew, d) in enumerate(ep[1:]):
                    rb2.store(o, a, rew, d, t + 1)
                rb2.flush()
                tally["committed"] += 1
                tally["finished"] += 1
                tally["successes"] += int(bool(info.get("is_success", False)))
                tally["length_sum"] += len(ep) - 1
                tally["return_sum"] += returns[i]
                returns[i] = 0.0
                episodes[i] = [mirror.begin(i, st)]
    rb2.commit()
    got = actor.sync()
    assert {k: got[k] for k in tally} == tally, (got, tally)
    assert got["staged"] == got["committed"] and got["dropped"] == 0
    assert tally["committed"] > E, "the ring did not wrap"
    mine, ref = replay_arrays(rb), replay_arrays(rb2)
    for key in ref:
        assert mine[key].tobytes() == ref[key].tobytes(), key
    assert (ref["obs"] == rb.obs_mask).any() and ref["dones"].min() == 0 and (ref["ep_len"] < cap).any(), "no cleansed tail in the comparison"
    assert list(rb.pos) == list(rb2.pos) and np.array_equal(rb.episode_lengths, rb2.episode_lengths)
    # store = 0: nothing of the replay moves, episodes still finish and are counted
    version = rb.version
    for k in range(steps):
        actor.set_forced(rng.integers(0, agent.num_actions, size=N))
        actor.step_all(1.0, store=False)
    after = actor.sync()
    assert after["committed"] == tally["committed"] and after["finished"] > tally["finished"] and after["env_steps"] == 2 * steps * N
    again = replay_arrays(rb)
    for key in mine:
        assert again[key].tobytes() == mine[key].tobytes(), key
    assert rb.version == version and list(rb.pos) == list(rb2.pos)
    actor.set_forced(None)


# ------------------------------------------------------------------------------------------ 4. context and action parity
def host_q_rows(agent, contexts, n_max):
    """dtqn_actor_forward_batch on the block VectorActor would stage from `contexts`, with the given n_max -> [N][A]."""
    from dtqn_amd.agents.dtqn import _live_rows
    from dtqn_amd.agents.vector import actor_block
    eng, dev = agent.engine, agent.device
    n, A, Ln = len(contexts), agent.num_actions, agent.context_len
    pin = (lambda t: t.pin_memory()) if dev.type == "cuda" else (lambda t: t)
    total, ctx_h, obs_np, act_np, len_np = actor_block(n, Ln, int(agent.env_obs_length), lambda nb: pin(torch.zeros(nb, dtype=torch.uint8)))
    for i, ctx in enumerate(contexts):
        m = _live_rows(ctx)
        obs_np[i, :m], act_np[i, :m], len_np[i] = ctx.obs[:m], ctx.action[:m, 0], m
    ctx_d = torch.zeros(total, dtype=torch.uint8, device=dev)
    q_d = torch.zeros(n * Ln * A, device=dev)
    q_h = pin(torch.zeros(n, A))
    need = eng.lib.dtqn_forward_workspace_floats(eng._actor_net_ref, n)
    ws = torch.zeros(max(1, need), device=dev)
    rc = eng.lib.dtqn_actor_forward_batch(eng._actor_net_ref, agent._theta_p, ptr(ctx_h), ptr(ctx_d), n, n_max, ptr(q_d), ptr(q_h),
                                          ptr(ws) if need > 0 else None, 1, 0, 0, eng._stream())
    assert rc == 0
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return q_h.numpy().copy(), (obs_np, act_np, len_np)


def check_context_and_action_parity(lib, device, kind, shape, row_block, steps=16):
    """(Memory's cap of 6 is below the context of 8: its network gets a context of 4, so that its windows slide too.)"""
    from dtqn_amd.utils.context import Context
    agent = make_agent(lib, device, kind, context=L if kind == "car" else 4, **shape)
    L_ = agent.context_len
    assert bool(agent.engine.actor_net.tiled) == row_block
    actor = make_actor(agent, kind)
    mirror = HostMirror(kind, N)
    contexts = [Context(L_, agent.obs_mask, agent.num_actions, agent.env_obs_length, discrete=agent.is_discrete_env) for _ in range(N)]

    def begin(i, st):
        contexts[i].reset(mirror.begin(i, st))
        contexts[i].action[0, 0] = st.block.actions[i, 0]         # the padding action of row 0 is a draw of the device's

    st = actor.get_state()
    for i in range(N):
        begin(i, st)
    slid = boundaries = 0
    for k in range(steps):
        n_max = min(L_, k + 1)
        q_ref, (obs_ref, act_ref, len_ref) = host_q_rows(agent, contexts, n_max)
        for i in range(N):                                        # the resident block: what the host would have staged
            m = int(len_ref[i])
            assert st.block.lens[i] == m == min(L_, contexts[i].timestep + 1), (k, i)
            assert np.array_equal(f32_bits(st.block.obs[i, :m]), f32_bits(obs_ref[i, :m])), (k, i)
            assert np.array_equal(st.block.actions[i, :m], act_ref[i, :m]), (k, i, st.block.actions[i], act_ref[i])
            slid += contexts[i].timestep >= L_
        actor.step_all(0.0, store=False)
        q_dev = actor.q_rows()
        st = actor.get_state()
        assert np.isfinite(q_ref).all() and np.array_equal(f32_bits(q_dev), f32_bits(q_ref)), (k, q_dev, q_ref)
        actions = np.argmax(q_ref, axis=1)
        assert np.array_equal(st.last[:, 0], actions) and not st.last[:, 1].any(), (k, st.last[:, :2], actions)
        for i in range(N):
            obs, r, done, info = mirror.step(i, actions[i], st)
            stored = False if info.get("TimeLimit.truncated", False) else done
            contexts[i].add_transition(np.array(obs, copy=True), int(actions[i]), r, stored)
            if done:
                boundaries += 1
                begin(i, st)
    assert slid > 0 and boundaries > 0, (slid, boundaries)


# ------------------------------------------------------------------------------------------ 5. exploration
def _run_exploration(actor, epsilon, steps):
    actions, explored, resets = [], [], []
    for _ in range(steps):
        actor.step_all(epsilon, store=False)
        st = actor.get_state()
        actions.append(st.last[:, 0].copy())
        explored.append(st.last[:, 1].copy())
        for i in np.nonzero(st.last[:, 6])[0]:
            resets.append((float(st.env_f64[i, 0]), float(st.env_f64[i, 3])))
    return np.array(actions), np.array(explored), resets


def check_exploration(lib, device, n=64, steps=200, seed=2024):
    agent = make_agent(lib, device, "car")
    A = agent.num_actions
    a1, e1, resets = _run_exploration(make_actor(agent, "car", n=n, seed=seed), 1.0, steps)
    assert e1.all()                                               # epsilon = 1 always explores
    a2, e2, resets2 = _run_exploration(make_actor(agent, "car", n=n, seed=seed), 1.0, steps)
    assert np.array_equal(a1, a2) and resets == resets2           # a pure function of (seed, vector step, environment)
    a3, _, _ = _run_exploration(make_actor(agent, "car", n=n, seed=seed + 1), 1.0, 20)
    assert not np.array_equal(a1[:20], a3)
    total = n * steps
    assert total == 12_800
    p = 1.0 / A
    sigma = math.sqrt(p * (1 - p) / total)
    freq = np.bincount(a1.reshape(-1), minlength=A) / total
    print("action frequencies", freq, "5 sigma", 5 * sigma)
    assert (np.abs(freq - p) <= 5 * sigma).all(), freq
    # CarFlag resets: the side, and the start position on [-0.2, 0.2)
    starts, sides = np.array([r[0] for r in resets]), np.array([r[1] for r in resets])
    m = len(resets)
    assert m >= total // CAR_CAP - n
    share = float((sides > 0).mean())
    print("resets", m, "heaven right", share, "mean start", starts.mean())
    assert abs(share - 0.5) <= 5 * math.sqrt(0.25 / m)
    assert (starts >= -0.2).all() and (starts < 0.2).all()
    assert abs(starts.mean()) <= 5 * (0.4 / math.sqrt(12.0)) / math.sqrt(m)
    # epsilon = 0 never explores; at 0.3 the explored share
    _, e0, _ = _run_exploration(make_actor(agent, "car", n=n, seed=seed), 0.0, 5)
    assert not e0.any()
    _, e3, _ = _run_exploration(make_actor(agent, "car", n=n, seed=seed), 0.3, steps)
    share = float(e3.mean())
    print("explored share at 0.3:", share)
    assert abs(share - 0.3) <= 5 * math.sqrt(0.3 * 0.7 / total)


# ------------------------------------------------------------------------------------------ 7. end to end
def _patch_emu(lib, monkeypatch):
    from dtqn_amd.networks.dtqn import DTQN
    from dtqn_amd.utils import agent_utils
    if lib is not None:
        def emu_dtqn(*a, **k):
            m = DTQN(*a, _test_lib=lib, **k)
            m._allow_cpu = True
            return m
        monkeypatch.setitem(agent_utils.MODEL_MAP, "DTQN", emu_dtqn)


def check_run_py(lib, device, monkeypatch, tmp_path):
    import glob
    import pytest
    import run as runpy
    _patch_emu(lib, monkeypatch)
    monkeypatch.chdir(tmp_path)
    common = ("--envs DiscreteCarFlag-v0 --sampler device --in-embed 64 --context 8 --batch 2 --num-steps 24 --prepopulate 60 "
              "--max-episode-steps 12 --history 8 --heads 4 --layers 1 --buf-size 240 --eval-frequency 12 --eval-episodes 2 --disable-wandb "
              f"--device {device}")
    assert runpy.get_args(common.split()).device_envs == 0
    agent = runpy.run_experiment(runpy.get_args((common + " --device-envs 3 --project-name dev").split()))
    assert agent.num_train_steps == 24
    rb = agent.replay_buffer
    assert rb.pos[0] >= 3 and rb.pos[1] == 0                      # 20 prepopulation vector steps under a cap of 12: one episode per environment
    assert np.array_equal(rb.episode_lengths, rb.dev.ep_len.cpu().numpy())
    files = glob.glob(str(tmp_path / "policies" / "dev" / "**" / "*_results.csv"), recursive=True)
    assert len(files) == 1
    rows = open(files[0], newline="").read().splitlines()
    assert len(rows) == 3 and [r.split(",")[1] for r in rows[1:]] == ["0", "12"]
    for row in rows[1:]:
        assert all(np.isfinite(float(v)) for v in row.split(","))
    # refusals
    for extra, exc in ((" --device-envs 3 --num-envs 2", ValueError), (" --device-envs 3 --overlap", ValueError),
                       (" --device-envs 3 --sampler reference", ValueError), (" --device-envs -1", ValueError)):
        with pytest.raises(exc):
            runpy.run_experiment(runpy.get_args((common + extra + " --project-name refused").split()))


def check_checkpoint_round_trip(lib, device, tmp_path):
    """A checkpoint written after sync() restores the replay the device rollout wrote: arrays, position, episode lengths."""
    from dtqn_amd.utils.epsilon_anneal import LinearAnneal
    from dtqn_amd.utils.logging_utils import RunningAverage
    agent = make_agent(lib, device, "car")
    actor = make_actor(agent, "car")
    actor.prepopulate(60)
    for _ in range(4):
        actor.step_all(0.5, updates=N)
    assert agent.num_train_steps == 4 * N
    actor.sync()
    path = str(tmp_path / "ck")
    agent.save_checkpoint(path, None, RunningAverage(10), RunningAverage(10), RunningAverage(10), LinearAnneal(1.0, 0.1, 10))
    before, pos, lens = replay_arrays(agent.replay_buffer), list(agent.replay_buffer.pos), agent.replay_buffer.episode_lengths.copy()
    assert np.array_equal(lens, before["ep_len"]) and pos[0] == actor.pos0 + actor.counters()["committed"]
    other = make_agent(lib, device, "car", seed=12)
    other.load_checkpoint(path)
    after = replay_arrays(other.replay_buffer)
    for key in before:
        assert after[key].tobytes() == before[key].tobytes(), key
    assert list(other.replay_buffer.pos) == pos and np.array_equal(other.replay_buffer.episode_lengths, lens)
    assert other.num_train_steps == 4 * N
    # a rollout attached to the restored replay goes on in the next slot
    again = make_actor(other, "car")
    assert again.pos0 == pos[0]


def check_refusals(lib, device):
    import pytest
    from dtqn_amd.agents.device_rollout import DeviceVectorActor
    agent = make_agent(lib, device, "car")
    with pytest.raises(NotImplementedError):
        DeviceVectorActor(agent, "CartPole-v1", 3, 0)
    with pytest.raises(ValueError):
        DeviceVectorActor(agent, "DiscreteCarFlag-v0", 0, 0)
    with pytest.raises(ValueError):                               # the registry's cap of 200 does not fit this replay's 12 rows
        DeviceVectorActor(agent, "DiscreteCarFlag-v0", 3, 0)
    with pytest.raises(ValueError):
        make_actor(make_agent(lib, device, "car", sampler="reference"), "car")
    with pytest.raises(NotImplementedError):
        make_actor(make_agent(lib, device, "car", d_model=64, heads=8, bag_size=4), "car")
    image = make_agent(lib, device, "car")
    image.image = (1, 24, 24)
    with pytest.raises(NotImplementedError):
        make_actor(image, "car")
    dp = make_agent(lib, device, "car")
    dp.dp = object()
    with pytest.raises(NotImplementedError):
        make_actor(dp, "car")
    # the C entry points refuse a descriptor that does not fit the network
    actor = make_actor(agent, "car")
    lib_, net, rp = actor._lib_args()
    actor.ro.max_episode_steps = CAR_CAP + 1
    assert lib_.dtqn_rollout_reset(net, rp, actor._ro_ref, 0, agent.engine._stream()) != 0
    actor.ro.max_episode_steps = CAR_CAP
    actor.ro.env_kind = 1
    assert lib_.dtqn_rollout_step(net, agent._theta_p, rp, actor._ro_ref, 0, 0, 1, 1.0, 0, 0, 0, 0, 0, 0, agent.engine._stream()) != 0
