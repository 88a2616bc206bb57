"""Shared by test_emu_pomdp_env.py (HIP emulation on the CPU) and test_gpu_pomdp_env.py (MI355X): the tabular POMDP environment kind
(DTQN_ROLLOUT_POMDP) of the device-resident rollout and evaluation against the host `TabularPOMDP`, the host Context, the host
ReplayBuffer producer API and dtqn_actor_forward_batch.

Shapes, the smallest that can still go wrong: a hand-built model with S = 5, A = 3, Z = 4 (a zero inside a row, trailing zeros, a
deterministic row, a start distribution with zeros, two `reset` pairs -- (s3, a1) pays, (s4, a2) costs -- and rewards that depend on s'
and on z), N = 3 environments, a replay of E = 5 slots, context 8, step cap 12; networks: d_model 64 / 4 heads / 1 layer, and one
row-block network, d_model 128 with the GRU gate.

The host side never draws: the device records the uniforms it used in env_f64 ([0], [1] the step's, [2], [3] those of the reset that
started the episode in progress); they are read back with get_state and handed to the host environment, which is then compared bit
for bit.  The replay and context procedures are those of device_rollout_helpers.py (check_replay_parity,
check_context_and_action_parity), restated for this kind: those two build their agents and mirrors for CarFlag and Memory only."""
import atexit
import ctypes
import os
import tempfile

import numpy as np

from device_rollout_helpers import ROWBLOCK, WHOLE, _patch_emu, check_step_against_host, f32_bits, host_q_rows, replay_arrays
from device_rollout_helpers import make_agent as rollout_make_agent

__all__ = ["ROWBLOCK", "WHOLE"]

N, E, L, CAP = 3, 5, 8, 12
EPISODES = 7
POS_PAIR, NEG_PAIR = (3, 1), (4, 2)             # (state, action) of the two reset pairs

MODEL_TEXT = """\
# the test model: S = 5, A = 3, Z = 4
discount: 0.9
values: reward
states: s0 s1 s2 s3 s4
actions: a0 a1 a2
observations: z0 z1 z2 z3
start: 0.5 0.0 0.3 0.2 0.0
T: a0
0.5 0.0 0.5 0.0 0.0
0.0 1.0 0.0 0.0 0.0
0.2 0.2 0.2 0.2 0.2
0.0 0.0 0.0 0.25 0.75
0.1 0.2 0.3 0.4 0.0
T: a1
uniform
T: a2
identity
T: a1 : s3 reset
T: a2 : s4 reset
O: a0
0.7 0.0 0.3 0.0
0.0 0.0 1.0 0.0
0.25 0.25 0.25 0.25
0.0 0.5 0.5 0.0
0.1 0.2 0.3 0.4
O: a1
uniform
O: a2 : *
0.4 0.0 0.0 0.6
R: * : * : * : * -0.125
R: a0 : s0 : s2 : * 0.5
R: a0 : * : s3
0.25 -0.25 0.75 0.0
R: a1 : s0
0.0 0.1 0.2 0.3
1.0 1.1 1.2 1.3
2.0 2.1 2.2 2.3
3.0 3.1 3.2 3.3
4.0 4.1 4.2 4.3
R: a1 : s3 : * : * 2.0
R: a2 : s4 : * : * -3.0
"""

_dir = tempfile.TemporaryDirectory(prefix="pomdp_env_")
atexit.register(_dir.cleanup)
MODEL_PATH = os.path.join(_dir.name, "five.pomdp")
with open(MODEL_PATH, "w") as _f:
    _f.write(MODEL_TEXT)


def model():
    from dtqn_amd.envs.pomdp_file import load_pomdp
    return load_pomdp(MODEL_PATH)


def host_env(cap=CAP):
    from dtqn_amd import envs
    return envs.make(MODEL_PATH, max_episode_steps=cap)


def make_agent(lib, device, cap=CAP, **kw):
    """make_agent of device_rollout_helpers.py (its shapes and keywords) for the test model."""
    agent = rollout_make_agent(lib, device, host_env(cap), **kw)
    assert agent.env_obs_length == 1 and agent.obs_mask == 4 and agent.num_actions == 3 and agent.is_discrete_env
    return agent


def make_actor(agent, n=N, seed=5, cap=CAP):
    from dtqn_amd.agents.device_rollout import DeviceVectorActor
    return DeviceVectorActor(agent, MODEL_PATH, n, seed, max_episode_steps=cap)


def make_evaluator(agent, n=N, seed=5, cap=CAP, max_episodes=8):
    from dtqn_amd.agents.device_eval import DeviceEvaluator
    return DeviceEvaluator(agent, MODEL_PATH, n, seed, max_episode_steps=cap, max_episodes=max_episodes)


class RecordedUniforms:
    """np_random of a host TabularPOMDP that replays the device's recorded draws."""

    def __init__(self):
        self.next = []

    def random(self):
        return self.next.pop(0)          # (IndexError: the host wanted a draw the device did not make)


class HostMirror:
    """N host environments that replay what the device environments do, from the uniforms the device recorded.  begin(i, st):
    environment i starts the episode the device state `st` has just reset to; step(i, action, st_after) -> the host's step."""

    def __init__(self, n, cap=CAP):
        self.envs = [host_env(cap) for _ in range(n)]
        for e in self.envs:
            e.env.np_random = RecordedUniforms()

    def begin(self, i, st):
        env = self.envs[i]
        env.env.np_random.next = [float(st.env_f64[i, 2]), float(st.env_f64[i, 3])]
        obs = env.reset()
        assert not env.env.np_random.next
        assert env.env.state == st.env_i32[i, 0] and obs == st.env_i32[i, 1], (i, env.env.state, obs, st.env_i32[i, :2], st.env_f64[i])
        return obs

    def step(self, i, action, st_after):
        env = self.envs[i]
        env.env.np_random.next = [float(st_after.env_f64[i, 0]), float(st_after.env_f64[i, 1])]
        out = env.step(int(action))
        assert not env.env.np_random.next
        return out


# ------------------------------------------------------------------------------------------ 1. dynamics
def _steer(i, s, elapsed):
    """Environment 0 looks for the two terminals, environment 1 never ends (a0 is no reset pair: it runs into the cap), environment 2
    waits in s3 (a2 is the identity) and ends the episode on the cap's step."""
    if i == 1:
        return 0
    if i == 0:
        return 1 if s == 3 else (2 if s == 4 else 1)
    if s == 3:
        return 1 if elapsed == CAP - 1 else 2
    return 0 if s == 4 else 1


def check_dynamics(lib, device, steps=96):
    m = model()
    agent = make_agent(lib, device)
    actor = make_actor(agent)
    mirror = HostMirror(N)
    st = actor.get_state()
    for i in range(N):
        obs0 = mirror.begin(i, st)
        assert np.array_equal(f32_bits(st.stage_obs[i, 0]), f32_bits(obs0)) and np.array_equal(f32_bits(st.block.obs[i, 0]), f32_bits(obs0))
        assert m.start[st.env_i32[i, 0]] > 0
    seen = dict(positive_terminal=0, negative_terminal=0, truncated=0, real_end_on_the_cap=0, reward_by_obs=set())
    for k in range(steps):
        forced = [_steer(i, int(st.env_i32[i, 0]), int(st.elapsed[i])) for i in range(N)]
        before = st
        actor.set_forced(forced)
        actor.step_all(1.0, store=False)
        st = actor.get_state()
        for i in range(N):
            s, a, t = int(before.env_i32[i, 0]), forced[i], int(before.elapsed[i]) + 1
            obs, r, done, info = mirror.step(i, a, st)
            assert st.last[i, 0] == a and st.last[i, 1] == 0
            check_step_against_host("pomdp", i, st, t, obs, r, done, info, where=(k, forced))
            assert bool(st.last[i, 5]) == bool(info["is_success"])
            truncated = bool(info.get("TimeLimit.truncated", False))
            terminal = (s, a) in (POS_PAIR, NEG_PAIR)
            assert terminal == (bool(done) and not truncated)
            if terminal:
                assert (r > 0) == ((s, a) == POS_PAIR) and bool(info["is_success"]) == (r > 0)
                seen["positive_terminal" if r > 0 else "negative_terminal"] += 1
                seen["real_end_on_the_cap"] += t == CAP
            seen["truncated"] += truncated
            if (s, a) == (0, 1):
                seen["reward_by_obs"].add(r)
            if done:
                assert st.elapsed[i] == 0 and st.last[i, 6] == 1
                obs0 = mirror.begin(i, st)
                assert np.array_equal(f32_bits(st.stage_obs[i, 0]), f32_bits(obs0))
            else:
                assert st.env_i32[i, 0] == mirror.envs[i].env.state and st.env_i32[i, 1] == obs and st.elapsed[i] == t
                assert np.array_equal(st.env_f64[i, 2:].view(np.uint64), before.env_f64[i, 2:].view(np.uint64)), "a step moved the reset's record"
    assert all(seen[k] > 0 for k in ("positive_terminal", "negative_terminal", "truncated", "real_end_on_the_cap")), seen
    assert len(seen["reward_by_obs"]) > 2, seen
    actor.set_forced(None)


# ------------------------------------------------------------------------------------------ 2. draw statistics
def _run_draws(agent, n, steps, seed, action):
    """`steps` vector steps of `action` -> (state before, state after, observation after) of every environment step that did not end
    its episode (the state after the last step of an episode is the next episode's first)."""
    actor = make_actor(agent, n=n, seed=seed)
    actor.set_forced([action] * n)
    st = actor.get_state()
    out = []
    for _ in range(steps):
        before = st
        actor.step_all(1.0, store=False)
        st = actor.get_state()
        live = st.last[:, 2] == 0
        out.append(np.stack([before.env_i32[live, 0], st.env_i32[live, 0], st.env_i32[live, 1]], axis=1))
    return np.concatenate(out)


def check_draw_statistics(lib, device, n=64, steps=200, seed=2024):
    """Action a0 throughout (no reset pair: episodes end at the cap only).  The next-state frequencies of the row (s0, a0) -- a zero
    inside, trailing zeros -- and the observation frequencies of the row (a0, s' = s3) -- zeros at both ends -- against the tables."""
    m = model()
    agent = make_agent(lib, device)
    draws = _run_draws(agent, n, steps, seed, 0)
    assert n * steps == 12_800 and len(draws) >= n * steps * (CAP - 1) // CAP - n
    rows = draws[draws[:, 0] == 0]
    p_row = m.T[0, 0]
    freq = np.bincount(rows[:, 1], minlength=len(p_row)) / len(rows)
    sigma = np.sqrt(p_row * (1 - p_row) / len(rows))
    print("next state of (s0, a0)", "n", len(rows), "frequencies", freq, "table", p_row, "5 sigma", 5 * sigma)
    assert len(rows) > 500 and (np.abs(freq - p_row) <= 5 * sigma).all(), (freq, p_row)
    assert (freq[p_row == 0] == 0).all()
    rows = draws[draws[:, 1] == 3]
    p_row = m.O[0, 3]
    freq = np.bincount(rows[:, 2], minlength=len(p_row)) / len(rows)
    sigma = np.sqrt(p_row * (1 - p_row) / len(rows))
    print("observation of (a0, s3)", "n", len(rows), "frequencies", freq, "table", p_row, "5 sigma", 5 * sigma)
    assert len(rows) > 500 and (np.abs(freq - p_row) <= 5 * sigma).all(), (freq, p_row)
    assert (freq[p_row == 0] == 0).all()
    # no zero-probability transition or observation anywhere in the run
    assert (m.T[0][draws[:, 0], draws[:, 1]] > 0).all() and (m.O[0][draws[:, 1], draws[:, 2]] > 0).all()
    again = _run_draws(agent, n, 20, seed, 0)
    assert np.array_equal(again, draws[:len(again)]), "the same seed gave another run"
    other = _run_draws(agent, n, 20, seed + 1, 0)
    assert not np.array_equal(other, again)


# ------------------------------------------------------------------------------------------ 3. replay parity
def check_replay_parity(lib, device, shape, row_block, steps=40):
    """check_replay_parity of device_rollout_helpers.py for this kind: `steps` forced-action vector steps with store = 1 against a
    second ReplayBuffer filled through store_obs / store / flush from host re-simulations of the same episodes, committed in the stated
    slot order; then the same number of steps with store = 0 leaves the replay bitwise untouched."""
    from dtqn_amd.buffers.replay_buffer import ReplayBuffer
    agent = make_agent(lib, device, **shape)
    assert bool(agent.engine.actor_net.tiled) == row_block
    actor = make_actor(agent)
    rb = agent.replay_buffer
    cap = rb.max_episode_steps
    rb2 = ReplayBuffer(E * cap, agent.env_obs_length, agent.obs_mask, cap, context_len=L, device=agent.device, lib=agent.engine.lib)
    mirror = HostMirror(N)
    st = actor.get_state()
    episodes = [[mirror.begin(i, st)] for i in range(N)]
    rng = np.random.default_rng(17)
    tally = dict(committed=0, env_steps=0, successes=0, finished=0, length_sum=0, return_sum=0.0)
    returns = [0.0] * N
    for k in range(steps):
        forced = rng.integers(0, agent.num_actions, size=N)
        forced[1] = 0                                             # environment 1 never ends before the cap: full-length episodes too
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
def check_context_and_action_parity(lib, device, shape, row_block, steps=30):
    """check_context_and_action_parity of device_rollout_helpers.py for this kind, context 8 under a cap of 12: the resident context
    blocks and the Q rows bit-equal to dtqn_actor_forward_batch on host-staged contexts, the actions their arg-max."""
    from dtqn_amd.utils.context import Context
    agent = make_agent(lib, device, **shape)
    L_ = agent.context_len
    assert L_ == L and bool(agent.engine.actor_net.tiled) == row_block
    actor = make_actor(agent)
    mirror = HostMirror(N)
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


# ------------------------------------------------------------------------------------------ 5. device evaluation
def check_eval_independent_of_n(lib, device):
    """The results table of a 7-episode quota played by N = 1 equals the one played by N = 3, row for row: return, length, success
    (the other two columns say which environment played the episode and in which vector step it finished)."""
    agent = make_agent(lib, device)
    tables = []
    for n in (1, 3):
        ev = make_evaluator(agent, n=n)
        triple = ev.evaluate(EPISODES, key=9)
        res = ev.results()
        assert len(res.returns) == EPISODES and np.array_equal(res.envs, np.arange(EPISODES) % n)
        assert ((res.lengths >= 1) & (res.lengths <= CAP)).all() and all(np.isfinite(v) for v in triple)
        tables.append((res.returns.tobytes(), res.lengths.tobytes(), res.successes.tobytes(), triple))
        print("N", n, "returns", res.returns, "lengths", res.lengths, "successes", res.successes)
    assert tables[0] == tables[1]


def check_eval_step_parity(lib, device):
    """One evaluation stepped with get_state against the host environment, from the recorded uniforms."""
    agent = make_agent(lib, device)
    ev = make_evaluator(agent)
    mirror = HostMirror(N)
    episode, returns, host_rows = [-1] * N, [0.0] * N, {}
    ev.begin(EPISODES, key=3)
    st = ev.get_state()
    for i in range(N):
        assert st.episode[i] == i and st.block.lens[i] == 1
        obs0 = mirror.begin(i, st)
        assert np.array_equal(f32_bits(st.block.obs[i, 0]), f32_bits(obs0))
        episode[i] = i
    k = env_steps = 0
    seen = dict(done=0, idle=0)
    while any(e >= 0 for e in episode):
        assert k < 3 * CAP
        before = st
        ev.step()
        q = ev.q_rows()
        st = ev.get_state()
        for i in range(N):
            if episode[i] < 0:
                seen["idle"] += 1
                assert st.last[i, 0] == -1 and st.episode[i] == -1 and np.array_equal(st.env_i32[i], before.env_i32[i])
                continue
            a = int(st.last[i, 0])
            assert a == int(np.argmax(q[i])) and st.last[i, 6] == episode[i]
            obs, r, done, info = mirror.step(i, a, st)
            truncated = bool(info.get("TimeLimit.truncated", False))
            assert np.array_equal(f32_bits(st.obs_new[i]), f32_bits(obs)) and f32_bits(st.reward[i]) == f32_bits(r), (k, i)
            assert (bool(st.last[i, 2]), bool(st.last[i, 3]), bool(st.last[i, 4])) == (bool(done), bool(done) and not truncated, truncated), (k, i)
            assert bool(st.last[i, 5]) == bool(info["is_success"])
            returns[i] += r
            env_steps += 1
            if not done:
                assert st.env_i32[i, 0] == mirror.envs[i].env.state and st.env_i32[i, 1] == obs
                assert st.elapsed[i] == mirror.envs[i]._elapsed_steps and st.ep_ret[i] == returns[i]
                continue
            seen["done"] += 1
            e = episode[i]
            host_rows[e] = (float(returns[i]), mirror.envs[i]._elapsed_steps, int(bool(info["is_success"]) or returns[i] > 0))
            row = st.results[e]
            assert (float(row["ret"]), int(row["length"]), int(row["success"]), int(row["env"]), int(row["vstep"])) == host_rows[e] + (i, k), (e, row)
            returns[i] = 0.0
            if e + N < EPISODES:
                episode[i] = e + N
                assert st.episode[i] == e + N
                mirror.begin(i, st)
            else:
                episode[i] = -1
                assert st.episode[i] == -1 and st.block.lens[i] == 1
        k += 1
    assert sorted(host_rows) == list(range(EPISODES)) and all(v > 0 for v in seen.values()), (host_rows, seen)
    got = ev.poll()
    assert got["finished"] == EPISODES and got["live"] == 0 and got["env_steps"] == env_steps, got


# ------------------------------------------------------------------------------------------ 6. run.py
def _results_rows(tmp_path, name):
    import glob
    files = glob.glob(str(tmp_path / "policies" / name / "**" / "*_results.csv"), recursive=True)
    assert len(files) == 1, files
    rows = open(files[0], newline="").read().splitlines()
    assert len(rows) == 3 and [r.split(",")[1] for r in rows[1:]] == ["0", "12"], rows
    for row in rows[1:]:
        assert all(np.isfinite(float(v)) for v in row.split(","))


def check_run_py(lib, device, monkeypatch, tmp_path):
    import pytest
    import run as runpy
    _patch_emu(lib, monkeypatch)
    monkeypatch.chdir(tmp_path)
    shape = ("--sampler device --in-embed 64 --context 8 --batch 2 --num-steps 24 --prepopulate 60 --history 8 --heads 4 --layers 1 "
             f"--buf-size 240 --eval-frequency 12 --eval-episodes 2 --disable-wandb --device {device}")
    tiger = "--envs POMDP-tiger-episodic-v0 --max-episode-steps 12 " + shape
    agent = runpy.run_experiment(runpy.get_args((tiger + " --device-envs 3 --device-eval-envs 2 --project-name dev").split()))
    assert agent.num_train_steps == 24 and agent.env_obs_length == 1 and agent.num_actions == 3 and agent.obs_mask == 2
    rb = agent.replay_buffer
    assert rb.pos[0] >= 3 and rb.pos[1] == 0
    assert np.array_equal(rb.episode_lengths, rb.dev.ep_len.cpu().numpy()) and rb.episode_lengths.max() <= 12
    _results_rows(tmp_path, "dev")
    # the same domain on the host path
    agent = runpy.run_experiment(runpy.get_args((tiger + " --num-envs 2 --eval-envs 2 --project-name host").split()))
    assert agent.num_train_steps == 24
    _results_rows(tmp_path, "host")
    # ... and through the single-environment actor, prepopulation and run.evaluate included
    agent = runpy.run_experiment(runpy.get_args((tiger + " --project-name single").split()))
    assert agent.num_train_steps == 24
    _results_rows(tmp_path, "single")
    # a .pomdp path: runs with a step cap, refused with a clear message without one
    path = "--envs " + MODEL_PATH + " " + shape
    agent = runpy.run_experiment(runpy.get_args((path + " --max-episode-steps 12 --device-envs 3 --device-eval-envs 2 --project-name path").split()))
    assert agent.num_train_steps == 24 and agent.num_actions == 3 and agent.obs_mask == 4
    _results_rows(tmp_path, "path")
    with pytest.raises(ValueError, match="--max-episode-steps"):
        runpy.run_experiment(runpy.get_args((path + " --device-envs 3 --project-name refused").split()))


# ------------------------------------------------------------------------------------------ 7. refusals
def check_refusals(lib, device):
    import pytest
    from dtqn_amd import _binding as B
    from dtqn_amd.agents.device_eval import DeviceEvaluator
    from dtqn_amd.agents.device_rollout import DeviceVectorActor
    agent = make_agent(lib, device)
    for cls in (DeviceVectorActor, DeviceEvaluator):
        with pytest.raises(NotImplementedError):
            cls(agent, "CartPole-v1", 3, 0)
        with pytest.raises(ValueError, match="max-episode-steps"):    # a path has no cap of its own
            cls(agent, MODEL_PATH, 3, 0)
    for make in (make_actor, make_evaluator):
        with pytest.raises(NotImplementedError):
            make(make_agent(lib, device, d_model=64, heads=8, bag_size=4))
        image = make_agent(lib, device)
        image.image = (1, 24, 24)
        with pytest.raises(NotImplementedError):
            make(image)
        dp = make_agent(lib, device)
        dp.dp = object()
        with pytest.raises(NotImplementedError):
            make(dp)
    # the C entry points: the descriptor's table fields against the network
    ERR_ARG = B.DEFINES["DTQN_ERR_ARG"]
    actor, ev = make_actor(agent), make_evaluator(agent)
    lib_, net, rp = actor._lib_args()
    stream, theta = agent.engine._stream(), agent._theta_p
    calls = [
        (actor.ro, lambda n=net: lib_.dtqn_rollout_reset(n, rp, actor._ro_ref, 0, stream)),
        (actor.ro, lambda n=net: lib_.dtqn_rollout_step(n, theta, rp, actor._ro_ref, 0, 0, 1, 1.0, 0, 0, 0, 0, 0, 0, stream)),
        (ev.ev, lambda n=net: lib_.dtqn_deval_begin(n, ev._ev_ref, 1, 2, stream)),
        (ev.ev, lambda n=net: lib_.dtqn_deval_step(n, theta, ev._ev_ref, 1, 0, 0, 1, 2, stream)),
    ]
    for desc, call in calls:
        assert desc.env_kind == B.DEFINES["DTQN_ROLLOUT_POMDP"] == 2
        for field, value in (("pomdp_actions", 4), ("pomdp_actions", 2), ("pomdp_tables", None), ("pomdp_states", 0), ("pomdp_obs", 0),
                             ("pomdp_first_obs_action", 3), ("pomdp_first_obs_action", -1)):
            keep = getattr(desc, field)
            setattr(desc, field, value)
            assert call() == ERR_ARG, (field, value)
            setattr(desc, field, keep)
        wide = B.DtqnNet.from_buffer_copy(agent.engine.actor_net)     # obs_dim != 1: no tabular POMDP observation
        wide.obs_dim = 2
        assert call(ctypes.byref(wide)) == ERR_ARG
        more = B.DtqnNet.from_buffer_copy(agent.engine.actor_net)     # a network with another action count than the tables
        more.num_actions = 4
        assert call(ctypes.byref(more)) == ERR_ARG
    actor.reset_all()
    ev.begin(2, key=1)
    if agent.device.type == "cuda":
        agent._main_stream.synchronize()
    actor.get_state()
    ev.get_state()
