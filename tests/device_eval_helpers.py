"""Shared by test_emu_device_eval.py (HIP emulation on the CPU) and test_gpu_device_eval.py (MI355X): the device-resident greedy
evaluation (csrc/dtqn_deval.hip, dtqn_amd.agents.device_eval.DeviceEvaluator) against the host environments, the host Context,
dtqn_actor_forward_batch and run.evaluate's formulas.

Shapes, those of device_rollout_helpers.py: N = 3 environments, context 8, CarFlag with a step cap of 12, Memory with 2 pairs, a cap of
6 and a context of 4; 7 episodes, so that the environments go idle at different times (environment 0 plays three, the others two).

The host side never draws: where the device drew (a reset, Memory's next card) the host is given that draw, read back with get_state."""
import ctypes

import numpy as np

from device_rollout_helpers import (CAR_CAP, ENV_ID, L, MEM_CAP, MEM_PAIRS, N, ROWBLOCK, WHOLE, HostMirror, f32_bits, host_env, host_q_rows,
                                    make_agent, replay_arrays)

EPISODES = 7
__all__ = ["ROWBLOCK", "WHOLE"]


def make_evaluator(agent, kind, n=N, seed=5, cap=None, max_episodes=8):
    from dtqn_amd.agents.device_eval import DeviceEvaluator
    return DeviceEvaluator(agent, ENV_ID[kind], n, seed, max_episode_steps=cap if cap is not None else (CAR_CAP if kind == "car" else MEM_CAP),
                           num_pairs=MEM_PAIRS if kind == "mem" else None, max_episodes=max_episodes)


def make_agent_dropout(lib, device, kind, dropout, seed=11, q_scale=100.0):
    """make_agent of device_rollout_helpers.py (WHOLE shape) with a dropout probability: that helper builds dropout-0 networks only."""
    from dtqn_amd.networks.dtqn import DTQN
    from dtqn_amd.utils import agent_utils
    from dtqn_amd.utils.random import set_global_seed
    env = host_env(kind)
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
        agent = agent_utils.get_agent("DTQN", [env], 8, 0, 64, 5 * cap, device, 3e-4, 2, L, cap, L, 1000, 0.99, 4, 1, dropout, False, "res",
                                      "learned", 0, sampler="device", sample_seed=seed)
    finally:
        agent_utils.MODEL_MAP["DTQN"] = orig
    sd = {k: v.clone() for k, v in agent.policy_network.state_dict().items()}
    sd["ffn.2.weight"] = sd["ffn.2.weight"] * q_scale
    agent.policy_network.load_state_dict(sd)
    agent.target_update()
    return agent


class _NewestObs:
    """HostMirror.step reads the observation a truncated Memory step stored as stage_obs[i, t]: here it is the newest-observation row."""

    def __init__(self, obs_new):
        self.obs_new = obs_new

    def __getitem__(self, key):
        return self.obs_new[key[0]]


def _for_mirror(st):
    st.stage_obs = _NewestObs(st.obs_new)
    return st


def run_formulas(returns, lengths, successes):
    """run.evaluate's accumulation (run.py evaluate) over per-episode records in episode order."""
    n = max(len(returns), 1)
    ret = ok = steps = 0
    for r, length, s in zip(returns, lengths, successes):
        ret += r
        steps += length
        ok += s
    return ok / n, ret / n, steps / n


# ------------------------------------------------------------------------------------------ 1. step-by-step parity
def check_step_parity(lib, device, kind, shape, row_block):
    """The evaluator one vector step at a time against N host environments and N host contexts.  (Memory's cap of 6 is below the context
    of 8: its network gets a context of 4, so that its windows slide too.)  The natural terminal step is staged through set_state -- a
    greedy car does not reach a flag in 12 steps, nor a fresh network the last pair in 6: before vector step 2 environment 1 is put
    where the action the host has already computed for it ends the episode."""
    from dtqn_amd.utils.context import Context
    agent = make_agent(lib, device, kind, context=L if kind == "car" else 4, **shape)
    L_ = agent.context_len
    cap = CAR_CAP if kind == "car" else MEM_CAP
    assert bool(agent.engine.actor_net.tiled) == row_block
    ev = make_evaluator(agent, kind)
    mirror = HostMirror(kind, N)
    mk = lambda: Context(L_, agent.obs_mask, agent.num_actions, agent.env_obs_length, discrete=agent.is_discrete_env)
    contexts = [mk() for _ in range(N)]
    episode = [-1] * N
    returns = [0.0] * N
    host_rows = {}

    def begin(i, e, st):
        assert st.episode[i] == e and st.elapsed[i] == 0 and st.ep_ret[i] == 0.0 and st.block.lens[i] == 1, (i, e, st.episode, st.block.lens)
        contexts[i].reset(mirror.begin(i, st))
        contexts[i].action[0, 0] = st.block.actions[i, 0]         # the padding action of row 0 is a draw of the device's
        episode[i], returns[i] = e, 0.0

    key = ev.begin(EPISODES, key=3)
    assert key == 3
    st = ev.get_state()
    assert not st.counters[:5].any() and st.counters[5] == N
    for i in range(N):
        begin(i, i, st)
    seen = dict(slid=0, truncated=0, terminal=0, idle=0)
    env_steps, k = 0, 0
    while any(e >= 0 for e in episode):
        assert k < 3 * cap, "more vector steps than ceil(7 / 3) episodes of `cap` steps"
        n_max = ev.next_n_max()
        assert n_max >= min(L_, k + 1)
        staged = []
        for i in range(N):
            if episode[i] >= 0:
                staged.append(contexts[i])
            else:                                                 # idle: what the device carries -- one row
                c = mk()
                c.reset(st.block.obs[i, 0].astype(np.float64))
                c.action[0, 0] = st.block.actions[i, 0]
                staged.append(c)
        q_ref, (obs_ref, act_ref, len_ref) = host_q_rows(agent, staged, n_max)
        for i in range(N):                                        # the resident block: what the host would have staged
            m = int(len_ref[i])
            if episode[i] < 0:
                seen["idle"] += 1
                assert st.block.lens[i] == 1 and st.episode[i] == -1 and np.isfinite(st.block.obs[i, 0]).all(), (k, i)
                continue
            assert st.block.lens[i] == m == min(L_, contexts[i].timestep + 1), (k, i, st.block.lens)
            assert np.array_equal(f32_bits(st.block.obs[i, :m]), f32_bits(obs_ref[i, :m])), (k, i)
            assert np.array_equal(st.block.actions[i, :m], act_ref[i, :m]), (k, i, st.block.actions[i], act_ref[i])
            seen["slid"] += contexts[i].timestep >= L_
        actions = np.argmax(q_ref, axis=1)
        if k == 2 and episode[1] >= 0:                            # the staged terminal step
            a = int(actions[1])
            if kind == "car":
                st.env_f64[1, :2] = (0.95, 0.06)
                mirror.envs[1].env.state = np.array([0.95, 0.06, st.env_f64[1, 2]])
            else:                                                 # every card but the shown one has left the table, and every card matches it
                C, removed = 2 * MEM_PAIRS, MEM_PAIRS + 1
                cur = 0 if a != 0 else 1
                hidden = np.ones(C, dtype=np.int32)
                shown = np.full(C, removed, dtype=np.int32)
                shown[cur] = 1
                st.env_i32[1, 0], st.env_i32[1, 1:1 + C], st.env_i32[1, 1 + C:1 + 2 * C] = cur, hidden, shown
                inner = mirror.envs[1].env
                inner.state, inner.observation, inner.current_card = hidden.astype(np.int64), shown.astype(np.float64), cur
            ev.set_state(st)
        before = st
        ev.step()
        q_dev = ev.q_rows()
        st = _for_mirror(ev.get_state())
        assert np.isfinite(q_ref).all() and np.array_equal(f32_bits(q_dev), f32_bits(q_ref)), (k, q_dev, q_ref)
        for i in range(N):
            if episode[i] < 0:                                    # idle: no step, len 1, never counted
                assert st.last[i, 0] == -1 and st.last[i, 6] == -1 and not st.last[i, 1:6].any(), (k, i, st.last[i])
                assert st.episode[i] == -1 and st.elapsed[i] == 0 and st.block.lens[i] == 1, (k, i)
                assert np.array_equal(st.env_f64[i], before.env_f64[i]) and np.array_equal(st.env_i32[i], before.env_i32[i]), (k, i)
                continue
            assert st.last[i, 0] == actions[i] and st.last[i, 6] == episode[i], (k, i, st.last[i], actions)
            obs, r, done, info = mirror.step(i, actions[i], st)
            truncated = bool(info.get("TimeLimit.truncated", False))
            stored = False if truncated else bool(done)
            assert np.array_equal(f32_bits(st.obs_new[i]), f32_bits(obs)), (k, i, st.obs_new[i], obs)
            assert f32_bits(st.reward[i]) == f32_bits(r), (k, i, st.reward[i], r)
            assert (bool(st.last[i, 2]), bool(st.last[i, 3]), bool(st.last[i, 4])) == (bool(done), stored, truncated), (k, i, st.last[i], info)
            contexts[i].add_transition(np.array(obs, copy=True), int(actions[i]), r, stored)
            returns[i] += r
            env_steps += 1
            if not done:
                assert st.elapsed[i] == contexts[i].timestep and st.ep_ret[i] == returns[i] and st.episode[i] == episode[i], (k, i)
                continue
            seen["truncated"] += truncated
            seen["terminal"] += not truncated
            e = episode[i]
            host_rows[e] = (float(returns[i]), contexts[i].timestep, int(bool(info.get("is_success", False)) or returns[i] > 0))
            row = st.results[e]
            assert (float(row["ret"]), int(row["length"]), int(row["success"]), int(row["env"]), int(row["vstep"])) == host_rows[e] + (i, k), (e, row)
            if e + N < EPISODES:
                begin(i, e + N, st)
            else:
                episode[i] = -1
                assert st.episode[i] == -1 and st.block.lens[i] == 1, (k, i)
        c = st.counters
        assert c[0] == len(host_rows) and c[1] == env_steps and c[5] == sum(e >= 0 for e in episode) and c[6] == k + 1, (k, c)
        assert c[2] == sum(r[2] for r in host_rows.values()) and c[3] == sum(r[1] for r in host_rows.values()), (k, c)
        k += 1
    assert sorted(host_rows) == list(range(EPISODES))
    assert all(v > 0 for v in seen.values()), seen
    got = ev.poll()
    assert got["finished"] == EPISODES and got["live"] == 0 and got["env_steps"] == env_steps, got
    # steps past the end (the host runs ahead of the status record): nothing is counted, nobody wakes up
    ev.step()
    ev.step()
    st = ev.get_state()
    assert st.counters[0] == EPISODES and st.counters[1] == env_steps and (st.episode == -1).all() and (st.block.lens == 1).all()


# ------------------------------------------------------------------------------------------ 2. episodes do not depend on N
def _start_states(ev, kind, episodes, key):
    """Episode index -> (environment state, padding action) as the episode begins; the environments that were idle from the start."""
    C = 2 * MEM_PAIRS
    state = (lambda st, i: st.env_f64[i].copy()) if kind == "car" else (lambda st, i: st.env_i32[i, :1 + 2 * C].copy())
    ev.begin(episodes, key=key)
    st = ev.get_state()
    starts = {int(st.episode[i]): (state(st, i), int(st.block.actions[i, 0])) for i in range(ev.n) if st.episode[i] >= 0}
    idle = [i for i in range(ev.n) if st.episode[i] < 0]
    for i in idle:
        assert st.block.lens[i] == 1
    bound = -(-episodes // ev.n) * ev.cap
    for _ in range(bound):
        ev.step()
        st = ev.get_state()
        for i in range(ev.n):
            if st.last[i, 2] and st.episode[i] >= 0:
                assert int(st.episode[i]) not in starts
                starts[int(st.episode[i])] = (state(st, i), int(st.block.actions[i, 0]))
        if st.counters[0] == episodes:
            break
    assert st.counters[0] == episodes and sorted(starts) == list(range(episodes)), (st.counters, sorted(starts))
    return starts, idle


def check_independent_of_n(lib, device, kind):
    """(A cap of 3 keeps the N = 1 run short: the start of an episode does not depend on how long the one before it lasted.)"""
    agent = make_agent(lib, device, kind, context=L if kind == "car" else 4)
    ref = None
    for n in (1, 3, 8):
        ev = make_evaluator(agent, kind, n=n, cap=3)
        starts, idle = _start_states(ev, kind, EPISODES, key=9)
        assert idle == ([7] if n == 8 else []), (n, idle)
        if ref is None:
            ref = starts
        for e in range(EPISODES):
            assert starts[e][0].tobytes() == ref[e][0].tobytes() and starts[e][1] == ref[e][1], (n, e, starts[e], ref[e])
    other, _ = _start_states(ev, kind, EPISODES, key=10)
    assert any(other[e][0].tobytes() != ref[e][0].tobytes() for e in range(EPISODES))
    again, _ = _start_states(ev, kind, EPISODES, key=9)             # a given key replays its episodes
    assert all(again[e][0].tobytes() == ref[e][0].tobytes() for e in range(EPISODES))
    ev.evaluate(2)
    first = ev.key
    ev.evaluate(2)
    assert ev.key != first and first > 10                        # keys never repeat, explicit ones included


# ------------------------------------------------------------------------------------------ 3. quota
def check_quota(lib, device, kind):
    import pytest
    agent = make_agent(lib, device, kind, context=L if kind == "car" else 4)
    ev = make_evaluator(agent, kind)
    cap = ev.cap
    for episodes in (EPISODES, 2, 3, 0):
        triple = ev.evaluate(episodes)
        res = ev.results()
        assert len(res.returns) == len(res.lengths) == len(res.successes) == episodes
        if episodes == 0:
            assert triple == (0.0, 0.0, 0.0)
            continue
        got = ev.poll()
        assert got["finished"] == episodes and got["live"] == 0, got
        assert got["env_steps"] == int(res.lengths.sum()) == got["length_sum"] and got["successes"] == int(res.successes.sum()), (got, res)
        assert triple == run_formulas(res.returns.tolist(), res.lengths.tolist(), res.successes.tolist()), triple
        assert ((res.lengths >= 1) & (res.lengths <= cap)).all() and np.array_equal(res.envs, np.arange(episodes) % N), res
        if kind == "car":                                         # the only reward is the flag's
            assert np.array_equal(res.successes, (res.returns > 0).astype(np.int32)), res
        assert all(np.isfinite(v) for v in triple)
    with pytest.raises(ValueError):
        ev.evaluate(ev.max_episodes + 1)
    with pytest.raises(ValueError):
        ev.evaluate(-1)


# ------------------------------------------------------------------------------------------ 4. nothing else moves
def _agent_snapshot(agent):
    from dtqn_amd.utils.random import RNG
    rb = agent.replay_buffer
    ctx = [(c.obs.copy(), c.action.copy(), c.reward.copy(), c.done.copy(), c.timestep) for c in (agent.train_context, agent.eval_context)]
    return dict(rng=repr(RNG.rng.bit_generator.state), ctx=ctx, mode=agent.train_mode, replay=replay_arrays(rb), version=rb.version,
                pos=list(rb.pos), theta=agent.engine.theta_pol.cpu().numpy().copy(), drop=agent._actor_calls,
                training=agent.policy_network.training)


def _assert_same(a, b):
    assert a["rng"] == b["rng"] and a["mode"] == b["mode"] and a["version"] == b["version"] and a["pos"] == b["pos"] and a["drop"] == b["drop"]
    assert a["training"] == b["training"] and a["theta"].tobytes() == b["theta"].tobytes()
    for x, y in zip(a["ctx"], b["ctx"]):
        assert all(np.array_equal(p, q) for p, q in zip(x[:4], y[:4])) and x[4] == y[4]
    for key in a["replay"]:
        assert a["replay"][key].tobytes() == b["replay"][key].tobytes(), key


def check_nothing_else_moves(lib, device, steps=24):
    from dtqn_amd.agents.device_rollout import DeviceVectorActor
    agent = make_agent(lib, device, "car")
    agent.eval_on()
    agent.context_reset(np.array([0.1, 0.0, 0.0]))
    agent.eval_off()
    agent.context_reset(np.array([-0.1, 0.0, 0.0]))
    ev = make_evaluator(agent, "car")
    before = _agent_snapshot(agent)
    ev.evaluate(EPISODES)
    ev.evaluate(2, key=1)
    _assert_same(before, _agent_snapshot(agent))
    # a device rollout on the same agent, parameters frozen: the same replay bytes with evaluations between its steps and without
    out = []
    for interleave in (False, True):
        ag = make_agent(lib, device, "car")
        actor = DeviceVectorActor(ag, ENV_ID["car"], N, 5, max_episode_steps=CAR_CAP)
        ev2 = make_evaluator(ag, "car")
        for k in range(steps):
            actor.step_all(0.3)
            if interleave and k % 5 == 2:
                ev2.evaluate(3)
        got = actor.sync()
        assert got["committed"] >= 3
        out.append((replay_arrays(ag.replay_buffer), got, list(ag.replay_buffer.pos), ag._actor_calls))
    (ra, ga, pa, da), (rb_, gb, pb, db) = out                     # (rb.version counts the commits the host saw: timing, not content)
    assert ga == gb and pa == pb and da == db
    for key in ra:
        assert ra[key].tobytes() == rb_[key].tobytes(), key


# ------------------------------------------------------------------------------------------ 5. dropout
def check_dropout_is_off(lib, device):
    plain, drop = make_agent_dropout(lib, device, "car", 0.0), make_agent_dropout(lib, device, "car", 0.1)
    assert drop.policy_network.dropout_p == 0.1 and plain.policy_network.dropout_p == 0.0
    drop.policy_network.load_state_dict({k: v.clone() for k, v in plain.policy_network.state_dict().items()})
    assert drop.engine.theta_pol.cpu().numpy().tobytes() == plain.engine.theta_pol.cpu().numpy().tobytes()
    assert drop.train_mode.name == "TRAIN"
    out = []
    for agent in (plain, drop):
        ev = make_evaluator(agent, "car")
        triple = ev.evaluate(EPISODES, key=4)
        st = ev.get_state()
        out.append((triple, st.results.tobytes(), ev.q_rows().tobytes()))
    assert out[0] == out[1]


# ------------------------------------------------------------------------------------------ 6. run.py
def check_run_py(lib, device, monkeypatch, tmp_path):
    import glob
    import pytest
    import run as runpy
    from device_rollout_helpers import _patch_emu
    _patch_emu(lib, monkeypatch)
    monkeypatch.chdir(tmp_path)
    common = ("--envs DiscreteCarFlag-v0 --sampler device --in-embed 64 --context 8 --batch 2 --num-steps 24 --prepopulate 60 "
              "--max-episode-steps 12 --history 8 --heads 4 --layers 1 --buf-size 240 --eval-frequency 12 --eval-episodes 2 --disable-wandb "
              f"--device {device}")
    assert runpy.get_args(common.split()).device_eval_envs == 0
    for name, extra in (("both", " --device-envs 3 --device-eval-envs 3"), ("evalonly", " --device-eval-envs 3")):
        agent = runpy.run_experiment(runpy.get_args((common + extra + f" --project-name {name}").split()))
        assert agent.num_train_steps == 24 or name == "evalonly"
        files = glob.glob(str(tmp_path / "policies" / name / "**" / "*_results.csv"), recursive=True)
        assert len(files) == 1
        rows = open(files[0], newline="").read().splitlines()
        assert len(rows) == 3 and [r.split(",")[1] for r in rows[1:]] == ["0", "12"]
        for row in rows[1:]:
            assert all(np.isfinite(float(v)) for v in row.split(","))
    for extra, exc in ((" --device-eval-envs 3 --eval-envs 2", ValueError), (" --device-eval-envs -1", ValueError)):
        with pytest.raises(exc):
            runpy.run_experiment(runpy.get_args((common + extra + " --project-name refused").split()))
    monkeypatch.setattr(runpy.ddp, "init_from_env", lambda *a, **k: (0, 2, 0))
    with pytest.raises(NotImplementedError):
        runpy.run_experiment(runpy.get_args((common + " --device-eval-envs 3 --project-name refused").split()))


# ------------------------------------------------------------------------------------------ 7. refusals
def check_refusals(lib, device):
    import pytest
    from dtqn_amd import _binding as B
    from dtqn_amd.agents.device_eval import DeviceEvaluator
    agent = make_agent(lib, device, "car")
    with pytest.raises(NotImplementedError):
        DeviceEvaluator(agent, "CartPole-v1", 3, 0)
    with pytest.raises(ValueError):
        DeviceEvaluator(agent, "DiscreteCarFlag-v0", 0, 0)
    with pytest.raises(ValueError):
        DeviceEvaluator(agent, "DiscreteCarFlag-v0", 3, 0, max_episode_steps=0)
    with pytest.raises(NotImplementedError):
        make_evaluator(make_agent(lib, device, "car", d_model=64, heads=8, bag_size=4), "car")
    image = make_agent(lib, device, "car")
    image.image = (1, 24, 24)
    with pytest.raises(NotImplementedError):
        make_evaluator(image, "car")
    dp = make_agent(lib, device, "car")
    dp.dp = object()
    with pytest.raises(NotImplementedError):
        make_evaluator(dp, "car")
    # the C entry points
    ev = make_evaluator(agent, "car")
    lib_, net = ev._lib_args()
    stream, theta, d = agent.engine._stream(), agent._theta_p, ev.ev
    ERR_ARG, ERR_CONFIG = B.DEFINES["DTQN_ERR_ARG"], B.DEFINES["DTQN_ERR_CONFIG"]
    begin = lambda n=net, episodes=2: lib_.dtqn_deval_begin(n, ev._ev_ref, 1, episodes, stream)
    step = lambda n=net, cur=0, n_max=1, episodes=2: lib_.dtqn_deval_step(n, theta, ev._ev_ref, 1, 0, cur, n_max, episodes, stream)
    assert begin() == 0 and step() == 0
    for field, value in (("bag_size", 4), ("img_c", 1)):
        other = B.DtqnNet.from_buffer_copy(agent.engine.actor_net)
        setattr(other, field, value)
        assert begin(ctypes.byref(other)) == ERR_CONFIG and step(ctypes.byref(other)) == ERR_CONFIG, field
    for field, value in (("n_envs", 0), ("max_episode_steps", 0), ("env_kind", B.DEFINES["DTQN_ROLLOUT_MEMORY"]), ("env_kind", 7)):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert begin() == ERR_ARG and step() == ERR_ARG, (field, value)
        setattr(d, field, keep)
    mem = B.DtqnNet.from_buffer_copy(agent.engine.actor_net)      # observation and action counts that do not fit CarFlag
    mem.obs_dim = 4
    assert begin(ctypes.byref(mem)) == ERR_ARG
    mem.obs_dim, mem.num_actions = 3, 4
    assert begin(ctypes.byref(mem)) == ERR_ARG
    assert begin(episodes=-1) == ERR_ARG and begin(episodes=ev.max_episodes + 1) == ERR_ARG
    assert step(episodes=-1) == ERR_ARG and step(episodes=ev.max_episodes + 1) == ERR_ARG
    assert step(cur=2) == ERR_ARG and step(cur=-1) == ERR_ARG
    assert step(n_max=0) == ERR_ARG and step(n_max=agent.context_len + 1) == ERR_ARG
    assert begin() == 0 and step() == 0
    ev.get_state()
