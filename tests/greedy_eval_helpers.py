"""Shared by test_greedy_eval.py (HIP emulation on the CPU) and test_gpu_greedy_eval.py (MI355X): the greedy entry points with idle
environments (dtqn_actor_greedy_batch, dtqn_img_actor_greedy_batch) and dtqn_amd.agents.vector.VectorEvaluator.

Shapes: the smallest that reach each kernel family -- whole-sequence d_model 16 / 2 heads / context 8, row-block d_model 64 / 8 heads /
context 70 (two 64-row blocks), bag: the row-block shape with bag_size 4, image: (1, 24, 24) / d_model 64 / context 4.  N = 5 environments
with the pattern live, idle, live, live, idle and ragged prefixes that include 1 and the full context."""
import ctypes

import numpy as np
import torch

from oracle import dtqn_oracle as O

from helpers import net_from_cfg, pack_theta, ptr

WHOLE = dict(obs_dim=3, num_actions=4, inner_embed_size=16, num_heads=2, history_len=8)
ROWBLOCK = dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=8, history_len=70, num_layers=1)
LIVE = (True, False, True, True, False)
SENTINEL = -12345.0


def live_lens(L):
    """len_i of the five environments: 1, the full context and one in between on the live ones, 0 on the idle ones."""
    return [1, 0, L, max(2, L // 2 + 1), 0]


def stage(net, lens, obs_list, act_list, device):
    """The packed block of dtqn_actor_forward_batch for len(lens) environments (len 0: nothing staged) -> (ctx_h, n_max)."""
    from dtqn_amd.agents.vector import actor_block
    L, Od, N = net.ctx_len, net.obs_dim, len(lens)
    pin = (lambda t: t.pin_memory()) if device != "cpu" else (lambda t: t)
    _, ctx_h, o, a, ln = actor_block(N, L, Od, lambda nbytes: pin(torch.zeros(nbytes, dtype=torch.uint8)))
    for i, n in enumerate(lens):
        ln[i] = n
        if n > 0:
            o[i, :n], a[i, :n] = obs_list[i], act_list[i]
    return ctx_h, max([1] + list(lens))


def call(lib, net, theta, ctx_h, N, n_max, device, stream, greedy):
    """One call of the greedy entry point (greedy=True) or of dtqn_actor_forward_batch on the block -> (rc, q_last [N][A], actions [N])."""
    L, A = net.ctx_len, net.num_actions
    q_last = torch.full((N, A), SENTINEL)
    actions = torch.full((N,), 77, dtype=torch.int32)
    if device != "cpu":
        q_last, actions = q_last.pin_memory(), actions.pin_memory()
    ctx_d = torch.zeros(ctx_h.numel(), dtype=torch.uint8, device=device)
    q_d = torch.full((N * L * A,), float("nan"), device=device)
    need = lib.dtqn_forward_workspace_floats(ctypes.byref(net), N)
    ws = torch.zeros(max(1, need), device=device)
    wsp = ptr(ws) if need > 0 else None
    if greedy:
        rc = lib.dtqn_actor_greedy_batch(ctypes.byref(net), ptr(theta), ptr(ctx_h), ptr(ctx_d), N, n_max, ptr(q_d), ptr(q_last), ptr(actions),
                                         wsp, 0, 0, 0, stream)
    else:
        rc = lib.dtqn_actor_forward_batch(ctypes.byref(net), ptr(theta), ptr(ctx_h), ptr(ctx_d), N, n_max, ptr(q_d), ptr(q_last), wsp, 0, 0, 0,
                                          stream)
    if device != "cpu":
        torch.cuda.synchronize()
    if rc == 0 and need > 0 and not net.tiled:
        assert not ws[lib.dtqn_td_xch_floats(ctypes.byref(net), N):].any()           # hand-over flags lowered again
    return rc, q_last.numpy().copy(), actions.numpy().copy()


def make_inputs(cfg, lens, seed=5):
    rng = np.random.default_rng(seed)
    obs = [rng.uniform(-1, 1, size=(n, cfg.obs_dim)).astype(np.float32) for n in lens]
    act = [rng.integers(0, cfg.num_actions, size=n) for n in lens]
    return obs, act


def check_entry_parity(lib, kw, device="cpu", stream=None):
    """The live environments' rows from the greedy entry equal, bit for bit, the rows dtqn_actor_forward_batch gives on the live subset
    alone (the same kernels on independent sequences); actions are the arg-max; idle environments get -1 and keep their Q sentinel."""
    cfg = O.NetCfg(**kw)
    net = net_from_cfg(lib, cfg)
    theta = torch.from_numpy(pack_theta(net, O.init_params(cfg, seed=41, perturb=True))).to(device)
    lens = live_lens(cfg.history_len)
    assert [n > 0 for n in lens] == list(LIVE) and 1 in lens and cfg.history_len in lens
    obs, act = make_inputs(cfg, lens)
    N, live = len(lens), [i for i, n in enumerate(lens) if n > 0]
    ctx_h, n_max = stage(net, lens, obs, act, device)
    rc, q, actions = call(lib, net, theta, ctx_h, N, n_max, device, stream, greedy=True)
    assert rc == 0 and lib.dtqn_debug_last_actor_live() == len(live)
    sub_h, sub_max = stage(net, [lens[i] for i in live], [obs[i] for i in live], [act[i] for i in live], device)
    assert sub_max == n_max
    rc, q_sub, _ = call(lib, net, theta, sub_h, len(live), sub_max, device, stream, greedy=False)
    assert rc == 0 and np.isfinite(q_sub).all()
    for k, i in enumerate(live):
        assert np.array_equal(q[i], q_sub[k]), (i, q[i], q_sub[k])
        assert actions[i] == np.argmax(q[i]), (i, actions[i], q[i])
    for i in range(N):
        if i not in live:
            assert actions[i] == -1 and (q[i] == SENTINEL).all(), (i, actions[i], q[i])
    # every environment idle: nothing is launched, the answer is -1 everywhere
    idle_h, _ = stage(net, [0] * N, obs, act, device)
    rc, q0, a0 = call(lib, net, theta, idle_h, N, 0, device, stream, greedy=True)
    assert rc == 0 and lib.dtqn_debug_last_actor_live() == 0 and (a0 == -1).all() and (q0 == SENTINEL).all()
    # every environment live: the whole block, as dtqn_actor_forward_batch runs it
    full = [1, 2, cfg.history_len, 3, cfg.history_len - 1]
    fobs, fact = make_inputs(cfg, full, seed=6)
    full_h, full_max = stage(net, full, fobs, fact, device)
    rc, qg, ag = call(lib, net, theta, full_h, N, full_max, device, stream, greedy=True)
    rc2, qf, _ = call(lib, net, theta, full_h, N, full_max, device, stream, greedy=False)
    assert rc == 0 and rc2 == 0 and lib.dtqn_debug_last_actor_live() == N
    assert np.array_equal(qg, qf) and np.array_equal(ag, np.argmax(qf, axis=1))


def check_argument_errors(lib, device="cpu", stream=None):
    from dtqn_amd import _binding as B
    cfg = O.NetCfg(**WHOLE)
    net = net_from_cfg(lib, cfg)
    theta = torch.from_numpy(pack_theta(net, O.init_params(cfg, seed=1))).to(device)
    obs, act = make_inputs(cfg, [4, 8])
    ERR = B.DEFINES["DTQN_ERR_ARG"]
    for lens, n_max in (([4, 9], 8), ([-1, 8], 8), ([4, 8], 7), ([4, 8], 9)):
        h, _ = stage(net, [4, 8], obs, act, device)
        h.numpy()[-8:].view(np.int32)[:] = lens
        assert call(lib, net, theta, h, 2, n_max, device, stream, greedy=True)[0] == ERR, (lens, n_max)


def check_ties(lib, kw, device="cpu", stream=None):
    """A Q head whose last layer has zero weight: Q is its bias on every row.  Two equal maxima give the index of the first, an all-equal
    bias gives 0 (torch.argmax / np.argmax)."""
    cfg = O.NetCfg(**kw)
    net = net_from_cfg(lib, cfg)
    lens = live_lens(cfg.history_len)
    obs, act = make_inputs(cfg, lens)
    for bias, want in (([0.25, 1.5, -2.0, 1.5], 1), ([0.5, 0.5, 0.5, 0.5], 0), ([-3.0, -3.0, -1.0, -1.0], 2)):
        params = O.init_params(cfg, seed=41, perturb=True)
        params["ffn.2.weight"] = torch.zeros_like(params["ffn.2.weight"])
        params["ffn.2.bias"] = torch.tensor(bias, dtype=torch.float32)
        theta = torch.from_numpy(pack_theta(net, params)).to(device)
        ctx_h, n_max = stage(net, lens, obs, act, device)
        rc, q, actions = call(lib, net, theta, ctx_h, len(lens), n_max, device, stream, greedy=True)
        assert rc == 0
        for i, n in enumerate(lens):
            if n > 0:
                assert np.array_equal(q[i], np.asarray(bias, dtype=np.float32)) and actions[i] == want == np.argmax(q[i]), (bias, i, q[i], actions[i])
            else:
                assert actions[i] == -1


# ------------------------------------------------------------------------------------------ agents and environments
IMG_SHAPE, IMG_L, IMG_A = (1, 24, 24), 4, 4


def make_image_agent(lib, device, seed=3, max_steps=11):
    """lib: the emulation library (agent on the CPU), or None for the product engine on `device`."""
    from dtqn_amd.agents.dtqn import DtqnAgent
    from dtqn_amd.networks.dtqn import DTQN
    from dtqn_amd.utils.random import set_global_seed
    set_global_seed(seed)

    def factory():
        m = DTQN(IMG_SHAPE, IMG_A, 8, 0, 64, 8, 1, IMG_L, **({"_test_lib": lib} if lib is not None else {}))
        m._allow_cpu = lib is not None
        return m.to(device)
    return DtqnAgent(factory, buffer_size=24 * max_steps, device=torch.device(device), env_obs_length=IMG_SHAPE, max_env_steps=max_steps,
                     obs_mask=0, num_actions=IMG_A, is_discrete_env=False, batch_size=2, context_len=IMG_L, history=IMG_L,
                     target_update_frequency=1000, sampler="device", sample_seed=seed)


def make_vector_agent(lib, device, env_id, d_model, heads, layers, context, bag_size=0, seed=11, q_scale=100.0):
    """An agent for one of the project's environments through get_agent, as run.py builds it."""
    from dtqn_amd import envs
    from dtqn_amd.networks.dtqn import DTQN
    from dtqn_amd.utils import agent_utils
    from dtqn_amd.utils.random import set_global_seed
    env = envs.make(env_id)
    set_global_seed(seed, env)
    orig = agent_utils.MODEL_MAP["DTQN"]
    if lib is not None:          # CPU kernel emulation: the network factory needs the test library
        def emu_dtqn(*a, **k):
            m = DTQN(*a, _test_lib=lib, **k)
            m._allow_cpu = True
            return m
        agent_utils.MODEL_MAP["DTQN"] = emu_dtqn
    try:
        agent = agent_utils.get_agent("DTQN", [env], 8, 0, d_model, 2000, device, 3e-4, 4, context, -1, context, 1000, 0.99, heads, layers,
                                      0.0, False, "res", "learned", bag_size, sampler="reference", sample_seed=seed)
    finally:
        agent_utils.MODEL_MAP["DTQN"] = orig
    # a freshly initialised Q head gives values of a few 1e-3, whose top-two gaps sit at the Q bound: a head 100 x as steep, as after training
    sd = {k: v.clone() for k, v in agent.policy_network.state_dict().items()}
    sd["ffn.2.weight"] = sd["ffn.2.weight"] * q_scale
    agent.policy_network.load_state_dict(sd)
    agent.target_update()
    return agent


class EpisodeSeeded:
    """An environment re-seeded at every reset with base + the number of the episode it is about to play, so that a trajectory depends on
    the episode's number and the actions alone.  first / stride: the episodes this copy plays (VectorEvaluator deals episode i, i + N, ...
    to environment i).  Keeps (episode, [actions]) of everything it played."""

    def __init__(self, env, base, first=0, stride=1, limits=None):
        self.env, self.base, self.next, self.stride, self.limits = env, base, first, stride, limits
        self.observation_space, self.action_space = env.observation_space, env.action_space
        self._max_episode_steps = getattr(env, "_max_episode_steps", None)
        self.played = {}

    def seed(self, seed=None):
        return self.env.seed(seed)

    def reset(self):
        inner = self.env
        while hasattr(inner, "env"):
            inner = inner.env
        inner.np_random = None              # (the project's environments keep the stream of their first seed() otherwise)
        self.env.seed(self.base + self.next)
        if self.limits is not None:         # a step limit per episode number (a TimeLimit wrapper): episodes of known, different lengths
            self.env._max_episode_steps = self.limits[self.next % len(self.limits)]
        self.current = self.played.setdefault(self.next, [])
        assert not self.current, "an episode was dealt twice"
        self.next += self.stride
        return self.env.reset()

    def step(self, action):
        self.current.append(int(action))
        return self.env.step(action)


def seeded_copies(env_id, n, base, limits=None):
    from dtqn_amd import envs
    return [EpisodeSeeded(envs.make(env_id), base, first=i, stride=n, limits=limits) for i in range(n)]


def agent_fingerprint(agent):
    """What an evaluation must leave as it found it."""
    from dtqn_amd.utils.random import RNG
    ctx = lambda c: tuple(np.array(getattr(c, k), copy=True) for k in ("obs", "action", "reward", "done") if hasattr(c, k)) + (int(c.timestep),)
    return {"train_ctx": ctx(agent.train_context), "eval_ctx": ctx(agent.eval_context), "pos": list(agent.replay_buffer.pos),
            "rng": repr(RNG.rng.bit_generator.state), "steps": int(agent.num_train_steps), "theta": agent.policy_network.flat.detach().cpu().clone()}


def same_fingerprint(a, b):
    for k in ("train_ctx", "eval_ctx"):
        assert all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
    assert a["pos"] == b["pos"] and a["rng"] == b["rng"] and a["steps"] == b["steps"] and torch.equal(a["theta"], b["theta"])


def check_evaluator_against_the_sequential_loop(lib, device, env_id, shape_kw, base, episodes=7, n_envs=3, limits=None):
    """VectorEvaluator with N = 3 against itself with N = 1 (exact: that isolates the batching), and against run.evaluate through
    agent.get_action (other kernels) step by step: a step counts only where the single-environment Q row's top-two gap exceeds
    1e-4 max(1, |Q|max), the project's Q bound; at most 2 % of the steps may be left out."""
    import run as runpy
    from dtqn_amd import envs
    from dtqn_amd.agents.vector import VectorEvaluator
    agent = make_vector_agent(lib, device, env_id, **shape_kw)
    before = agent_fingerprint(agent)
    copies3 = seeded_copies(env_id, n_envs, base, limits)
    got3 = VectorEvaluator(agent, copies3).evaluate(episodes)
    same_fingerprint(before, agent_fingerprint(agent))
    assert agent.train_mode.name == "TRAIN"
    copies1 = seeded_copies(env_id, 1, base, limits)
    got1 = VectorEvaluator(agent, copies1).evaluate(episodes)
    same_fingerprint(before, agent_fingerprint(agent))
    print(env_id, "N=3", got3, "N=1", got1)
    assert got3 == got1
    played3 = {}
    for c in copies3:
        played3.update(c.played)
    assert sorted(played3) == list(range(episodes)) and played3 == copies1[0].played
    assert [sorted(c.played) for c in copies3] == [list(range(i, episodes, n_envs)) for i in range(n_envs)]
    # -- the single-environment actor on the same episodes
    seq_env = EpisodeSeeded(envs.make(env_id), base, limits=limits)
    rows, orig_get = [], agent.get_action

    def get_action(epsilon=0.0):
        a = orig_get(epsilon=epsilon)
        rows.append((a, agent._q_np.copy() if agent.bag.size == 0 else None))
        return a
    agent.get_action = get_action
    try:
        seq = runpy.evaluate(agent, seq_env, episodes)
    finally:
        agent.get_action = orig_get
    total = left_out = k = 0
    for ep in range(episodes):
        mine, theirs = played3[ep], seq_env.played[ep]
        comparable = True
        for t, a_seq in enumerate(theirs):
            _, q = rows[k]
            k += 1
            total += 1
            if q is not None:
                top = np.sort(q)[::-1]
                clear = float(top[0] - top[1]) > 1e-4 * max(1.0, float(np.abs(q).max()))
            else:
                clear = True
            if not comparable or not clear:
                left_out += 1
                if t >= len(mine) or mine[t] != a_seq:
                    comparable = False      # a near-tie went the other way: the rest of this episode is another trajectory
                continue
            assert t < len(mine) and mine[t] == a_seq, (env_id, ep, t, mine[:t + 1], theirs[:t + 1], q)
        if comparable:
            assert len(mine) == len(theirs), (env_id, ep)
    print(env_id, "steps", total, "left out", left_out, "sequential", seq)
    assert k == len(rows) and left_out <= 0.02 * total, (left_out, total)
    if left_out == 0:
        assert tuple(seq) == tuple(got3)
    return got3, total, left_out


# ------------------------------------------------------------------------------------------ image evaluation
def check_image_evaluation(lib, device):
    """A scripted evaluation with frozen parameters: three environments with episodes of 2, 5 and 11 steps play 5 episodes (environment
    0: episodes 0 and 3, environment 1: 1 and 4, environment 2: 2), so environments go idle at different times.  Every frame is encoded
    exactly once; an idle environment's ring rows keep their bytes; Q of every live row equals the module forward bit for bit; after one
    optimizer step in between every live frame is encoded again."""
    import image_vector_helpers as IV
    from dtqn_amd.agents.vector import VectorEvaluator
    lengths, episodes = (2, 5, 11), 5
    N, L, O, D = len(lengths), IMG_L, int(np.prod(IMG_SHAPE)), 64

    def run(train_before_call=None):
        agent = make_image_agent(lib, device)
        if train_before_call is not None:
            IV.prefill(agent, IMG_SHAPE)
        elib = agent.engine.lib
        before = agent_fingerprint(agent)
        ev = VectorEvaluator(agent, [IV.PixelEnv(IMG_SHAPE, n, 100 + k) for k, n in enumerate(lengths)])
        orig, log, hist = ev._greedy_actions, [], [[] for _ in range(N)]

        def greedy_actions():
            call = len(log)
            if call == train_before_call:
                agent.train()
            live = ev.live.copy()
            for i in range(N):
                if live[i]:
                    if ev.contexts[i].timestep == 0:
                        hist[i] = []
                    hist[i].append(ev.episodes[i][0].copy())
            frames0, embs0 = ev._frame_ring.cpu().numpy().reshape(N, L, O).copy(), ev._emb_ring.cpu().numpy().reshape(N, L, D).copy()
            valid0 = ev._valid.copy()
            actions = orig().copy()
            frames1, embs1 = ev._frame_ring.cpu().numpy().reshape(N, L, O), ev._emb_ring.cpu().numpy().reshape(N, L, D)
            windows = sum(min(L, ev.contexts[i].timestep + 1) for i in range(N) if live[i])
            log.append((int(elib.dtqn_debug_last_img_actor_tokens()), int(ev._fresh_np.sum()), windows, int(live.sum())))
            assert elib.dtqn_debug_last_actor_live() == int(live.sum())
            for i in range(N):
                if not live[i]:
                    assert actions[i] == -1 and ev._len_np[i] == 0
                    assert frames0[i].tobytes() == frames1[i].tobytes() and embs0[i].tobytes() == embs1[i].tobytes(), (call, i)
                    assert np.array_equal(valid0[i], ev._valid[i])
            idx = [i for i in range(N) if live[i]]
            assert np.array_equal(actions[idx], np.argmax(ev._q_np[idx], axis=1))
            if train_before_call is None and call in (0, 3, 4, 10):      # windows of one frame; all live and full; the first idle; one live
                rows = IV.module_rows(agent, [np.stack(hist[i][-L:]) for i in idx])
                assert np.array_equal(ev._q_np[idx], rows), (call, ev._q_np[idx], rows)
            return actions
        ev._greedy_actions = greedy_actions
        result = ev.evaluate(episodes)
        if train_before_call is None:
            same_fingerprint(before, agent_fingerprint(agent))
        return result, log

    (sr, ret, length), log = run()
    pushed = sum(lengths[e % N] for e in range(episodes))          # an episode of T steps shows T frames to the actor (the last one ends it)
    print("tokens, fresh, window rows, live per call:", log)
    assert length == pushed / episodes and len(log) == 11
    assert [t for t, _, _, _ in log] == [f for _, f, _, _ in log] and sum(t for t, _, _, _ in log) == pushed == 25
    assert [n for _, _, _, n in log] == [3, 3, 3, 3, 2, 2, 2, 2, 2, 2, 1]
    k = 3                                                          # every environment is live and has a window of more than one frame
    _, moved = run(train_before_call=k)
    assert moved[k][0] == moved[k][2] == 2 + 4 + 4 and moved[k][1] == 3, moved[k]
    assert [t for j, (t, _, _, _) in enumerate(moved) if j != k] == [f for j, (_, f, _, _) in enumerate(moved) if j != k]
    assert [f for _, f, _, _ in moved] == [f for _, f, _, _ in log]


# ------------------------------------------------------------------------------------------ bag networks
def check_bag_evaluator(lib, device, episodes=2, n_envs=2, base=700, limits=(73, 20)):
    """Bag networks (the row-block shape with bag_size 4) evaluate through the module forward over the environments that still play:
    N = 2 gives exactly what N = 1 gives, and the agent is as found.  Memory under step limits of 73 and 20: the first episode outlives
    the context of 70, which evicts into the bag; the second environment is idle for most of it."""
    from dtqn_amd.agents.vector import VectorEvaluator
    agent = make_vector_agent(lib, device, "Memory-5-v0", d_model=64, heads=8, layers=1, context=70, bag_size=4)
    before = agent_fingerprint(agent)
    c3, c1 = seeded_copies("Memory-5-v0", n_envs, base, limits), seeded_copies("Memory-5-v0", 1, base, limits)
    ev3 = VectorEvaluator(agent, c3)
    got3, got1 = ev3.evaluate(episodes), VectorEvaluator(agent, c1).evaluate(episodes)
    print("bag N=2", got3, "N=1", got1)
    same_fingerprint(before, agent_fingerprint(agent))
    played = {}
    for c in c3:
        played.update(c.played)
    assert got3 == got1 and played == c1[0].played
    assert max(len(a) for a in played.values()) > 70, "no episode outlived the context: the bag was never used"
    assert (ev3.bags[0].obss != agent.obs_mask).any(), "nothing reached the bag"


# ------------------------------------------------------------------------------------------ run.py
def check_run_py_plumbing(lib, device, monkeypatch, tmp_path):
    """--eval-envs 1 evaluates through run.evaluate, called as before, and builds no evaluator; --eval-envs 3 evaluates through
    VectorEvaluator alone and logs the same CSV header with one row per evaluation."""
    import run as runpy
    from dtqn_amd.agents import vector
    from dtqn_amd.networks.dtqn import DTQN
    from dtqn_amd.utils import agent_utils
    if lib is not None:
        def emu_dtqn(*a, **k):
            m = DTQN(*a, _test_lib=lib, **k)
            m._allow_cpu = True
            return m
        monkeypatch.setitem(agent_utils.MODEL_MAP, "DTQN", emu_dtqn)
    monkeypatch.chdir(tmp_path)
    calls = {"evaluate": [], "evaluator": 0, "vector": []}
    orig_evaluate, orig_vec = runpy.evaluate, vector.VectorEvaluator.evaluate

    def evaluate(*a, **k):
        calls["evaluate"].append((len(a), sorted(k)))
        return orig_evaluate(*a, **k)

    def vec_evaluate(self, episodes):
        calls["vector"].append((self.n, episodes))
        return orig_vec(self, episodes)
    monkeypatch.setattr(runpy, "evaluate", evaluate)
    monkeypatch.setattr(vector.VectorEvaluator, "evaluate", vec_evaluate)
    common = ("--envs DiscreteCarFlag-v0 --num-steps 12 --prepopulate 300 --batch 4 --context 8 --history 8 --in-embed 16 --heads 2 "
              f"--layers 1 --buf-size 2000 --eval-frequency 6 --eval-episodes 4 --disable-wandb --device {device}")

    def results(project):
        import glob
        files = glob.glob(str(tmp_path / "policies" / project / "**" / "*_results.csv"), recursive=True)
        assert len(files) == 1
        return open(files[0], newline="").read().splitlines()
    assert runpy.get_args(common.split()).eval_envs == 1
    runpy.run_experiment(runpy.get_args((common + " --project-name one").split()))
    assert calls["evaluate"] == [(3, [])] * 2 and not calls["vector"]            # evaluate(agent, eval_env, eval_episodes) at steps 0 and 6
    one = results("one")
    runpy.run_experiment(runpy.get_args((common + " --project-name three --eval-envs 3").split()))
    assert len(calls["evaluate"]) == 2 and calls["vector"] == [(3, 4)] * 2
    three = results("three")
    assert three[0] == one[0] == "Hours,Step,DiscreteCarFlag-v0/SuccessRate,DiscreteCarFlag-v0/EpisodeLength,DiscreteCarFlag-v0/Return"
    assert len(three) == len(one) == 3 and [r.split(",")[1] for r in three[1:]] == ["0", "6"]
    for row in three[1:]:
        assert all(np.isfinite(float(v)) for v in row.split(","))
    with __import__("pytest").raises(NotImplementedError):
        runpy.run_experiment(runpy.get_args((common + " --project-name r --eval-envs 3 --render").split()))


# (environment, network shape, base of the episode seeds, step limit per episode number or None = the registered limit).
# Seeds checked on the emulation: agent seed 11 with CarFlag base 300 and with Memory base 500 -- the single-environment actor alone
# leaves no step out at them (no top-two gap of its Q rows at or under the bound).  Memory runs under short step limits, one of them past
# 64 rows (the second row block), so that a case stays at a few seconds.
EVALUATOR_CASES = [
    ("DiscreteCarFlag-v0", dict(d_model=16, heads=2, layers=2, context=8), 300, None),
    ("Memory-5-v0", dict(d_model=64, heads=8, layers=1, context=70), 500, (66, 5, 9, 12, 5, 9, 12)),
]
