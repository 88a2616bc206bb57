"""Device-resident rollout: N CarFlag, Memory or tabular POMDP environments stepped on the GPU behind the batched actor forward.

`VectorActor` (agents/vector.py) makes a round trip through Python on every vector step: N numpy environments, N `Context` objects
re-staged and copied over, N Q rows read back after an event wait, the epsilon-greedy draw in numpy, finished episodes replayed record
by record.  `DeviceVectorActor` keeps all of it in one device allocation (csrc/dtqn_rollout.hip, include/dtqn_hip.h `DtqnRollout`):
a vector step is `dtqn_rollout_step` -- the forward of `dtqn_actor_forward_batch` on the resident context block, then one
one-workgroup kernel that acts, steps the environments, maintains the contexts, writes finished episodes into the replay and posts
cumulative counters to a pinned status record.  Nothing is awaited and nothing is read back in the loop.

What the host still does for `ReplayBuffer`, whose arrays the kernel writes directly:
  * finished episodes wait in a pending ring on the device until the host has SEEN them in the status record (polled without
    blocking before every vector step); the next launch is then authorised to write them out, the k-th episode since attach to slot
    (pos0 + k) mod E.  So the host knows which launch changes the replay: it sets `rb.pos = [pos0 + authorised, 0]` -- exact in stream
    order -- and bumps `rb.version` with that launch alone.  A window drawn ahead of a commit (TdEngine pipeline) is never used, and
    the target pass launched ahead is lost only on the vector steps that really commit.  A late look only delays a commit;
  * the host stays at most RUN_AHEAD vector steps in front of the device (an event per step), which bounds the pending ring;
  * `sync()` drains the stream, writes out what still waits and refreshes `rb.episode_lengths` from the device's `ep_len`: call it
    before a checkpoint (`prepopulate` does).  The host mirror is stale in between, which is why `--sampler reference` is refused.

Differences from the host actor, by design: exploration and environment draws come from a counter-based generator keyed by
(seed, vector step, environment), not from `RNG.rng` / the environments' `np_random`; `prepopulate` discards the episodes in progress
when it has its steps (the host loop finishes its last episode); `step_all` does not know how many episodes finished (`counters()`).
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .. import _binding as B
from .. import dist as ddp
from .. import envs as _envs

ENV_KINDS = {"DiscreteCarFlag-v0": B.DEFINES["DTQN_ROLLOUT_CARFLAG"], "Memory-5-v0": B.DEFINES["DTQN_ROLLOUT_MEMORY"]}
COUNTERS = ("committed", "env_steps", "successes", "finished", "length_sum", "return_sum", "staged", "dropped")
_STATUS_WORDS, _OFFSETS = B.DEFINES["DTQN_ROLLOUT_STATUS_WORDS"], B.DEFINES["DTQN_ROLLOUT_OFFSETS"]
_ENV_INTS, _LAST_INTS = 40, 8
LAST_FIELDS = ("action", "explored", "done", "stored_done", "truncated", "success", "reset")

_ptr = lambda t: ctypes.c_void_p(t.data_ptr())


def make_device_env(env_id: str, max_episode_steps: Optional[int], what: str):
    """The host twin of the device environments -> (env, kind).  A registered id names its kind; a tabular POMDP (an id or a `.pomdp`
    path) is recognised from the made environment: a TabularPOMDP under the TimeLimit.  Anything else is refused."""
    if env_id in ENV_KINDS:
        return _envs.make(env_id), ENV_KINDS[env_id]
    if _envs.is_pomdp(env_id):
        env = _envs.make(env_id, max_episode_steps=max_episode_steps)
        if isinstance(getattr(env, "env", None), _envs.TabularPOMDP):
            return env, B.DEFINES["DTQN_ROLLOUT_POMDP"]
    raise NotImplementedError(f"device-resident {what} covers {sorted(ENV_KINDS)} and tabular POMDPs, not {env_id!r}")


def upload_pomdp_tables(lib, desc, env, device) -> torch.Tensor:
    """Pack the model's tables (start_cdf | T_cdf | O_cdf | R | D) at the offsets the library states, upload them once and point the
    descriptor (DtqnRollout / DtqnEval) at them -> the tensor, which the caller keeps alive."""
    pomdp = env.env
    S, A, Z = pomdp.model.sizes
    offsets = (ctypes.c_longlong * B.DEFINES["DTQN_POMDP_SECTIONS"])()
    nbytes = int(lib.dtqn_pomdp_table_bytes(S, A, Z, offsets))
    if nbytes <= 0:
        raise ValueError("dtqn_pomdp_table_bytes refused this model")
    tables = torch.from_numpy(pomdp.model.pack(list(offsets), nbytes)).to(device)
    desc.pomdp_tables = tables.data_ptr()
    desc.pomdp_states, desc.pomdp_actions, desc.pomdp_obs, desc.pomdp_first_obs_action = S, A, Z, pomdp.first_obs_action
    return tables


class DeviceVectorActor:
    RUN_AHEAD = 8                  # vector steps the host may be in front of the device; the pending ring is sized for them

    def __init__(self, agent, env_id: str, n_envs: int, seed: int, max_episode_steps: Optional[int] = None, num_pairs: Optional[int] = None):
        env, kind = make_device_env(env_id, max_episode_steps, "rollout (use --num-envs otherwise)")
        if getattr(agent, "image", None) is not None:
            raise NotImplementedError("device-resident rollout: image networks are not covered (use --num-envs)")
        if agent.bag.size > 0:
            raise NotImplementedError("device-resident rollout: bag networks are not covered (use --num-envs)")
        if agent.dp is not None or ddp.is_distributed():
            raise NotImplementedError("device-resident rollout: data-parallel runs are not covered")
        if agent.sampler != "device":
            raise ValueError("device-resident rollout needs --sampler device: the host mirror of the episode lengths, which the reference "
                             "sampler draws from, is only refreshed by sync()")
        if n_envs < 1:
            raise ValueError("device-resident rollout needs at least one environment")
        self.agent, self.env_id, self.n, self.seed = agent, env_id, int(n_envs), int(seed) & 0xFFFFFFFF
        eng, rb, dev = agent.engine, agent.replay_buffer, agent.device
        self.L, self.O, self.A = agent.context_len, int(agent.env_obs_length), agent.num_actions
        self.kind = kind
        self.cap = int(max_episode_steps if max_episode_steps is not None else env._max_episode_steps)
        self.pairs = int(num_pairs if num_pairs is not None else getattr(env, "num_pairs", 0))
        if self.cap > rb.max_episode_steps:
            raise ValueError(f"the step cap {self.cap} exceeds the replay's {rb.max_episode_steps} rows per episode")
        rb.commit()                                      # nothing of a host producer may be left in the staging
        if rb.pos[1] != 0:
            raise ValueError("the replay has an episode in progress: flush() it before a device rollout attaches")
        cuda = dev.type == "cuda"
        pin = (lambda t: t.pin_memory()) if cuda else (lambda t: t)
        N, L, A = self.n, self.L, self.A
        self._forced = torch.full((N,), -1, dtype=torch.int32, device=dev)
        self._q_last = torch.zeros(N * A, device=dev)
        self._q_d = torch.zeros(N * L * A, device=dev)
        need = eng.lib.dtqn_forward_workspace_floats(eng._actor_net_ref, N)
        self._ws = torch.zeros(max(1, need), dtype=torch.float32, device=dev)
        self._status_h = pin(torch.zeros(_STATUS_WORDS * 8, dtype=torch.uint8))
        self._status_np = self._status_h.numpy().view(np.uint32).reshape(_STATUS_WORDS, 2)       # {word, tag} per granule
        ro = self.ro = B.DtqnRollout()
        ro.status_host, ro.forced_actions = self._status_h.data_ptr(), self._forced.data_ptr()
        ro.q_last, ro.q_dev, ro.workspace = self._q_last.data_ptr(), self._q_d.data_ptr(), (self._ws.data_ptr() if need > 0 else None)
        ro.env_kind, ro.n_envs, ro.max_episode_steps, ro.num_pairs = kind, N, self.cap, self.pairs
        if kind == B.DEFINES["DTQN_ROLLOUT_POMDP"]:
            self.env = env                               # the host twin: its model is what the device steps
            self._tables = upload_pomdp_tables(eng.lib, ro, env, dev)
        ro.pos0, ro.seed = int(rb.pos[0]), self.seed
        ro.pending_slots = (self.RUN_AHEAD + 2) * N      # at most N episodes finish per vector step
        self.pos0 = int(rb.pos[0])
        self._ro_ref = ctypes.byref(ro)
        offsets = (ctypes.c_int32 * _OFFSETS)()
        nbytes = int(eng.lib.dtqn_rollout_state_bytes(eng._actor_net_ref, rb.dev.view_ref, self._ro_ref, offsets))
        if nbytes <= 0:
            raise ValueError("dtqn_rollout_state_bytes refused this shape")
        self._offsets, self._nbytes = list(offsets), nbytes
        self._state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self._state_h = pin(torch.zeros(nbytes, dtype=torch.uint8))
        ro.state = self._state.data_ptr()
        self._vstep = 0            # key of the next vector step's draws: never repeated
        self._since_reset = 0      # vector steps since reset_all: min(L, this + 1) bounds every live-row count
        self._cur = 0              # the block that holds the contexts
        self.steps = 0             # env steps enqueued (the device's counter says how many have run)
        self._seen = dict.fromkeys(COUNTERS, 0)
        self._authorized = 0       # episodes the launches so far were allowed to write into the replay
        self._issued = 0           # vector steps enqueued
        self._events = [torch.cuda.Event() for _ in range(self.RUN_AHEAD)] if cuda else None
        self._check(eng.lib.dtqn_rollout_reset(eng._actor_net_ref, rb.dev.view_ref, self._ro_ref, 0, eng._stream()), "dtqn_rollout_reset")
        # (the constructor's reset validates the descriptor against the network and the replay; reset_all repeats it for the caller)

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _check(rc: int, what: str) -> None:
        if rc == B.DEFINES["DTQN_ERR_CONFIG"]:
            raise NotImplementedError(f"{what}: this network or replay is outside the device-resident rollout's coverage")
        if rc != 0:
            raise RuntimeError(f"{what} failed with DTQN status {rc}")

    def _lib_args(self):
        eng = self.agent.engine
        return eng.lib, eng._actor_net_ref, self.agent.replay_buffer.dev.view_ref

    def attach(self) -> None:
        """Take the replay's position as it is now (a restored checkpoint): the next finished episode goes to slot rb.pos[0] mod E."""
        rb = self.agent.replay_buffer
        got = self.sync()
        if rb.pos[1] != 0:
            raise ValueError("the replay has an episode in progress: flush() it before a device rollout attaches")
        self.pos0 = self.ro.pos0 = int(rb.pos[0]) - got["committed"]
        if self.pos0 < 0:
            raise ValueError("the replay's position lies before the episodes this rollout has already committed")

    def reset_all(self) -> None:
        """Reset every environment and start fresh contexts; episodes in progress are dropped, counters kept."""
        lib, net, rp = self._lib_args()
        self._check(lib.dtqn_rollout_reset(net, rp, self._ro_ref, self._vstep & 0xFFFFFFFF, self.agent.engine._stream()), "dtqn_rollout_reset")
        self._vstep += 1           # (the reset's draws have a range of their own, but a repeated reset_all must not repeat them)
        self._since_reset, self._cur = 0, 0

    def set_forced(self, actions=None) -> None:
        """Tests: actions[i] >= 0 overrides environment i's choice on the following steps (None / -1: not forced)."""
        a = np.full(self.n, -1, dtype=np.int32) if actions is None else np.asarray(actions, dtype=np.int32).reshape(self.n)
        self._forced.copy_(torch.from_numpy(a))

    def _throttle(self) -> None:
        """Never more than RUN_AHEAD vector steps in front of the device: the pending ring holds what can finish in that many."""
        if self._events is None:
            return                                   # (the emulation runs every launch to completion)
        k = self._issued % len(self._events)
        if self._issued >= len(self._events):
            self._events[k].synchronize()            # the step issued RUN_AHEAD steps ago has run: its status record is in pinned memory

    def _authorize(self, staged: int) -> int:
        """The episodes a launch may write into the replay: those the host has SEEN finished.  It therefore knows which launch changes
        the replay: the version moves with that launch alone, and rb.pos is exact in stream order."""
        if staged > self._authorized:
            rb = self.agent.replay_buffer
            rb.version += 1                          # a window drawn ahead of this commit must not be used
            self._authorized = staged
            rb.pos = [self.pos0 + staged, 0]
        return self._authorized

    def step_all(self, epsilon: float, updates: int = 0, store: bool = True) -> None:
        """One vector step, enqueued: two launches (one with epsilon >= 1: the forward is skipped).  updates > 0: that many
        agent.train() calls are queued right behind it; this step's actions come from the parameters before those updates, as with
        VectorActor.step_all.  store=False: the episodes that finish are counted and dropped."""
        agent = self.agent
        lib, net, rp = self._lib_args()
        self._throttle()
        authorize = self._authorize(self.poll()["staged"])
        run_forward = epsilon < 1.0
        seed, step = agent._actor_drop_key() if run_forward else (0, 0)
        n_max = min(self.L, self._since_reset + 1)
        rc = lib.dtqn_rollout_step(net, agent._theta_p, rp, self._ro_ref, self._vstep & 0xFFFFFFFF, self._cur, n_max, float(epsilon),
                                   1 if store else 0, authorize, 1 if run_forward else 0, 1 if agent.train_mode.name == "TRAIN" else 0, seed,
                                   step & 0xFFFFFFFF, agent.engine._stream())
        self._check(rc, "dtqn_rollout_step")
        if self._events is not None:
            self._events[self._issued % len(self._events)].record(agent._main_stream)
        self._issued += 1
        self._vstep += 1
        self._since_reset += 1
        self._cur ^= 1
        self.steps += self.n
        for _ in range(updates):
            agent.train()

    def poll(self) -> dict:
        """The newest complete status record (no blocking) -> counters."""
        snap = self._status_np.copy()
        tags = snap[:, 1]
        if tags[0] != 0 and (tags == tags[0]).all():          # every granule of one launch
            words = snap[:, 0].astype(np.uint64)
            vals = (words[0::2] | (words[1::2] << np.uint64(32))).astype(np.uint64)
            ints = vals.view(np.int64)
            got = {k: int(ints[j]) for j, k in enumerate(COUNTERS) if k != "return_sum"}
            got["return_sum"] = float(vals[5:6].view(np.float64)[0])
            if got["env_steps"] >= self._seen["env_steps"]:
                self._seen = got
        return dict(self._seen)

    def counters(self) -> dict:
        """Cumulative since construction: episodes committed to the replay, env steps, successes, episodes finished, the sums of their
        lengths and returns, episodes staged for the replay, episodes dropped (0 unless the run-ahead bound was broken) -- as of the last
        launch whose status record has arrived (sync() first for exact figures)."""
        return self.poll()

    def sync(self) -> dict:
        """Drain the stream and write out the episodes that still wait in the pending ring; rb.pos and rb.episode_lengths then describe
        the device arrays exactly.  -> counters."""
        agent, rb = self.agent, self.agent.replay_buffer
        stream = agent._main_stream if agent.device.type == "cuda" else None
        if stream is not None:
            stream.synchronize()
        got = self.poll()
        if got["staged"] > got["committed"]:
            lib, net, rp = self._lib_args()
            authorize = self._authorize(got["staged"])
            self._check(lib.dtqn_rollout_commit(net, rp, self._ro_ref, (self._vstep - 1) & 0xFFFFFFFF, authorize, agent.engine._stream()),
                        "dtqn_rollout_commit")
            if stream is not None:
                stream.synchronize()
            got = self.poll()
        if got["env_steps"] != self.steps or got["committed"] != got["staged"]:
            raise RuntimeError(f"device rollout: the status record reports {got}, {self.steps} env steps were enqueued")
        if got["dropped"]:
            raise RuntimeError(f"device rollout: {got['dropped']} finished episodes found the pending ring full")
        rb.episode_lengths[:] = rb.dev.ep_len.cpu().numpy()
        return got

    def prepopulate(self, steps: int) -> None:
        """At least `steps` uniformly random env steps into the replay (epsilon = 1: no forward is launched).  The host looks at the status
        record before every vector step and stays at most RUN_AHEAD steps in front of the device.  The episodes in progress at the end
        are discarded (the host loop finishes its last one)."""
        target = self.steps + int(steps)
        self.reset_all()
        while self.steps < target:
            self.step_all(1.0)
        self.sync()
        self.reset_all()

    # ---- state access (tests, sync) -----------------------------------------------------------------
    def _views(self, raw: np.ndarray) -> SimpleNamespace:
        N, L, O, A, T = self.n, self.L, self.O, self.A, self.agent.replay_buffer.max_episode_steps
        off = self._offsets
        sec = lambda k, nbytes, dt: raw[off[k]:off[k] + nbytes].view(dt)
        blocks = []
        for k in (6, 7):
            obs_b, act_b = N * L * O * 4, (N * L + 3) & ~3
            base = off[k]
            blocks.append(SimpleNamespace(obs=raw[base:base + obs_b].view(np.float32).reshape(N, L, O),
                                          actions=raw[base + obs_b:base + obs_b + N * L].reshape(N, L),
                                          lens=raw[base + obs_b + act_b:base + obs_b + act_b + 4 * N].view(np.int32)))
        last = sec(5, 4 * N * _LAST_INTS, np.int32).reshape(N, _LAST_INTS)
        return SimpleNamespace(
            raw=raw, counters=sec(0, 64, np.int64), env_f64=sec(1, 32 * N, np.float64).reshape(N, 4),
            env_i32=sec(2, 4 * N * _ENV_INTS, np.int32).reshape(N, _ENV_INTS), elapsed=sec(3, 4 * N, np.int32), ep_ret=sec(4, 8 * N, np.float64),
            last=last, reward=last[:, 7].view(np.float32), blocks=blocks, block=blocks[self._cur],
            stage_obs=sec(8, 4 * N * (T + 1) * O, np.float32).reshape(N, T + 1, O), stage_act=sec(9, N * T, np.uint8).reshape(N, T),
            stage_rew=sec(10, 4 * N * T, np.float32).reshape(N, T), stage_done=sec(11, N * T, np.uint8).reshape(N, T))

    def get_state(self) -> SimpleNamespace:
        """A host copy of the whole device state as named numpy views (include/dtqn_hip.h lists the sections); `block` is the context
        block the next step reads.  Memory: env_i32[i] = current card | hidden values | shown table.  POMDP: env_i32[i] = state |
        observation, env_f64[i] = the recorded uniforms (u_state, u_obs of the last step | of the reset that started the episode)."""
        agent = self.agent
        lib, net, rp = self._lib_args()
        self._check(lib.dtqn_rollout_get_state(net, rp, self._ro_ref, _ptr(self._state_h), agent.engine._stream()), "dtqn_rollout_get_state")
        if agent.device.type == "cuda":
            agent._main_stream.synchronize()
        return self._views(self._state_h.numpy().copy())

    def set_state(self, state: SimpleNamespace) -> None:
        """Write a state obtained from get_state (and edited in place) back to the device."""
        agent = self.agent
        lib, net, rp = self._lib_args()
        self._state_h.numpy()[:] = state.raw
        # n_max = min(L, steps since the reset + 1) must go on bounding every live-row count
        self._since_reset = max(self._since_reset, int(np.clip(state.elapsed, 0, self.cap).max()))
        self._check(lib.dtqn_rollout_set_state(net, rp, self._ro_ref, _ptr(self._state_h), agent.engine._stream()), "dtqn_rollout_set_state")
        if agent.device.type == "cuda":
            agent._main_stream.synchronize()

    def q_rows(self) -> np.ndarray:
        """Tests: the Q rows the last step's actions were taken from, [N][A] (the lengths are those of the block that step read)."""
        N, A = self.n, self.A
        if not self.agent.engine.actor_net.tiled:
            return self._q_last.cpu().numpy().reshape(N, A).copy()
        st = self.get_state()
        n_max = min(self.L, self._since_reset)              # the n_max of the step that ran last
        lens = st.blocks[self._cur ^ 1].lens
        q = self._q_d.cpu().numpy()[:N * n_max * A].reshape(N, n_max, A)
        return np.stack([q[i, lens[i] - 1] for i in range(N)])
