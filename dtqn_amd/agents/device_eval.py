"""Device-resident greedy evaluation: a quota of evaluation episodes played by N CarFlag, Memory or tabular POMDP environments on the GPU.

`run.evaluate` and `VectorEvaluator` (agents/vector.py) make one host round trip per environment step: a forward, an awaited read-back,
a numpy environment step, a `Context` re-staged.  `DeviceEvaluator` keeps all of it in one device allocation (csrc/dtqn_deval.hip,
include/dtqn_hip.h `DtqnEval`): a vector step is `dtqn_deval_step` -- the eval-mode forward of `dtqn_actor_forward_batch` on the
resident context block, then one one-workgroup kernel that takes the arg-max, steps the environments, maintains the contexts, writes
the rows of finished episodes into a results table and posts the counters to a pinned status record.  Nothing is awaited in the loop;
the stream is drained once per evaluation and the results table comes back in one copy.

Exactly `episodes` episodes are played: environment i plays episodes i, i + N, ... and goes idle when it has none left (it keeps a
context of length 1, takes no step and is never counted).  Every draw of an episode -- CarFlag's side and start, Memory's shuffle and
shown cards, the padding action of context row 0 -- is a function of (seed, key, episode index, step within the episode, draw kind):
an episode is the same episode whatever N plays it.  `evaluate(episodes)` takes a key it never repeats, so every evaluation plays
fresh episodes; `evaluate(episodes, key=k)` replays those of key k.

What it leaves alone: the agent's train and eval contexts, `train_mode` (the forward runs in eval mode whatever it says: no dropout
key is taken), `RNG.rng`, the replay and `rb.version`.  It runs on the agent's main stream behind whatever updates are queued, so it
sees the parameters `run.evaluate` would see, and a target pass launched ahead stays valid.
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .. import _binding as B
from .. import dist as ddp
from .device_rollout import make_device_env, upload_pomdp_tables

COUNTERS = ("finished", "env_steps", "successes", "length_sum", "return_sum", "live", "vector_steps", "spare")
_STATUS_WORDS, _OFFSETS, _ROW = B.DEFINES["DTQN_DEVAL_STATUS_WORDS"], B.DEFINES["DTQN_DEVAL_OFFSETS"], B.DEFINES["DTQN_DEVAL_RESULT_BYTES"]
_ENV_INTS, _LAST_INTS = 40, 8
LAST_FIELDS = ("action", "zero", "done", "stored_done", "truncated", "success", "episode")
RESULT_DTYPE = np.dtype([("ret", "<f8"), ("length", "<i4"), ("success", "<i4"), ("env", "<i4"), ("vstep", "<i4")])
assert RESULT_DTYPE.itemsize == _ROW

_ptr = lambda t: ctypes.c_void_p(t.data_ptr())


class DeviceEvaluator:
    RUN_AHEAD = 8                  # vector steps the host may be in front of the device

    def __init__(self, agent, env_id: str, n_envs: int, seed: int, max_episode_steps: Optional[int] = None, num_pairs: Optional[int] = None,
                 max_episodes: int = 64):
        env, kind = make_device_env(env_id, max_episode_steps, "evaluation (use --eval-envs otherwise)")
        if getattr(agent, "image", None) is not None:
            raise NotImplementedError("device-resident evaluation: image networks are not covered (use --eval-envs)")
        if agent.bag.size > 0:
            raise NotImplementedError("device-resident evaluation: bag networks are not covered (use --eval-envs)")
        if agent.dp is not None or ddp.is_distributed():
            raise NotImplementedError("device-resident evaluation: data-parallel runs are not covered")
        if n_envs < 1:
            raise ValueError("device-resident evaluation needs at least one environment")
        if max_episodes < 1:
            raise ValueError("device-resident evaluation needs a results table of at least one episode")
        self.agent, self.env_id, self.n, self.seed = agent, env_id, int(n_envs), int(seed) & 0xFFFFFFFF
        eng, dev = agent.engine, agent.device
        self.L, self.O, self.A = agent.context_len, int(agent.env_obs_length), agent.num_actions
        self.kind = kind
        self.cap = int(max_episode_steps if max_episode_steps is not None else env._max_episode_steps)
        self.pairs = int(num_pairs if num_pairs is not None else getattr(env, "num_pairs", 0))
        if self.cap < 1:
            raise ValueError(f"the step cap must be at least 1, not {self.cap}")
        self.max_episodes = int(max_episodes)
        cuda = dev.type == "cuda"
        pin = (lambda t: t.pin_memory()) if cuda else (lambda t: t)
        N, L, A = self.n, self.L, self.A
        self._q_last = torch.zeros(N * A, device=dev)
        self._q_d = torch.zeros(N * L * A, device=dev)
        need = eng.lib.dtqn_forward_workspace_floats(eng._actor_net_ref, N)
        self._ws = torch.zeros(max(1, need), dtype=torch.float32, device=dev)
        self._status_h = pin(torch.zeros(_STATUS_WORDS * 8, dtype=torch.uint8))
        self._status_np = self._status_h.numpy().view(np.uint32).reshape(_STATUS_WORDS, 2)       # {word, tag} per granule
        ev = self.ev = B.DtqnEval()
        ev.status_host = self._status_h.data_ptr()
        ev.q_last, ev.q_dev, ev.workspace = self._q_last.data_ptr(), self._q_d.data_ptr(), (self._ws.data_ptr() if need > 0 else None)
        ev.env_kind, ev.n_envs, ev.max_episode_steps, ev.num_pairs = kind, N, self.cap, self.pairs
        if kind == B.DEFINES["DTQN_ROLLOUT_POMDP"]:
            self.env = env                               # the host twin: its model is what the device steps
            self._tables = upload_pomdp_tables(eng.lib, ev, env, dev)
        ev.max_episodes, ev.seed = self.max_episodes, self.seed
        self._ev_ref = ctypes.byref(ev)
        offsets = (ctypes.c_int32 * _OFFSETS)()
        nbytes = int(eng.lib.dtqn_deval_state_bytes(eng._actor_net_ref, self._ev_ref, offsets))
        if nbytes <= 0:
            raise ValueError("dtqn_deval_state_bytes refused this shape")
        self._offsets, self._nbytes = list(offsets), nbytes
        self._state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self._state_h = pin(torch.zeros(nbytes, dtype=torch.uint8))
        ev.state = self._state.data_ptr()
        self._next_key = 0         # key of the next evaluate() without a key: never repeated
        self.key = None            # key of the evaluation in progress / last played
        self.episodes = 0          # its quota
        self._step = 0             # vector steps enqueued since its begin: min(L, this + 1) bounds every live-row count
        self._n_max_floor = 0
        self._cur = 0              # the block that holds the contexts
        self._issued = 0           # vector steps enqueued since construction (event ring)
        self._seen = dict.fromkeys(COUNTERS, 0)
        self._events = [torch.cuda.Event() for _ in range(self.RUN_AHEAD)] if cuda else None
        self._results = np.zeros(0, dtype=RESULT_DTYPE)
        self._pending = True       # launches that post into the status record may still be in flight
        self._check(eng.lib.dtqn_deval_begin(eng._actor_net_ref, self._ev_ref, 0, 0, eng._stream()), "dtqn_deval_begin")
        # (the constructor's empty begin validates the descriptor against the network and leaves every environment idle)

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _check(rc: int, what: str) -> None:
        if rc == B.DEFINES["DTQN_ERR_CONFIG"]:
            raise NotImplementedError(f"{what}: this network is outside the device-resident evaluation's coverage")
        if rc != 0:
            raise RuntimeError(f"{what} failed with DTQN status {rc}")

    def _lib_args(self):
        eng = self.agent.engine
        return eng.lib, eng._actor_net_ref

    def _sync(self) -> None:
        if self.agent.device.type == "cuda":
            self.agent._main_stream.synchronize()
        self._pending = False

    def begin(self, episodes: int, key: Optional[int] = None) -> int:
        """Start an evaluation of `episodes` episodes (enqueued); -> its key.  evaluate() calls this; tests drive step() after it."""
        episodes = int(episodes)
        if episodes < 0 or episodes > self.max_episodes:
            raise ValueError(f"{episodes} episodes do not fit the results table of {self.max_episodes}")
        if key is None:
            key, self._next_key = self._next_key, self._next_key + 1
        else:
            self._next_key = max(self._next_key, int(key) + 1)
        lib, net = self._lib_args()
        if self._pending:                                # nothing of an earlier evaluation may still post into the status record
            self._sync()                                 # (evaluate() has drained the stream already: this waits only behind begin() / step() calls)
        self._status_np[:] = 0
        self._seen = dict.fromkeys(COUNTERS, 0)
        self.key, self.episodes, self._step, self._cur, self._n_max_floor = int(key) & 0xFFFFFFFF, episodes, 0, 0, 0
        self._pending = True
        self._check(lib.dtqn_deval_begin(net, self._ev_ref, self.key, episodes, self.agent.engine._stream()), "dtqn_deval_begin")
        return self.key

    def _throttle(self) -> None:
        """Never more than RUN_AHEAD vector steps in front of the device (an event per step, as DeviceVectorActor._throttle)."""
        if self._events is None:
            return                                   # (the emulation runs every launch to completion)
        k = self._issued % len(self._events)
        if self._issued >= len(self._events):
            self._events[k].synchronize()

    def next_n_max(self) -> int:
        """The row count the next step's forward runs: min(L, vector steps since the begin + 1), at least every live-row count."""
        return min(self.L, max(self._step, self._n_max_floor) + 1)

    def step(self) -> None:
        """One vector step of the evaluation in progress, enqueued: two launches."""
        agent = self.agent
        lib, net = self._lib_args()
        self._throttle()
        n_max = self.next_n_max()
        rc = lib.dtqn_deval_step(net, agent._theta_p, self._ev_ref, self.key, self._step & 0xFFFFFFFF, self._cur, n_max, self.episodes,
                                 agent.engine._stream())
        self._check(rc, "dtqn_deval_step")
        self._pending = True
        if self._events is not None:
            self._events[self._issued % len(self._events)].record(agent._main_stream)
        self._issued += 1
        self._step += 1
        self._cur ^= 1

    def poll(self) -> dict:
        """The newest complete status record of the evaluation in progress (no blocking) -> counters."""
        snap = self._status_np.copy()
        tags = snap[:, 1]
        want = 0x4000 | (self.key & 0x3FFF) if self.key is not None else -1
        if tags[0] != 0 and (tags == tags[0]).all() and int(tags[0]) >> 16 == want:          # every granule of one launch of this evaluation
            words = snap[:, 0].astype(np.uint64)
            vals = (words[0::2] | (words[1::2] << np.uint64(32))).astype(np.uint64)
            ints = vals.view(np.int64)
            got = {k: int(ints[j]) for j, k in enumerate(COUNTERS) if k != "return_sum"}
            got["return_sum"] = float(vals[4:5].view(np.float64)[0])
            if got["vector_steps"] >= self._seen["vector_steps"]:
                self._seen = got
        return dict(self._seen)

    def evaluate(self, episodes: int, key: Optional[int] = None):
        """(success rate, mean return, mean episode length) over exactly `episodes` greedy episodes, by the formulas of run.evaluate:
        success is the environment's flag or a positive return, the length is the context's timestep when the episode ends."""
        episodes = int(episodes)
        if episodes < 0 or episodes > self.max_episodes:
            raise ValueError(f"{episodes} episodes do not fit the results table of {self.max_episodes}")
        if episodes == 0:
            self._results = np.zeros(0, dtype=RESULT_DTYPE)
            return 0.0, 0.0, 0.0
        self.begin(episodes, key)
        bound = -(-episodes // self.n) * self.cap        # every environment plays at most ceil(episodes / N) episodes of at most cap steps
        while self._step < bound and self.poll()["finished"] < episodes:
            self.step()
        self._sync()
        got = self.poll()
        if got["finished"] != episodes:
            raise RuntimeError(f"device evaluation: {got['finished']} of {episodes} episodes finished in {self._step} vector steps ({got})")
        res = self._fetch_results(episodes)
        n = max(episodes, 1)
        returns = successes = steps = 0
        for ret, length, ok in zip(res["ret"].tolist(), res["length"].tolist(), res["success"].tolist()):
            returns += ret
            steps += length
            successes += ok
        return successes / n, returns / n, steps / n

    def _fetch_results(self, episodes: int) -> np.ndarray:
        """The first `episodes` rows of the results table: one copy."""
        off = self._offsets[10]
        nb = episodes * _ROW
        if self.agent.device.type == "cuda":
            with torch.cuda.stream(self.agent._main_stream):
                self._state_h[off:off + nb].copy_(self._state[off:off + nb], non_blocking=True)
            self._sync()
        else:
            self._state_h[off:off + nb].copy_(self._state[off:off + nb])
        self._results = self._state_h.numpy()[off:off + nb].copy().view(RESULT_DTYPE)
        return self._results

    def results(self) -> SimpleNamespace:
        """Per-episode arrays of the last evaluate(), in episode order: returns f64, lengths, successes, the environment that played it."""
        r = self._results
        return SimpleNamespace(returns=r["ret"].copy(), lengths=r["length"].copy(), successes=r["success"].copy(), envs=r["env"].copy(),
                               vsteps=r["vstep"].copy())

    # ---- state access (tests) ---------------------------------------------------------------------
    def _views(self, raw: np.ndarray) -> SimpleNamespace:
        N, L, O = self.n, self.L, self.O
        off = self._offsets
        sec = lambda k, nbytes, dt: raw[off[k]:off[k] + nbytes].view(dt)
        blocks = []
        for k in (8, 9):
            obs_b, act_b = N * L * O * 4, (N * L + 3) & ~3
            base = off[k]
            blocks.append(SimpleNamespace(obs=raw[base:base + obs_b].view(np.float32).reshape(N, L, O),
                                          actions=raw[base + obs_b:base + obs_b + N * L].reshape(N, L),
                                          lens=raw[base + obs_b + act_b:base + obs_b + act_b + 4 * N].view(np.int32)))
        last = sec(6, 4 * N * _LAST_INTS, np.int32).reshape(N, _LAST_INTS)
        return SimpleNamespace(
            raw=raw, counters=sec(0, 64, np.int64), env_f64=sec(1, 32 * N, np.float64).reshape(N, 4),
            env_i32=sec(2, 4 * N * _ENV_INTS, np.int32).reshape(N, _ENV_INTS), elapsed=sec(3, 4 * N, np.int32), ep_ret=sec(4, 8 * N, np.float64),
            episode=sec(5, 4 * N, np.int32), last=last, reward=last[:, 7].view(np.float32), obs_new=sec(7, 4 * N * O, np.float32).reshape(N, O),
            blocks=blocks, block=blocks[self._cur], results=sec(10, _ROW * self.max_episodes, RESULT_DTYPE))

    def get_state(self) -> SimpleNamespace:
        """A host copy of the whole device state as named numpy views (include/dtqn_hip.h lists the sections); `block` is the context
        block the next step reads.  Memory: env_i32[i] = current card | hidden values | shown table.  POMDP: env_i32[i] = state |
        observation, env_f64[i] = the recorded uniforms (u_state, u_obs of the last step | of the reset that started the episode)."""
        agent = self.agent
        lib, net = self._lib_args()
        self._check(lib.dtqn_deval_get_state(net, self._ev_ref, _ptr(self._state_h), agent.engine._stream()), "dtqn_deval_get_state")
        self._sync()
        return self._views(self._state_h.numpy().copy())

    def set_state(self, state: SimpleNamespace) -> None:
        """Write a state obtained from get_state (and edited in place) back to the device."""
        agent = self.agent
        lib, net = self._lib_args()
        self._state_h.numpy()[:] = state.raw
        # n_max = min(L, steps since the begin + 1) must go on bounding every live-row count
        self._n_max_floor = max(self._n_max_floor, int(np.clip(state.elapsed, 0, self.cap).max()), int(state.block.lens.max()) - 1)
        self._check(lib.dtqn_deval_set_state(net, self._ev_ref, _ptr(self._state_h), agent.engine._stream()), "dtqn_deval_set_state")
        self._sync()

    def q_rows(self) -> np.ndarray:
        """Tests: the Q rows the last step's actions were taken from, [N][A] (the lengths are those of the block that step read)."""
        N, A = self.n, self.A
        if not self.agent.engine.actor_net.tiled:
            return self._q_last.cpu().numpy().reshape(N, A).copy()
        st = self.get_state()
        n_max = min(self.L, max(self._step - 1, self._n_max_floor) + 1)      # the n_max of the step that ran last
        lens = st.blocks[self._cur ^ 1].lens
        q = self._q_d.cpu().numpy()[:N * n_max * A].reshape(N, n_max, A)
        return np.stack([q[i, lens[i] - 1] for i in range(N)])
