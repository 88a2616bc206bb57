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

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .. import _binding as B
from .device_env import DeviceEnvs

COUNTERS = ("finished", "env_steps", "successes", "length_sum", "return_sum", "live", "vector_steps", "spare")
_ROW = B.DEFINES["DTQN_DEVAL_RESULT_BYTES"]
LAST_FIELDS = ("action", "zero", "done", "stored_done", "truncated", "success", "episode")
RESULT_DTYPE = np.dtype([("ret", "<f8"), ("length", "<i4"), ("success", "<i4"), ("env", "<i4"), ("vstep", "<i4")])
assert RESULT_DTYPE.itemsize == _ROW


class DeviceEvaluator(DeviceEnvs):
    WHAT, FLAG, COVERAGE = "evaluation", "--eval-envs", "network"
    ENTRY, DESC = "dtqn_deval", B.DtqnEval
    COUNTERS, RETURN_SUM = COUNTERS, 4
    LAST_SECTION, BLOCK_SECTION = 6, 8

    def __init__(self, agent, env_id: str, n_envs: int, seed: int, max_episode_steps: Optional[int] = None, num_pairs: Optional[int] = None,
                 max_episodes: int = 64):
        super().__init__(agent, env_id, n_envs, seed, max_episode_steps, num_pairs)
        if max_episodes < 1:
            raise ValueError("device-resident evaluation needs a results table of at least one episode")
        if self.cap < 1:
            raise ValueError(f"the step cap must be at least 1, not {self.cap}")
        self.max_episodes = int(max_episodes)
        ev = self.ev = self._make_descriptor()
        ev.max_episodes = self.max_episodes
        self._ev_ref = self._desc_ref
        self._alloc_state(ev)
        self._next_key = 0         # key of the next evaluate() without a key: never repeated
        self.key = None            # key of the evaluation in progress / last played
        self.episodes = 0          # its quota
        self._step = 0             # vector steps enqueued since its begin: min(L, this + 1) bounds every live-row count
        self._n_max_floor = 0
        self._results = np.zeros(0, dtype=RESULT_DTYPE)
        self._pending = True       # launches that post into the status record may still be in flight
        self._call("begin", 0, 0)  # (validates the descriptor against the network and leaves every environment idle)

    # ------------------------------------------------------------------------------------------
    def _lib_args(self):
        eng = self.agent.engine
        return eng.lib, eng._actor_net_ref

    def _sync(self) -> None:
        super()._sync()
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
        if self._pending:                                # nothing of an earlier evaluation may still post into the status record
            self._sync()                                 # (evaluate() has drained the stream already: this waits only behind begin() / step() calls)
        self._status_np[:] = 0
        self._seen = dict.fromkeys(COUNTERS, 0)
        self.key, self.episodes, self._step, self._cur, self._n_max_floor = int(key) & 0xFFFFFFFF, episodes, 0, 0, 0
        self._pending = True
        self._call("begin", self.key, episodes)
        return self.key

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
        self._issue()
        self._step += 1

    def poll(self) -> dict:
        """The newest complete status record of the evaluation in progress (no blocking) -> counters."""
        return self._poll("vector_steps", 0x4000 | (self.key & 0x3FFF) if self.key is not None else -1)

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

    # ---- state access (tests): get_state / set_state / q_rows are DeviceEnvs' ----------------------------------
    def _views(self, raw: np.ndarray) -> SimpleNamespace:
        N, O = self.n, self.O
        return super()._views(raw, episode=self._section(raw, 5, 4 * N, np.int32), obs_new=self._section(raw, 7, 4 * N * O, np.float32).reshape(N, O),
                              results=self._section(raw, 10, _ROW * self.max_episodes, RESULT_DTYPE))

    def _note_state(self, state: SimpleNamespace) -> None:
        self._n_max_floor = max(self._n_max_floor, int(np.clip(state.elapsed, 0, self.cap).max()), int(state.block.lens.max()) - 1)

    def _last_n_max(self) -> int:
        return min(self.L, max(self._step - 1, self._n_max_floor) + 1)
