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

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .. import _binding as B
from .device_env import ENV_KINDS, DeviceEnvs, make_device_env, upload_pomdp_tables  # noqa: F401  (re-exported: run.py, tests, tests/perf)

COUNTERS = ("committed", "env_steps", "successes", "finished", "length_sum", "return_sum", "staged", "dropped")
LAST_FIELDS = ("action", "explored", "done", "stored_done", "truncated", "success", "reset")


class DeviceVectorActor(DeviceEnvs):
    WHAT, FLAG, COVERAGE = "rollout", "--num-envs", "network or replay"
    ENTRY, DESC = "dtqn_rollout", B.DtqnRollout
    COUNTERS, RETURN_SUM = COUNTERS, 5
    LAST_SECTION, BLOCK_SECTION = 5, 6

    def __init__(self, agent, env_id: str, n_envs: int, seed: int, max_episode_steps: Optional[int] = None, num_pairs: Optional[int] = None):
        super().__init__(agent, env_id, n_envs, seed, max_episode_steps, num_pairs)
        rb = agent.replay_buffer
        if self.cap > rb.max_episode_steps:
            raise ValueError(f"the step cap {self.cap} exceeds the replay's {rb.max_episode_steps} rows per episode")
        rb.commit()                                      # nothing of a host producer may be left in the staging
        if rb.pos[1] != 0:
            raise ValueError("the replay has an episode in progress: flush() it before a device rollout attaches")
        self._forced = torch.full((self.n,), -1, dtype=torch.int32, device=agent.device)
        ro = self.ro = self._make_descriptor()
        ro.forced_actions = self._forced.data_ptr()
        ro.pos0 = self.pos0 = int(rb.pos[0])
        ro.pending_slots = (self.RUN_AHEAD + 2) * self.n          # at most N episodes finish per vector step
        self._ro_ref = self._desc_ref
        self._alloc_state(ro)
        self._vstep = 0            # key of the next vector step's draws: never repeated
        self._since_reset = 0      # vector steps since reset_all: min(L, this + 1) bounds every live-row count
        self.steps = 0             # env steps enqueued (the device's counter says how many have run)
        self._authorized = 0       # episodes the launches so far were allowed to write into the replay
        self._call("reset", 0)     # (validates the descriptor against the network and the replay; reset_all repeats it for the caller)

    def _refuse(self, agent) -> None:
        if agent.sampler != "device":
            raise ValueError("device-resident rollout needs --sampler device: the host mirror of the episode lengths, which the reference "
                             "sampler draws from, is only refreshed by sync()")

    # ------------------------------------------------------------------------------------------
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
        self._call("reset", self._vstep & 0xFFFFFFFF)
        self._vstep += 1           # (the reset's draws have a range of their own, but a repeated reset_all must not repeat them)
        self._since_reset, self._cur = 0, 0

    def set_forced(self, actions=None) -> None:
        """Tests: actions[i] >= 0 overrides environment i's choice on the following steps (None / -1: not forced)."""
        a = np.full(self.n, -1, dtype=np.int32) if actions is None else np.asarray(actions, dtype=np.int32).reshape(self.n)
        self._forced.copy_(torch.from_numpy(a))

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
        self._issue()
        self._vstep += 1
        self._since_reset += 1
        self.steps += self.n
        for _ in range(updates):
            agent.train()

    def poll(self) -> dict:
        """The newest complete status record (no blocking) -> counters."""
        return self._poll("env_steps")

    def counters(self) -> dict:
        """Cumulative since construction: episodes committed to the replay, env steps, successes, episodes finished, the sums of their
        lengths and returns, episodes staged for the replay, episodes dropped (0 unless the run-ahead bound was broken) -- as of the last
        launch whose status record has arrived (sync() first for exact figures)."""
        return self.poll()

    def sync(self) -> dict:
        """Drain the stream and write out the episodes that still wait in the pending ring; rb.pos and rb.episode_lengths then describe
        the device arrays exactly.  -> counters."""
        rb = self.agent.replay_buffer
        self._sync()
        got = self.poll()
        if got["staged"] > got["committed"]:
            self._call("commit", (self._vstep - 1) & 0xFFFFFFFF, self._authorize(got["staged"]))
            self._sync()
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

    # ---- state access (tests, sync): get_state / set_state / q_rows are DeviceEnvs' ------------------------------
    def _views(self, raw: np.ndarray) -> SimpleNamespace:
        N, O, T = self.n, self.O, self.agent.replay_buffer.max_episode_steps
        return super()._views(
            raw, stage_obs=self._section(raw, 8, 4 * N * (T + 1) * O, np.float32).reshape(N, T + 1, O),
            stage_act=self._section(raw, 9, N * T, np.uint8).reshape(N, T), stage_rew=self._section(raw, 10, 4 * N * T, np.float32).reshape(N, T),
            stage_done=self._section(raw, 11, N * T, np.uint8).reshape(N, T))

    def _note_state(self, state: SimpleNamespace) -> None:
        self._since_reset = max(self._since_reset, int(np.clip(state.elapsed, 0, self.cap).max()))

    def _last_n_max(self) -> int:
        return min(self.L, self._since_reset)
