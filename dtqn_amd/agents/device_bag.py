"""Device-resident rollout of a bag network: the persistent-memory bag of every environment kept, filled and chosen on the GPU.

`DeviceVectorActor` (device_rollout.py) refuses a bag agent: its vector step knows nothing of bags.  `DeviceBagVectorActor` is that
actor with one bag per environment in a second device allocation (csrc/dtqn_devbag.hip, include/dtqn_hip.h `DtqnDevBag`).  A vector
step is `dtqn_rollout_step_bag`: the actor forward with the bags, the rollout's step kernel, one kernel that clears the bag of an
episode that ended, appends what a full context evicted or writes the K + 1 candidate bags, and -- on the steps where a choice can
be due -- a forward over N (K + 1) sequences and a kernel that keeps, per environment, the candidate with the highest mean-over-time
max-Q (`DtqnAgent._bag_insert`, the reference's dtqn/agents/dtqn.py:125-157).  Nothing is read back.

`may_choose`, the switch of the last two launches, is the host's: an environment can have a full context and a full bag after the
j-th vector step since `reset_all` only from j = L + K on (L rows slide out first, K of them fill the bag), and never under a step
cap below L + K.  After `set_state` the same count is taken from the state that was written.

Bags are maintained on every step, exploration included (prepopulation ends in `reset_all`, which clears them).  The replay stores
no bags: the learner draws them from the stored episodes (`dtqn_replay_gather_bag`).  The greedy evaluation of a bag run has its own
device-resident class, `DeviceBagEvaluator` (device_bag_eval.py, `--device-bag-eval-envs`): the same bag state and kernels behind the
evaluation's step kernel, with the candidate forward on a shared trunk (`dtqn_forward_bag_candidates`)."""
from __future__ import annotations

import ctypes
import math
from types import SimpleNamespace

import numpy as np
import torch

from .. import _binding as B
from .device_env import _ptr
from .device_rollout import DeviceVectorActor

BAG_COUNTERS = ("appends", "choices", "kept", "cleared")


class DeviceBags:
    """What the device-resident bags need on the host, whatever steps the environments (a mixin in front of a `DeviceEnvs` subclass: this
    rollout actor, `DeviceBagEvaluator` in device_bag_eval.py): the second allocation, the clock of `may_choose`, the views of the bag
    state, get_state / set_state and the counters."""
    BAGS = True

    def _alloc_bags(self, desc, ws_floats: int) -> None:
        """The bags' descriptor, its state, Q of the candidate forward, and one workspace of `ws_floats` (the candidate forward's size)
        that the actor forward shares."""
        agent, eng, dev = self.agent, self.agent.engine, self.agent.device
        N, K, L, A = self.n, agent.bag.size, self.L, self.A
        self.K = K
        bag = self.bag_desc = B.DtqnDevBag()
        bag.n_envs, bag.obs_mask = N, float(agent.bag.obs_mask)
        self._bag_ref = ctypes.byref(bag)
        offsets = (ctypes.c_int32 * B.DEFINES["DTQN_DEVBAG_OFFSETS"])()
        nbytes = int(eng.lib.dtqn_devbag_state_bytes(eng._actor_net_ref, self._bag_ref, offsets))
        if nbytes <= 0:
            raise ValueError("dtqn_devbag_state_bytes refused this shape")
        self._bag_offsets, self._bag_nbytes = list(offsets), nbytes
        self._bag_state = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        self._bag_state_h = self._pin(torch.zeros(nbytes, dtype=torch.uint8))
        self._q_cand = torch.zeros(N * (K + 1) * L * A, device=dev)
        if ws_floats <= 0:
            raise ValueError(f"the candidate forward of {N} x {K + 1} sequences is outside the row-block kernels' workspace")
        self._ws = torch.zeros(ws_floats, dtype=torch.float32, device=dev)
        bag.state, bag.q_cand, bag.workspace = self._bag_state.data_ptr(), self._q_cand.data_ptr(), self._ws.data_ptr()
        desc.workspace = self._ws.data_ptr()
        self._to_choice = math.inf
        self.vector_steps = self.choice_steps = 0        # vector steps enqueued; those that launched the candidate forward

    def _restart_choice_clock(self) -> None:
        """Every bag was cleared: the first vector step after which an environment can hold a full context and a full bag (never under a
        cap below L + K)."""
        self._to_choice = self.L + self.K if self.cap >= self.L + self.K else math.inf

    def _may_choose(self) -> bool:
        return self._to_choice <= 1

    def _count_step(self, may_choose: bool) -> None:
        self._to_choice = max(self._to_choice - 1, 0)
        self.vector_steps += 1
        self.choice_steps += int(may_choose)

    # ---- state access (tests) ---------------------------------------------------------------------------
    def _bag_views(self, raw: np.ndarray) -> SimpleNamespace:
        N, K, O, off = self.n, self.K, self.O, self._bag_offsets
        C = K + 1
        sec = lambda k, nbytes, dtype: raw[off[k]:off[k] + nbytes].view(dtype)
        return SimpleNamespace(
            raw=raw, obs=sec(0, 4 * N * K * O, np.float32).reshape(N, K, O), actions=sec(1, N * K, np.uint8).reshape(N, K),
            pos=sec(2, 4 * N, np.int32), cand_obs=sec(3, 4 * N * C * K * O, np.float32).reshape(N, C, K, O),
            cand_actions=sec(4, N * C * K, np.uint8).reshape(N, C, K), choosing=sec(5, 4 * N, np.int32),
            scores=sec(6, 4 * N * C, np.float32).reshape(N, C), choice=sec(7, 4 * N, np.int32),
            counters=sec(8, 8 * len(BAG_COUNTERS), np.int64), seq_ctx=sec(9, 8 * N * C, np.int32).reshape(2, N * C))

    def get_state(self) -> SimpleNamespace:
        """The environments' get_state, plus `.bag`: named views of the bag sections (include/dtqn_hip.h lists them) -- obs [N][K][O],
        actions [N][K], pos [N], cand_obs / cand_actions, choosing, scores [N][K+1], choice [N], counters (BAG_COUNTERS), seq_ctx."""
        eng = self.agent.engine
        self._check(eng.lib.dtqn_devbag_get_state(eng._actor_net_ref, self._bag_ref, _ptr(self._bag_state_h), eng._stream()), "dtqn_devbag_get_state")
        state = super().get_state()                      # (drains the stream)
        state.bag = self._bag_views(self._bag_state_h.numpy().copy())
        return state

    def set_state(self, state: SimpleNamespace) -> None:
        eng = self.agent.engine
        self._bag_state_h.numpy()[:] = state.bag.raw
        self._check(eng.lib.dtqn_devbag_set_state(eng._actor_net_ref, self._bag_ref, _ptr(self._bag_state_h), eng._stream()), "dtqn_devbag_set_state")
        super().set_state(state)                         # (drains the stream)
        # environment i slides at the step that takes `elapsed` to L, fills what is left of its bag, and chooses with the next pair
        elapsed, pos = np.clip(state.elapsed, 0, self.cap), np.clip(state.bag.pos, 0, self.K)
        self._to_choice = min(self._to_choice, int((np.maximum(self.L - elapsed, 1) + (self.K - pos)).min()))

    def bag_counters(self) -> dict:
        """Cumulative since construction (drains the stream): pairs appended, choices made, choices that kept the bag as it was, bags
        cleared by an episode end."""
        return dict(zip(BAG_COUNTERS, (int(v) for v in self.get_state().bag.counters)))


class DeviceBagVectorActor(DeviceBags, DeviceVectorActor):
    def _refuse(self, agent) -> None:
        if agent.bag.size < 1:
            raise ValueError("DeviceBagVectorActor is the device-resident rollout of a bag network (--bag-size K > 0); without a bag: "
                             "DeviceVectorActor")
        if agent.policy_network.dropout_p > 0.0:
            raise NotImplementedError("device-resident rollout of a bag network: dropout is not covered (the candidate forward would need "
                                      "a dropout key of its own)")
        super()._refuse(agent)

    def _alloc_state(self, desc) -> None:
        """The rollout's state, then the bags'."""
        super()._alloc_state(desc)
        eng = self.agent.engine
        self._alloc_bags(desc, eng.lib.dtqn_forward_workspace_floats(eng._actor_net_ref, self.n * (self.agent.bag.size + 1)))

    def _call(self, name: str, *more) -> None:
        """The rollout's entry points; `reset` is the bag path's (commit, get_state and set_state serve both)."""
        if name != "reset":
            return super()._call(name, *more)
        lib, *args = self._lib_args()
        self._check(lib.dtqn_rollout_reset_bag(*args, self._desc_ref, self._bag_ref, *more, self.agent.engine._stream()), "dtqn_rollout_reset_bag")
        self._restart_choice_clock()

    def step_all(self, epsilon: float, updates: int = 0, store: bool = True) -> None:
        """One vector step, enqueued: up to five launches (DeviceVectorActor.step_all's two, the bags' bookkeeping, and where a choice
        can be due the candidate forward and the selection).  The bags are maintained whatever epsilon is."""
        agent = self.agent
        lib, net, rp = self._lib_args()
        self._throttle()
        authorize = self._authorize(self.poll()["staged"])
        run_forward = epsilon < 1.0
        seed, step = agent._actor_drop_key() if run_forward else (0, 0)
        n_max = min(self.L, self._since_reset + 1)
        may_choose = self._may_choose()
        rc = lib.dtqn_rollout_step_bag(net, agent._theta_p, rp, self._ro_ref, self._bag_ref, self._vstep & 0xFFFFFFFF, self._cur, n_max,
                                       float(epsilon), 1 if store else 0, authorize, 1 if run_forward else 0,
                                       1 if agent.train_mode.name == "TRAIN" else 0, seed, step & 0xFFFFFFFF, 1 if may_choose else 0,
                                       agent.engine._stream())
        self._check(rc, "dtqn_rollout_step_bag")
        self._issue()
        self._vstep += 1
        self._since_reset += 1
        self.steps += self.n
        self._count_step(may_choose)
        for _ in range(updates):
            agent.train()
