"""Vectorised rollout: N host environments per learner, ONE batched actor launch per vector step.

The reference steps one environment per network forward (run.py:356-377); at 1 env step : 1 update the actor forward
and the Python env step sit on the critical path of every update.  `VectorActor` keeps N environments and N rolling
contexts, stages all N prefixes through one pinned buffer, runs `dtqn_actor_forward_batch` (ragged prefixes in one
launch: every sequence runs max n_i rows, causality keeps shorter prefixes exact) and reads the N Q-rows back from
pinned memory.

Replay semantics stay the reference's: an episode becomes sampleable when it has FINISHED (replay_buffer.py:141-145
excludes the slot in progress).  With N episodes in progress at once, each environment collects its episode on the
host and replays it into the buffer's producer API (store_obs, store x len, flush) when it ends, so the device arrays
hold exactly what the single-environment loop would have written for that episode.

Pixel observations (agent.image) take the same route with the window kept on the DEVICE: the frames of the N rolling contexts live
in a ring [N][L][C H W] of uint8 and their embeddings in a second ring [N][L][d_model], so a vector step stages the N newest frames
only, and `dtqn_img_actor_forward_batch` encodes only the frames whose embedding is not current -- the N new ones while the policy
parameters stand still, every live one after they moved.  (run.py queues N updates behind every vector step and evaluates and
prepopulates through the single-environment actor, so there every step re-encodes; the reuse serves callers that drive a VectorActor
with frozen parameters or with fewer updates than steps.)  A vector step on which every environment explores only pushes its frames.  The host keeps
(slot of the newest frame, live rows, which embeddings are current) per environment and drops the last of these whenever the
parameters can have changed: an optimizer launch (TdEngine.updates), a host-side write to the flat buffer or to one of the
Parameters that view it (their torch `_version`: load_state_dict, a checkpoint restore, an in-place op), a re-bound buffer.  The target network has its own
buffer, so target_update does not touch them; embedding dropout acts behind the ring, so a change of train / eval mode does not either.

Attention capture (DTQN(..., capture_attention=True)) is not done here: the batched actor launch keeps no attention records, so the
policy network's `alpha` / `attn_weights` are those of its last module forward (DtqnAgent.get_action captures).
"""
from __future__ import annotations

import ctypes
from typing import List, Sequence

import numpy as np
import torch

from .. import _binding as B
from ..utils.bag import Bag
from ..utils.context import Context
from ..utils.random import RNG


class _FrameContext:
    """Host side of one image environment's rolling context: the step count.  The frames themselves are in the device ring (the frame
    of step t sits in slot t mod L) and, until the episode ends, in VectorActor.episodes."""

    def __init__(self, context_length: int):
        self.max_length, self.timestep = context_length, 0

    def reset(self, obs) -> None:
        self.timestep = 0

    def add_transition(self, o, a, r, done):
        self.timestep += 1
        return None, None


class VectorActor:
    def __init__(self, agent, envs: Sequence, ref_quirks: bool = False):
        self.agent, self.envs = agent, list(envs)
        N = self.n = len(self.envs)
        L, O, A = agent.context_len, agent.env_obs_length, agent.num_actions
        self.L, self.O, self.A = L, O, A
        self.image = getattr(agent, "image", None)
        self.episodes = [[] for _ in range(N)]            # per env: [first_obs, (obs, action, reward, done), ...]
        self.returns = np.zeros(N)
        self.steps = 0
        self.episodes_done = 0
        self.bags = None
        if self.image is not None:
            self._init_image()
            return
        self.contexts: List[Context] = [Context(L, agent.obs_mask, A, O, discrete=agent.is_discrete_env, ref_quirks=ref_quirks)
                                        for _ in range(N)]
        # bag networks: one bag per environment (utils/bag.py; dtqn.py:66-74 keeps one per agent because it steps one environment)
        self.bags = [Bag(agent.bag.size, agent.obs_mask, O, discrete=agent.is_discrete_env, ref_quirks=ref_quirks)
                     for _ in range(N)] if agent.bag.size > 0 else None
        cuda = agent.device.type == "cuda"
        obs_bytes = N * L * O * 4
        act_bytes = (N * L + 3) & ~3
        total = obs_bytes + act_bytes + 4 * N
        pin = (lambda t: t.pin_memory()) if cuda else (lambda t: t)
        self._ctx_h = pin(torch.zeros(total, dtype=torch.uint8))
        self._ctx_d = torch.zeros(total, dtype=torch.uint8, device=agent.device)
        buf = self._ctx_h.numpy()
        self._obs_np = buf[:obs_bytes].view(np.float32).reshape(N, L, O)
        self._act_np = buf[obs_bytes:obs_bytes + N * L].reshape(N, L)
        self._len_np = buf[obs_bytes + act_bytes:].view(np.int32)
        self._q_d = torch.zeros(N * L * A, device=agent.device)
        self._q_h = pin(torch.zeros(N, A))
        self._q_np = self._q_h.numpy()
        eng = agent.engine
        need = eng.lib.dtqn_forward_workspace_floats(eng._actor_net_ref, N)
        self._ws = torch.zeros(max(1, need), dtype=torch.float32, device=agent.device)
        self._ws_p = ctypes.c_void_p(self._ws.data_ptr()) if need > 0 else None
        self._p = [ctypes.c_void_p(t.data_ptr()) for t in (self._ctx_h, self._ctx_d, self._q_d, self._q_h)]
        self._ev = torch.cuda.Event() if cuda else None      # completion of the batched actor forward alone

    def _init_image(self) -> None:
        """Device rings, the pinned block of a vector step and the workspace of dtqn_img_actor_forward_batch (include/dtqn_hip.h)."""
        from ..image import ImageEncoder
        agent, N, L, A = self.agent, self.n, self.L, self.A
        if agent.bag.size > 0:
            raise NotImplementedError("vectorised rollout of image observations with a bag")
        for env in self.envs:
            # the block carries raw uint8 pixels (what the replay and the reference's context hold): asked once, here; staging a frame
            # of another dtype is refused by the copy itself
            dt = getattr(getattr(env, "observation_space", None), "dtype", None)
            if dt is not None and np.dtype(dt) != np.uint8:
                raise TypeError(f"image observations must be uint8 pixels, the environment declares {np.dtype(dt)}")
        eng = agent.engine
        lib, net_ref, dev = eng.lib, eng._actor_net_ref, agent.device
        cuda = dev.type == "cuda"
        O, D = int(np.prod(self.image)), int(eng.actor_net.d_model)
        stage_bytes, need = int(lib.dtqn_img_actor_stage_bytes(net_ref, N)), int(lib.dtqn_img_actor_workspace_floats(net_ref, N))
        if stage_bytes <= 0 or need <= 0:
            raise NotImplementedError("vectorised rollout of image observations: this network shape is not covered")
        pin = (lambda t: t.pin_memory()) if cuda else (lambda t: t)
        self.contexts = [_FrameContext(L) for _ in range(N)]
        self._stage_h = pin(torch.zeros(stage_bytes, dtype=torch.uint8))
        buf = self._stage_h.numpy()
        ints = buf[:stage_bytes - N * O].view(np.int32)
        self._head_np, self._len_np, self._fresh_np = ints[:N], ints[N:2 * N], ints[2 * N:3 * N]
        self._valid_np = ints[3 * N:3 * N + N * L].reshape(N, L)
        self._frames_np = buf[stage_bytes - N * O:].reshape(N, O)
        self._valid = np.zeros((N, L), dtype=np.int32)       # which embedding ring rows are current (the block gets a copy per step)
        self._pushed = np.full(N, -1, dtype=np.int64)        # step of the newest frame each environment has in the ring (-1: none)
        self._param_version = None
        self._prep_due = False                               # the encoder's transposed weights are older than the parameters
        self._params = list(agent.policy_network.parameters())
        self._frame_ring = torch.zeros(N * L * O, dtype=torch.uint8, device=dev)
        self._emb_ring = torch.zeros(N * L * D, dtype=torch.float32, device=dev)
        self._enc = ImageEncoder(lib, eng.actor_net, dev)    # the transposed weights, refreshed once per parameter version
        self._ws = torch.zeros(need, dtype=torch.float32, device=dev)
        self._q_d = torch.zeros(N * L * A, device=dev)
        self._q_h = pin(torch.zeros(N, A))
        self._q_np = self._q_h.numpy()
        self._p = [ctypes.c_void_p(t.data_ptr()) for t in (self._enc.wprep, self._stage_h, self._frame_ring, self._emb_ring, self._q_d,
                                                           self._q_h, self._ws)]
        self._ev = torch.cuda.Event() if cuda else None
        self._inflight = False

    # ------------------------------------------------------------------------------------------
    def reset_all(self) -> None:
        for i, env in enumerate(self.envs):
            self._reset(i)

    def _reset(self, i: int) -> None:
        obs = self.envs[i].reset()
        self.contexts[i].reset(obs)
        if self.bags is not None:
            self.bags[i].reset()
        self.episodes[i] = [np.array(obs, copy=True)]
        self.returns[i] = 0.0
        if self.image is not None:
            self._pushed[i] = -1
            self._valid[i] = 0

    def _launch_q_image(self, push_only: bool = False) -> None:
        """Stage the newest frame of every environment and launch the batched image actor forward (no synchronisation).
        push_only: a vector step on which every environment explores -- the frames go to the ring, nothing is encoded or forwarded
        (their embeddings stay marked as missing and are made by the next full launch)."""
        a, eng, L = self.agent, self.agent.engine, self.L
        if self._inflight and self._ev is not None:
            self._ev.synchronize()              # the kernels of the last launch read the pinned block in place
        # (a Parameter that was re-pointed at a moved flat buffer keeps a version counter of its own: both are asked)
        version = (eng.updates, eng.theta_pol._version, eng.theta_pol.data_ptr(), sum(p._version for p in self._params))
        refresh = version != self._param_version
        if refresh:
            self._valid[:] = 0
            self._param_version = version
        for i, ctx in enumerate(self.contexts):
            t = ctx.timestep
            n, head = min(L, t + 1), t % L
            fresh = 0
            if self._pushed[i] != t:
                if self._pushed[i] != t - 1:
                    raise RuntimeError("the context moved by more than one frame since the last actor launch")
                last = self.episodes[i][-1]
                np.copyto(self._frames_np[i], (last if isinstance(last, np.ndarray) else last[0]).reshape(-1), casting="no")
                self._valid[i, head] = 0
                self._pushed[i] = t
                fresh = 1
            self._head_np[i], self._len_np[i], self._fresh_np[i] = head, n, fresh
        self._valid_np[:] = self._valid
        p = self._p
        if push_only:
            self._prep_due = self._prep_due or refresh
            rc = eng.lib.dtqn_img_actor_forward_batch(eng._actor_net_ref, None, None, 0, p[1], p[2], None, self.n, None, None, None, 0, 0, 0, eng._stream())
        else:
            a._actor_calls += 1
            rc = eng.lib.dtqn_img_actor_forward_batch(eng._actor_net_ref, a._theta_p, p[0], 1 if (refresh or self._prep_due) else 0, p[1], p[2], p[3],
                                                      self.n, p[4], p[5], p[6], 1 if a.train_mode.name == "TRAIN" else 0,
                                                      eng.td.dropout_seed ^ 0xAC70, a._actor_calls & 0xFFFFFFFF, eng._stream())
        if rc != 0:
            raise RuntimeError(f"dtqn_img_actor_forward_batch failed with DTQN status {rc}")
        if not push_only:
            self._prep_due = False
            for i, ctx in enumerate(self.contexts):        # behind this launch every live row holds a current embedding
                self._valid[i, :min(L, ctx.timestep + 1)] = 1
        if self._ev is not None:
            self._ev.record(a._main_stream)
        self._inflight = True

    def _launch_q(self) -> None:
        """Stage all N contexts and launch the batched actor forward on the learner's stream (no synchronisation)."""
        a, eng = self.agent, self.agent.engine
        if self.image is not None:
            return self._launch_q_image()
        if self.bags is not None:
            # bag networks: the module forward with the N bags (dtqn_forward_bag); every sequence runs the longest prefix, the
            # rows behind a shorter one cannot reach its last live row (causal), its own bag attends row by row
            lens = [min(c.max_length, c.timestep + 1) for c in self.contexts]
            groups = [list(range(self.n))]
            if a.policy_network.net.action_dim > 0 and max(lens) > 1 and min(lens) == 1:
                # a ONE-row sequence keeps its action embedding un-rolled (dtqn.py:187-191: `if history_len > 1`); run next to longer
                # prefixes it would be rolled and zeroed, so the fresh episodes of this vector step get a forward of their own
                groups = [[i for i in range(self.n) if lens[i] > 1], [i for i in range(self.n) if lens[i] == 1]]
            q_rows = None
            for idx in groups:
                n_max = max(lens[i] for i in idx)
                obs = np.stack([self.contexts[i].obs[:n_max] for i in idx])
                act = np.stack([self.contexts[i].action[:n_max] for i in idx])
                q = a._bag_forward(obs, act, np.stack([self.bags[i].obss for i in idx]), np.stack([self.bags[i].actions for i in idx]))
                rows = torch.as_tensor(np.asarray([lens[i] for i in idx]) - 1, device=q.device)
                last = q[torch.arange(len(idx), device=q.device), rows]           # the last live row of every sequence
                if q_rows is None:
                    q_rows = torch.empty(self.n, self.A, dtype=q.dtype, device=q.device)
                q_rows[torch.as_tensor(idx, device=q.device)] = last
            # -> pinned memory with one asynchronous copy, and an event right behind it: updates queued after this point
            # (step_all's `between`) no longer stand between the host and its Q-values
            if self._ev is not None:
                self._q_h.copy_(q_rows, non_blocking=True)
                self._ev.record(torch.cuda.current_stream(a.device))
            else:
                self._q_h.copy_(q_rows)
            return
        n_max = 1
        for i, ctx in enumerate(self.contexts):
            n = min(ctx.max_length, ctx.timestep + 1)
            self._obs_np[i, :n] = ctx.obs[:n]
            self._act_np[i, :n] = ctx.action[:n, 0]
            self._len_np[i] = n
            n_max = max(n_max, n)
        a._actor_calls += 1
        rc = eng.lib.dtqn_actor_forward_batch(eng._actor_net_ref, a._theta_p, self._p[0], self._p[1], self.n, n_max, self._p[2], self._p[3],
                                              self._ws_p, 1 if a.train_mode.name == "TRAIN" else 0, eng.td.dropout_seed ^ 0xAC70, a._actor_calls & 0xFFFFFFFF, eng._stream())
        if rc == B.DEFINES["DTQN_ERR_ARG"]:
            raise AssertionError("Cannot forward, history is longer than expected.")   # dtqn.py:170-173
        if rc != 0:
            raise RuntimeError(f"dtqn_actor_forward_batch failed with DTQN status {rc}")
        if self._ev is not None:
            self._ev.record(a._main_stream)

    def _wait_q(self) -> np.ndarray:
        if self._ev is not None:
            self._ev.synchronize()              # the forward only: work queued behind it (TD updates) keeps running
        self._inflight = False
        return self._q_np

    def q_values(self) -> np.ndarray:
        """Q[:, -1] of every actor's current context: one launch, [N][A] (pinned host view; valid until the next call)."""
        self._launch_q()
        return self._wait_q()

    def act(self, epsilon: float, between=None) -> np.ndarray:
        """Epsilon-greedy actions for all N environments (dtqn.py:76-107 per actor; draws from RNG.rng in env order).
        between(): called after the actor forward has been launched and before its result is awaited -- the place to
        queue GPU work that may run while the host steps the environments."""
        explore = RNG.rng.random(self.n) < epsilon
        actions = np.zeros(self.n, dtype=np.int64)
        greedy = not explore.all()
        if greedy:
            self._launch_q()
        elif self.image is not None:               # image contexts live in the device ring: this step's frames go there, nothing else runs
            self._launch_q_image(push_only=True)
        if between is not None:
            between()
        if greedy:
            actions[:] = np.argmax(self._wait_q(), axis=1)            # first max, like torch.argmax
        if explore.any():
            actions[explore] = RNG.rng.integers(self.A, size=int(explore.sum()))
        return actions

    def step_all(self, epsilon: float, updates: int = 0) -> int:
        """One vector step: act, step every environment, record; finished episodes are replayed into the buffer and their
        environments reset.  updates > 0: that many agent.train() calls are QUEUED right behind the actor forward, so the
        GPU runs them while the host steps the N environments (the actions of this vector step come from the parameters
        before those updates, exactly as when train() is called after the step).  Returns the number of finished episodes."""
        agent = self.agent

        def queue_updates():
            for _ in range(updates):
                agent.train()
        actions = self.act(epsilon, queue_updates if updates > 0 else None)
        done_count = 0
        for i, env in enumerate(self.envs):
            a = int(actions[i])
            obs, reward, done, info = env.step(a)
            stored_done = False if info.get("TimeLimit.truncated", False) else done     # run.py:368-376
            evicted_obs, evicted_action = self.contexts[i].add_transition(obs, a, reward, stored_done)
            if self.bags is not None and evicted_obs is not None:
                agent._bag_insert(self.bags[i], self.contexts[i], evicted_obs, evicted_action)
            self.episodes[i].append((np.array(obs, copy=True), a, float(reward), bool(stored_done)))
            self.returns[i] += reward
            if done:
                self._commit_episode(i)
                self._reset(i)
                done_count += 1
        self.steps += self.n
        self.episodes_done += done_count
        return done_count

    def _commit_episode(self, i: int) -> None:
        rb = self.agent.replay_buffer
        ep = self.episodes[i]
        rb.store_obs(ep[0])
        for t, (obs, a, r, d) in enumerate(ep[1:]):
            rb.store(obs, a, r, d, t + 1)
        rb.flush()
