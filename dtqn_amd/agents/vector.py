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
parameters stand still, every live one after they moved.  (run.py queues N updates behind every vector step and prepopulates through the
single-environment actor, so there every step re-encodes; the reuse serves callers with frozen parameters -- `VectorEvaluator` below, what
`run.py --eval-envs N` evaluates through -- or with fewer updates than steps.)  A vector step on which every environment explores only pushes its frames.  The host keeps
(slot of the newest frame, live rows, which embeddings are current) per environment and drops the last of these whenever the
parameters can have changed: an optimizer launch (TdEngine.updates), a host-side write to the flat buffer or to one of the
Parameters that view it (their torch `_version`: load_state_dict, a checkpoint restore, an in-place op), a re-bound buffer.  The target network has its own
buffer, so target_update does not touch them; embedding dropout acts behind the ring, so a change of train / eval mode does not either.

Attention capture (DTQN(..., capture_attention=True)) is not done here: the batched actor launch keeps no attention records, so the
policy network's `alpha` / `attn_weights` are those of its last module forward (DtqnAgent.get_action captures).
"""
from __future__ import annotations

import contextlib
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
        a, eng = self.agent, self.agent.engine
        refresh = self._stage_image()
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
            self._image_launched()
        if self._ev is not None:
            self._ev.record(a._main_stream)
        self._inflight = True

    def _image_launched(self, live=None) -> None:
        """Behind a full launch every live row of every (live) environment holds a current embedding."""
        self._prep_due = False
        for i, ctx in enumerate(self.contexts):
            if live is None or live[i]:
                self._valid[i, :min(self.L, ctx.timestep + 1)] = 1

    def _stage_image(self, live=None) -> bool:
        """Fill the pinned block of an image launch: the newest frame of every environment that has one the ring has not seen, window
        heads and lengths, the valid marks.  live: per environment, False = idle (length 0: dtqn_img_actor_greedy_batch); None = all.
        Returns whether the parameters moved since the last launch (all marks were dropped, the encoder's weights are due)."""
        eng, L = self.agent.engine, self.L
        if self._inflight and self._ev is not None:
            self._ev.synchronize()              # the kernels of the last launch read the pinned block in place
        # (a Parameter that was re-pointed at a moved flat buffer keeps a version counter of its own: both are asked)
        version = (eng.updates, eng.theta_pol._version, eng.theta_pol.data_ptr(), sum(p._version for p in self._params))
        refresh = version != self._param_version
        if refresh:
            self._valid[:] = 0
            self._param_version = version
        for i, ctx in enumerate(self.contexts):
            if live is not None and not live[i]:
                self._head_np[i], self._len_np[i], self._fresh_np[i] = 0, 0, 0
                continue
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
        return refresh

    def _launch_q(self) -> None:
        """Stage all N contexts and launch the batched actor forward on the learner's stream (no synchronisation)."""
        a, eng = self.agent, self.agent.engine
        if self.image is not None:
            return self._launch_q_image()
        if self.bags is not None:
            return self._launch_q_bag(list(range(self.n)))
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

    def _launch_q_bag(self, envs: List[int]) -> None:
        """Bag networks: the module forward with the bags of `envs` (dtqn_forward_bag; all N in a rollout, the environments that still play
        in an evaluation); every sequence runs the longest prefix, the rows behind a shorter one cannot reach its last live row (causal),
        its own bag attends row by row.  The Q rows of the other environments come back as zeros."""
        a = self.agent
        lens = {i: min(self.contexts[i].max_length, self.contexts[i].timestep + 1) for i in envs}
        groups = [list(envs)]
        if a.policy_network.net.action_dim > 0 and max(lens.values()) > 1 and min(lens.values()) == 1:
            # a ONE-row sequence keeps its action embedding un-rolled (dtqn.py:187-191: `if history_len > 1`); run next to longer
            # prefixes it would be rolled and zeroed, so the fresh episodes of this vector step get a forward of their own
            groups = [[i for i in envs if lens[i] > 1], [i for i in envs if lens[i] == 1]]
        q_rows = None
        for idx in groups:
            n_max = max(lens[i] for i in idx)
            obs = np.stack([self.contexts[i].obs[:n_max] for i in idx])
            act = np.stack([self.contexts[i].action[:n_max] for i in idx])
            q = a._bag_forward(obs, act, np.stack([self.bags[i].obss for i in idx]), np.stack([self.bags[i].actions for i in idx]))
            rows = torch.as_tensor(np.asarray([lens[i] for i in idx]) - 1, device=q.device)
            last = q[torch.arange(len(idx), device=q.device), rows]           # the last live row of every sequence
            if q_rows is None:
                q_rows = (torch.empty if len(envs) == self.n else torch.zeros)(self.n, self.A, dtype=q.dtype, device=q.device)
            q_rows[torch.as_tensor(idx, device=q.device)] = last
        # -> pinned memory with one asynchronous copy, and an event right behind it: updates queued after this point
        # (step_all's `between`) no longer stand between the host and its Q-values
        if self._ev is not None:
            self._q_h.copy_(q_rows, non_blocking=True)
            self._ev.record(torch.cuda.current_stream(a.device))
        else:
            self._q_h.copy_(q_rows)

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


@contextlib.contextmanager
def _private_rng(seed: int):
    """RNG.rng replaced by a generator of the caller's own for the duration: what runs inside draws nothing from the global stream."""
    keep, RNG.rng = RNG.rng, np.random.Generator(np.random.PCG64(seed))
    try:
        yield
    finally:
        RNG.rng = keep


class VectorEvaluator(VectorActor):
    """Greedy evaluation (reference run.py:187-243) of N environments at once: one batched launch per vector step, the arg-max taken on
    the device (`dtqn_actor_greedy_batch`, `dtqn_img_actor_greedy_batch`; bag networks: the module forward over the environments that
    still play).  The evaluator owns its N environments and N contexts (and bags): the agent's train and eval contexts, its replay
    and `RNG.rng` are not touched, the network runs in eval mode (no dropout) as under `eval_on()`.

    `evaluate(episodes)` deals the episodes out in order -- environment i plays episodes i, i + N, ... -- and an environment with no
    episode left goes idle: it is staged with length 0, takes no sequence of the forward and, with pixel observations, pushes no frame.
    The parameters stand still for a whole evaluation, so the embedding ring's valid marks are dropped once at its start (and again only
    if the parameter watch of `VectorActor` sees them move): every frame is encoded exactly once."""

    def __init__(self, agent, envs: Sequence, ref_quirks: bool = False):
        with _private_rng(0):
            super().__init__(agent, envs, ref_quirks=ref_quirks)
        pin = (lambda t: t.pin_memory()) if agent.device.type == "cuda" else (lambda t: t)
        self._greedy_h = pin(torch.full((self.n,), -1, dtype=torch.int32))         # the actions, written by the greedy kernel
        self._greedy_np = self._greedy_h.numpy()
        self._greedy_p = ctypes.c_void_p(self._greedy_h.data_ptr())
        self.live = np.zeros(self.n, dtype=bool)

    def _greedy_actions(self) -> np.ndarray:
        """The greedy action of every live environment (int per environment; -1 for an idle one): one launch, awaited."""
        a, eng, live = self.agent, self.agent.engine, self.live
        if self.bags is not None:
            envs = [i for i in range(self.n) if live[i]]
            self._launch_q_bag(envs)
            q = self._wait_q()
            self._greedy_np[:] = -1
            self._greedy_np[envs] = np.argmax(q[envs], axis=1)          # first max, like torch.argmax
            return self._greedy_np
        if self.image is not None:
            refresh = self._stage_image(live)
            p = self._p
            rc = eng.lib.dtqn_img_actor_greedy_batch(eng._actor_net_ref, a._theta_p, p[0], 1 if (refresh or self._prep_due) else 0, p[1], p[2],
                                                     p[3], self.n, p[4], p[5], self._greedy_p, p[6], 0, 0, 0, eng._stream())
            if rc != 0:
                raise RuntimeError(f"dtqn_img_actor_greedy_batch failed with DTQN status {rc}")
            self._image_launched(live)
            self._inflight = True
        else:
            n_max = 0
            for i, ctx in enumerate(self.contexts):
                n = min(ctx.max_length, ctx.timestep + 1) if live[i] else 0
                if n > 0:
                    self._obs_np[i, :n] = ctx.obs[:n]
                    self._act_np[i, :n] = ctx.action[:n, 0]
                self._len_np[i] = n
                n_max = max(n_max, n)
            rc = eng.lib.dtqn_actor_greedy_batch(eng._actor_net_ref, a._theta_p, self._p[0], self._p[1], self.n, n_max, self._p[2], self._p[3],
                                                 self._greedy_p, self._ws_p, 0, 0, 0, eng._stream())
            if rc == B.DEFINES["DTQN_ERR_ARG"]:
                raise AssertionError("Cannot forward, history is longer than expected.")   # dtqn.py:170-173
            if rc != 0:
                raise RuntimeError(f"dtqn_actor_greedy_batch failed with DTQN status {rc}")
        if self._ev is not None:
            self._ev.record(a._main_stream)
        self._wait_q()
        return self._greedy_np

    def _begin_episode(self, i: int, episode: int) -> None:
        # a context fills the action rows behind its prefix from RNG.rng (utils/context.py): here from a stream of the episode's own,
        # so the exploration stream stands still and an episode does not depend on which environment plays it
        with _private_rng(episode):
            self._reset(i)                 # environment, context, bag, ring marks; episodes[i] = [the first observation]
        self.live[i] = True

    @torch.no_grad()
    def evaluate(self, episodes: int):
        """(success rate, mean return, mean episode length) over `episodes` greedy episodes, by the formulas of run.evaluate: success
        is info["is_success"] or a positive return, the length is the context's timestep when the episode ends."""
        agent, N = self.agent, self.n
        agent.eval_on()
        if self.image is not None:
            self._valid[:] = 0
            self._param_version = None     # the first launch refreshes the encoder's transposed weights
        episode = np.full(N, -1, dtype=np.int64)          # the episode each environment is playing
        results = [None] * episodes                       # (return, length, success) in episode order
        self.live[:] = False
        for i in range(min(N, episodes)):
            episode[i] = i
            self._begin_episode(i, i)
        while self.live.any():
            actions = self._greedy_actions()
            for i in range(N):
                if not self.live[i]:
                    continue
                act = int(actions[i])
                obs, reward, done, info = self.envs[i].step(act)
                evicted_obs, evicted_action = self.contexts[i].add_transition(obs, act, reward, done)
                if self.bags is not None and evicted_obs is not None:
                    agent._bag_insert(self.bags[i], self.contexts[i], evicted_obs, evicted_action)
                self.episodes[i] = [np.array(obs, copy=True)]         # the newest frame (what the image staging reads)
                self.returns[i] += reward
                if done:
                    ret = float(self.returns[i])
                    results[episode[i]] = (ret, self.contexts[i].timestep, int(info.get("is_success", False) or ret > 0))
                    episode[i] += N
                    if episode[i] < episodes:
                        self._begin_episode(i, int(episode[i]))
                    else:
                        self.live[i] = False
        agent.eval_off()
        n = max(episodes, 1)
        returns = successes = steps = 0
        for ret, length, ok in results:
            returns += ret
            steps += length
            successes += ok
        return successes / n, returns / n, steps / n
