"""Vectorised rollout: N host environments per learner, ONE batched actor launch per vector step.

The reference steps one environment per network forward (run.py:356-377); at 1 env step : 1 update the actor forward
and the Python env step sit on the critical path of every update.  `VectorActor` keeps N environments, acts for all of them
with one launch per vector step and reads the N Q-rows back from pinned memory; `VectorEvaluator` plays greedy evaluation
episodes the same way.  Both are loops over one back-end (`_Backend`), chosen once by the kind of observation.

Replay semantics stay the reference's: an episode becomes sampleable when it has FINISHED (replay_buffer.py:141-145
excludes the slot in progress).  With N episodes in progress at once, each environment collects its episode on the
host and replays it into the buffer's producer API (store_obs, store x len, flush) when it ends, so the device arrays
hold exactly what the single-environment loop would have written for that episode.

Flat observations (`_FlatBackend`): all N prefixes are staged through one pinned block (`actor_block`) and run by
`dtqn_actor_forward_batch` (ragged prefixes in one launch: every sequence runs max n_i rows, causality keeps shorter prefixes
exact); greedy evaluation runs `dtqn_actor_greedy_batch` on the same block, an idle environment staged with length 0.

Bag networks (`_BagBackend`): one bag per environment (utils/bag.py; dtqn.py:66-74 keeps one per agent because it steps one
environment) and the module forward through `agent._bag_forward`, in an evaluation over the environments that still play.

Pixel observations (`_ImageBackend`, agent.image) take the flat route with the window kept on the DEVICE: the frames of the N rolling
contexts live in a ring [N][L][C H W] of uint8 and their embeddings in a second ring [N][L][d_model], so a vector step stages the N
newest frames only, and `dtqn_img_actor_forward_batch` encodes only the frames whose embedding is not current -- the N new ones while
the policy parameters stand still, every live one after they moved.  (run.py queues N updates behind every vector step and
prepopulates through the single-environment actor, so there every step re-encodes; the reuse serves callers with frozen parameters
-- `VectorEvaluator`, what `run.py --eval-envs N` evaluates through -- or with fewer updates than steps.)  A vector step on which
every environment explores only pushes its frames.  The host keeps (slot of the newest frame, live rows, which embeddings are
current) per environment and drops the last of these whenever the parameters can have changed: an optimizer launch
(TdEngine.updates), a host-side write to the flat buffer or to one of the Parameters that view it (their torch `_version`:
load_state_dict, a checkpoint restore, an in-place op), a re-bound buffer.  The target network has its own buffer, so
target_update does not touch them; embedding dropout acts behind the ring, so a change of train / eval mode does not either.

Attention capture (DTQN(..., capture_attention=True)) is not done here: the batched actor launch keeps no attention records, so the
policy network's `alpha` / `attn_weights` are those of its last module forward (DtqnAgent.get_action captures).
"""
from __future__ import annotations

import contextlib
import ctypes
from types import SimpleNamespace
from typing import Sequence

import numpy as np
import torch

from .. import _binding as B
from ..utils.bag import Bag
from ..utils.context import Context
from ..utils.random import RNG
from .dtqn import _live_rows


def actor_block(N: int, L: int, O: int, alloc):
    """The packed block of the batched actor entry points (ActorBlock in csrc/dtqn_actor.hpp): [N][L O] f32 observations |
    [N][L] u8 actions, padded to 4 bytes | [N] i32 live rows.  alloc(bytes) -> the zeroed uint8 host tensor that holds it (the size
    is known here alone).  -> (bytes, that tensor, obs view, action view, length view)."""
    obs_bytes, act_bytes = N * L * O * 4, (N * L + 3) & ~3
    total = obs_bytes + act_bytes + 4 * N
    t = alloc(total)
    buf = t.numpy()
    return (total, t, buf[:obs_bytes].view(np.float32).reshape(N, L, O), buf[obs_bytes:obs_bytes + N * L].reshape(N, L),
            buf[obs_bytes + act_bytes:].view(np.int32))


_ptr = lambda t: ctypes.c_void_p(t.data_ptr())


class _Backend:
    """A back-end owns the N rolling contexts, its pinned and device buffers, its event and its per-environment bookkeeping:
    reset(i, obs), add_transition(i, obs, a, r, done) -> evicted (obs, action) or (None, None), timestep(i);
    launch(live=None, greedy=False, push_only=False) stages and launches without synchronisation (live: None = every environment, or
    a bool mask with False = idle; the network's mode is the agent's); wait() -> (the pinned [N][A] Q view, the pinned [N] int
    actions of the last greedy launch, -1 for an idle environment); parameters_frozen(): they stand still from here on."""
    bags = None

    def __init__(self, actor, contexts):
        agent = self.agent = actor.agent
        self.eng, self.n, self.L, self.A = agent.engine, actor.n, actor.L, actor.A
        cuda = agent.device.type == "cuda"
        self._pin = (lambda t: t.pin_memory()) if cuda else (lambda t: t)
        self._q_h = self._pin(torch.zeros(self.n, self.A))
        self._q_np = self._q_h.numpy()
        self._greedy_h = self._pin(torch.full((self.n,), -1, dtype=torch.int32))       # the actions of a greedy launch
        self._greedy_np = self._greedy_h.numpy()
        self._ev = torch.cuda.Event() if cuda else None      # completion of the batched actor forward alone
        self._inflight = False
        self.contexts = contexts

    def reset(self, i: int, obs) -> None:
        self.contexts[i].reset(obs)

    def add_transition(self, i: int, obs, a: int, r: float, done: bool):
        return self.contexts[i].add_transition(obs, a, r, done)

    def timestep(self, i: int) -> int:
        return self.contexts[i].timestep

    def wait(self):
        if self._ev is not None:
            self._ev.synchronize()              # the forward only: work queued behind it (TD updates) keeps running
        self._inflight = False
        return self._q_np, self._greedy_np

    def parameters_frozen(self) -> None:
        pass


def _host_contexts(actor, ref_quirks: bool):
    return [Context(actor.L, actor.agent.obs_mask, actor.A, actor.O, discrete=actor.agent.is_discrete_env, ref_quirks=ref_quirks)
            for _ in range(actor.n)]


class _FlatBackend(_Backend):
    def __init__(self, actor, ref_quirks: bool):
        super().__init__(actor, _host_contexts(actor, ref_quirks))
        N, L, A, dev, eng = self.n, self.L, self.A, self.agent.device, self.eng
        total, self._ctx_h, self._obs_np, self._act_np, self._len_np = actor_block(
            N, L, actor.O, lambda nbytes: self._pin(torch.zeros(nbytes, dtype=torch.uint8)))
        self._ctx_d = torch.zeros(total, dtype=torch.uint8, device=dev)
        self._q_d = torch.zeros(N * L * A, device=dev)
        need = eng.lib.dtqn_forward_workspace_floats(eng._actor_net_ref, N)
        self._ws = torch.zeros(max(1, need), dtype=torch.float32, device=dev)
        self._ctx_hp, self._ctx_dp, self._q_dp, self._q_hp, self._greedy_p = map(_ptr, (self._ctx_h, self._ctx_d, self._q_d, self._q_h,
                                                                                       self._greedy_h))
        self._ws_p = _ptr(self._ws) if need > 0 else None

    def launch(self, live=None, greedy: bool = False, push_only: bool = False) -> None:
        """Stage the live contexts and launch the batched actor forward on the learner's stream."""
        if push_only:                           # the contexts live on the host: nothing to bring to the device
            return
        a, eng = self.agent, self.eng
        n_max = 0
        for i, ctx in enumerate(self.contexts):
            n = _live_rows(ctx) if live is None or live[i] else 0
            if n > 0:
                self._obs_np[i, :n] = ctx.obs[:n]
                self._act_np[i, :n] = ctx.action[:n, 0]
            self._len_np[i] = n
            n_max = max(n_max, n)
        if greedy:
            rc = eng.lib.dtqn_actor_greedy_batch(eng._actor_net_ref, a._theta_p, self._ctx_hp, self._ctx_dp, self.n, n_max, self._q_dp, self._q_hp,
                                                 self._greedy_p, self._ws_p, 0, 0, 0, eng._stream())
        else:
            seed, step = a._actor_drop_key()
            rc = eng.lib.dtqn_actor_forward_batch(eng._actor_net_ref, a._theta_p, self._ctx_hp, self._ctx_dp, self.n, n_max, self._q_dp, self._q_hp,
                                                  self._ws_p, 1 if a.train_mode.name == "TRAIN" else 0, seed, step & 0xFFFFFFFF, eng._stream())
        if rc == B.DEFINES["DTQN_ERR_ARG"]:
            raise AssertionError("Cannot forward, history is longer than expected.")   # dtqn.py:170-173
        if rc != 0:
            raise RuntimeError(f"dtqn_actor_{'greedy' if greedy else 'forward'}_batch failed with DTQN status {rc}")
        if self._ev is not None:
            self._ev.record(a._main_stream)


class _BagBackend(_Backend):
    def __init__(self, actor, ref_quirks: bool):
        super().__init__(actor, _host_contexts(actor, ref_quirks))
        self.bags = [Bag(self.agent.bag.size, self.agent.obs_mask, actor.O, discrete=self.agent.is_discrete_env, ref_quirks=ref_quirks)
                     for _ in range(self.n)]

    def reset(self, i: int, obs) -> None:
        super().reset(i, obs)
        self.bags[i].reset()

    def add_transition(self, i: int, obs, a: int, r: float, done: bool):
        ctx = self.contexts[i]
        evicted_obs, evicted_action = ctx.add_transition(obs, a, r, done)
        if evicted_obs is not None:
            self.agent._bag_insert(self.bags[i], ctx, evicted_obs, evicted_action)
        return evicted_obs, evicted_action

    def launch(self, live=None, greedy: bool = False, push_only: bool = False) -> None:
        """The module forward with the bags of the live environments (dtqn_forward_bag); every sequence runs the longest prefix, the
        rows behind a shorter one cannot reach its last live row (causal), its own bag attends row by row.  The Q rows of the idle
        environments come back as zeros."""
        if push_only:
            return
        a = self.agent
        envs = [i for i in range(self.n) if live is None or live[i]]
        self._greedy_envs = envs if greedy else None
        lens = {i: _live_rows(self.contexts[i]) for i in envs}
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

    def wait(self):
        q, actions = super().wait()
        if self._greedy_envs is not None:
            actions[:] = -1
            actions[self._greedy_envs] = np.argmax(q[self._greedy_envs], axis=1)          # first max, like torch.argmax
        return q, actions


class _ImageBackend(_Backend):
    """Host side of the N rolling image contexts (`contexts`): the step count of every environment (timestep) and its newest frame;
    the frames themselves are in the device ring (the frame of step t sits in slot t mod L).  It owns both rings, the pinned block of
    a vector step and the workspace of dtqn_img_actor_forward_batch (include/dtqn_hip.h)."""

    def __init__(self, actor):
        from ..image import ImageEncoder
        super().__init__(actor, [SimpleNamespace(max_length=actor.L, timestep=0, frame=None) for _ in range(actor.n)])
        agent, eng, N, L, A = self.agent, self.eng, self.n, self.L, self.A
        if agent.bag.size > 0:
            raise NotImplementedError("vectorised rollout of image observations with a bag")
        for env in actor.envs:
            # the block carries raw uint8 pixels (what the replay and the reference's context hold): asked once, here; staging a frame
            # of another dtype is refused by the copy itself
            dt = getattr(getattr(env, "observation_space", None), "dtype", None)
            if dt is not None and np.dtype(dt) != np.uint8:
                raise TypeError(f"image observations must be uint8 pixels, the environment declares {np.dtype(dt)}")
        lib, net_ref, dev = eng.lib, eng._actor_net_ref, agent.device
        O, D = int(np.prod(agent.image)), int(eng.actor_net.d_model)
        stage_bytes, need = int(lib.dtqn_img_actor_stage_bytes(net_ref, N)), int(lib.dtqn_img_actor_workspace_floats(net_ref, N))
        if stage_bytes <= 0 or need <= 0:
            raise NotImplementedError("vectorised rollout of image observations: this network shape is not covered")
        self._stage_h = self._pin(torch.zeros(stage_bytes, dtype=torch.uint8))
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
        self._wprep_p, self._stage_p, self._frames_p, self._embs_p, self._q_dp, self._q_hp, self._greedy_p, self._ws_p = map(
            _ptr, (self._enc.wprep, self._stage_h, self._frame_ring, self._emb_ring, self._q_d, self._q_h, self._greedy_h, self._ws))

    def reset(self, i: int, obs) -> None:
        self.contexts[i].timestep, self.contexts[i].frame = 0, obs
        self._pushed[i], self._valid[i] = -1, 0

    def add_transition(self, i: int, obs, a: int, r: float, done: bool):
        self.contexts[i].timestep += 1
        self.contexts[i].frame = obs
        return None, None

    def parameters_frozen(self) -> None:
        self._valid[:] = 0
        self._param_version = None         # the first launch refreshes the encoder's transposed weights

    def launch(self, live=None, greedy: bool = False, push_only: bool = False) -> None:
        """Fill the pinned block -- the newest frame of every live environment that has one the ring has not seen, window heads and
        lengths (idle: length 0), the valid marks -- and launch the batched image actor forward.
        push_only: a vector step on which every environment explores -- the frames go to the ring, nothing is encoded or forwarded
        (their embeddings stay marked as missing and are made by the next full launch)."""
        a, eng, lib = self.agent, self.eng, self.eng.lib
        if self._inflight and self._ev is not None:
            self._ev.synchronize()              # the kernels of the last launch read the pinned block in place
        # (a Parameter that was re-pointed at a moved flat buffer keeps a version counter of its own: both are asked)
        version = (eng.updates, eng.theta_pol._version, eng.theta_pol.data_ptr(), sum(p._version for p in self._params))
        refresh = version != self._param_version       # the parameters moved: all marks are dropped, the encoder's weights are due
        if refresh:
            self._valid[:] = 0
            self._param_version = version
        for i, ctx in enumerate(self.contexts):
            if live is not None and not live[i]:
                self._head_np[i], self._len_np[i], self._fresh_np[i] = 0, 0, 0
                continue
            t = ctx.timestep
            n, head = _live_rows(ctx), t % self.L
            fresh = 0
            if self._pushed[i] != t:
                if self._pushed[i] != t - 1:
                    raise RuntimeError("the context moved by more than one frame since the last actor launch")
                np.copyto(self._frames_np[i], ctx.frame.reshape(-1), casting="no")
                self._valid[i, head] = 0
                self._pushed[i] = t
                fresh = 1
            self._head_np[i], self._len_np[i], self._fresh_np[i] = head, n, fresh
        self._valid_np[:] = self._valid
        prep = 1 if (refresh or self._prep_due) else 0
        if push_only:
            self._prep_due = self._prep_due or refresh
            rc = lib.dtqn_img_actor_forward_batch(eng._actor_net_ref, None, None, 0, self._stage_p, self._frames_p, None, self.n, None, None, None,
                                                  0, 0, 0, eng._stream())
        elif greedy:
            rc = lib.dtqn_img_actor_greedy_batch(eng._actor_net_ref, a._theta_p, self._wprep_p, prep, self._stage_p, self._frames_p, self._embs_p,
                                                 self.n, self._q_dp, self._q_hp, self._greedy_p, self._ws_p, 0, 0, 0, eng._stream())
        else:
            seed, step = a._actor_drop_key()
            rc = lib.dtqn_img_actor_forward_batch(eng._actor_net_ref, a._theta_p, self._wprep_p, prep, self._stage_p, self._frames_p, self._embs_p,
                                                  self.n, self._q_dp, self._q_hp, self._ws_p, 1 if a.train_mode.name == "TRAIN" else 0,
                                                  seed, step & 0xFFFFFFFF, eng._stream())
        if rc != 0:
            raise RuntimeError(f"dtqn_img_actor_{'greedy' if greedy and not push_only else 'forward'}_batch failed with DTQN status {rc}")
        if not push_only:
            self._prep_due = False
            for i, n in enumerate(self._len_np):      # behind a full launch every live row (idle: none) holds a current embedding
                self._valid[i, :n] = 1
        if self._ev is not None:
            self._ev.record(a._main_stream)
        self._inflight = True


class VectorActor:
    def __init__(self, agent, envs: Sequence, ref_quirks: bool = False):
        self.agent, self.envs = agent, list(envs)
        N = self.n = len(self.envs)
        self.L, self.O, self.A = agent.context_len, agent.env_obs_length, agent.num_actions
        self.image = getattr(agent, "image", None)
        self.episodes = [[] for _ in range(N)]            # per env: [first_obs, (obs, action, reward, done), ...]
        self.returns = np.zeros(N)
        self.steps = 0
        self.episodes_done = 0
        if self.image is not None:
            self._be = _ImageBackend(self)             # (pixels are kept as they come: ref_quirks has nothing to change)
        else:
            self._be = (_BagBackend if agent.bag.size > 0 else _FlatBackend)(self, ref_quirks)
        self.contexts, self.bags = self._be.contexts, self._be.bags

    # ------------------------------------------------------------------------------------------
    def reset_all(self) -> None:
        for i, env in enumerate(self.envs):
            self._reset(i)

    def _reset(self, i: int) -> None:
        frame = np.array(self.envs[i].reset(), copy=True)
        self._be.reset(i, frame)
        self.episodes[i] = [frame]
        self.returns[i] = 0.0

    def q_values(self) -> np.ndarray:
        """Q[:, -1] of every actor's current context: one launch, [N][A] (pinned host view; valid until the next call)."""
        self._be.launch()
        return self._be.wait()[0]

    def act(self, epsilon: float, between=None) -> np.ndarray:
        """Epsilon-greedy actions for all N environments (dtqn.py:76-107 per actor; draws from RNG.rng in env order).
        between(): called after the actor forward has been launched and before its result is awaited -- the place to
        queue GPU work that may run while the host steps the environments."""
        explore = RNG.rng.random(self.n) < epsilon
        actions = np.zeros(self.n, dtype=np.int64)
        greedy = not explore.all()
        self._be.launch(push_only=not greedy)      # every environment explores: contexts kept on the device still take this step's frames
        if between is not None:
            between()
        if greedy:
            actions[:] = np.argmax(self._be.wait()[0], axis=1)            # first max, like torch.argmax
        if explore.any():
            actions[explore] = RNG.rng.integers(self.A, size=int(explore.sum()))
        return actions

    def _step_env(self, i: int, a: int, rollout: bool):
        """Step environment i with action a and record the transition -> (done, info).  rollout: the episode is collected for the
        replay, a time-limit truncation stored as not done (run.py:368-376); otherwise only its newest frame is kept."""
        obs, reward, done, info = self.envs[i].step(a)
        frame = np.array(obs, copy=True)
        if rollout:
            stored_done = False if info.get("TimeLimit.truncated", False) else done
            self.episodes[i].append((frame, a, float(reward), bool(stored_done)))
        else:
            stored_done = done
            self.episodes[i] = [frame]
        self._be.add_transition(i, frame, a, reward, stored_done)        # (a bag network's back-end takes what the context evicts)
        self.returns[i] += reward
        return done, info

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
        for i in range(self.n):
            if self._step_env(i, int(actions[i]), True)[0]:
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


for _name in ("_q_np", "_len_np", "_head_np", "_fresh_np", "_valid", "_pushed", "_frame_ring", "_emb_ring"):
    setattr(VectorActor, _name, property(lambda self, _n=_name: getattr(self._be, _n)))      # back-end state tests read, read-only


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
    if the parameter watch of the image back-end sees them move): every frame is encoded exactly once."""

    def __init__(self, agent, envs: Sequence, ref_quirks: bool = False):
        with _private_rng(0):
            super().__init__(agent, envs, ref_quirks=ref_quirks)
        self.live = np.zeros(self.n, dtype=bool)

    def _greedy_actions(self) -> np.ndarray:
        """The greedy action of every live environment (int per environment; -1 for an idle one): one launch, awaited."""
        self._be.launch(self.live, greedy=True)
        return self._be.wait()[1]

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
        self._be.parameters_frozen()
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
                done, info = self._step_env(i, int(actions[i]), False)
                if done:
                    ret = float(self.returns[i])
                    results[episode[i]] = (ret, self._be.timestep(i), int(info.get("is_success", False) or ret > 0))
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
