"""Device environments, host side: what `DeviceVectorActor` (device_rollout.py) and `DeviceEvaluator` (device_eval.py) have in common.

Both keep N CarFlag, Memory or tabular POMDP environments and their rolling contexts in one device allocation and step them behind
the batched actor forward (csrc/dtqn_devenv.hpp is the kernel side of this file).  `DeviceEnvs` owns what is the same: the host twin
of the environment and its kind, the refusals, the Q / workspace / pinned status buffers, the environment fields of the descriptor
(`DtqnRollout` and `DtqnEval` name them alike), the state allocation, the event ring that bounds the host's run-ahead, the decoding of
a status snapshot into counters, the views of the common state sections and get_state / set_state / q_rows.  A subclass keeps its
protocol and names its entry points and sections through the class attributes below."""
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
ENV_INTS, LAST_INTS = B.DEFINES["DTQN_DEVENV_STATE_INTS"], B.DEFINES["DTQN_DEVENV_LAST_INTS"]

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


class DeviceEnvs:
    RUN_AHEAD = 8                  # vector steps the host may be in front of the device
    # what a subclass states about itself:
    WHAT, FLAG, COVERAGE = "", "", ""              # "rollout", the run.py switch of the host path, what a DTQN_ERR_CONFIG names
    ENTRY, DESC = "", None                         # prefix of its entry points (dtqn_rollout / dtqn_deval), its descriptor type
    COUNTERS, RETURN_SUM = (), 0                   # names of the status record's counters; which one is the f64 return sum
    LAST_SECTION, BLOCK_SECTION = 0, 0             # state sections of the `last` record and of actor block 0 (block 1 follows)
    BAGS = False                                   # a subclass that keeps the bags on the device (device_bag.py) says True

    def __init__(self, agent, env_id: str, n_envs: int, seed: int, max_episode_steps: Optional[int], num_pairs: Optional[int]):
        what = self.WHAT
        env, kind = make_device_env(env_id, max_episode_steps, f"{what} (use {self.FLAG} otherwise)")
        if getattr(agent, "image", None) is not None:
            raise NotImplementedError(f"device-resident {what}: image networks are not covered (use {self.FLAG})")
        if agent.bag.size > 0 and not self.BAGS:
            raise NotImplementedError(f"device-resident {what}: bag networks are not covered by this class (use {self.FLAG}, or the bag "
                                      f"classes: --device-envs with --bag-size / --device-bag-eval-envs)")
        if agent.dp is not None or ddp.is_distributed():
            raise NotImplementedError(f"device-resident {what}: data-parallel runs are not covered")
        self._refuse(agent)
        if n_envs < 1:
            raise ValueError(f"device-resident {what} needs at least one environment")
        self.agent, self.env_id, self.n, self.seed = agent, env_id, int(n_envs), int(seed) & 0xFFFFFFFF
        self.L, self.O, self.A = agent.context_len, int(agent.env_obs_length), agent.num_actions
        self.kind = kind
        self.cap = int(max_episode_steps if max_episode_steps is not None else env._max_episode_steps)
        self.pairs = int(num_pairs if num_pairs is not None else getattr(env, "num_pairs", 0))
        if kind == B.DEFINES["DTQN_ROLLOUT_POMDP"]:
            self.env = env                               # the host twin: its model is what the device steps

    def _refuse(self, agent) -> None:
        """A subclass's own refusals, raised before the environment count is looked at."""

    def _make_descriptor(self):
        """The Q / workspace / pinned status buffers and a descriptor with its common fields -> the descriptor (`self._desc_ref` points
        at it); the subclass adds its own fields and calls _alloc_state."""
        eng, dev = self.agent.engine, self.agent.device
        cuda = dev.type == "cuda"
        self._pin = (lambda t: t.pin_memory()) if cuda else (lambda t: t)
        N, L, A = self.n, self.L, self.A
        words = 2 * len(self.COUNTERS)
        self._q_last = torch.zeros(N * A, device=dev)
        self._q_d = torch.zeros(N * L * A, device=dev)
        need = eng.lib.dtqn_forward_workspace_floats(eng._actor_net_ref, N)
        self._ws = torch.zeros(max(1, need), dtype=torch.float32, device=dev)
        self._status_h = self._pin(torch.zeros(words * 8, dtype=torch.uint8))
        self._status_np = self._status_h.numpy().view(np.uint32).reshape(words, 2)       # {word, tag} per granule
        d = self.DESC()
        d.status_host = self._status_h.data_ptr()
        d.q_last, d.q_dev, d.workspace = self._q_last.data_ptr(), self._q_d.data_ptr(), (self._ws.data_ptr() if need > 0 else None)
        d.env_kind, d.n_envs, d.max_episode_steps, d.num_pairs, d.seed = self.kind, N, self.cap, self.pairs, self.seed
        if self.kind == B.DEFINES["DTQN_ROLLOUT_POMDP"]:
            self._tables = upload_pomdp_tables(eng.lib, d, self.env, dev)
        self._desc_ref = ctypes.byref(d)
        self._cur = 0              # the block that holds the contexts
        self._issued = 0           # vector steps enqueued since construction (event ring)
        self._seen = dict.fromkeys(self.COUNTERS, 0)
        self._events = [torch.cuda.Event() for _ in range(self.RUN_AHEAD)] if cuda else None
        return d

    def _alloc_state(self, desc) -> None:
        """The one state allocation (and its pinned host copy) of the size `<ENTRY>_state_bytes` states for the finished descriptor."""
        lib, *args = self._lib_args()
        offsets = (ctypes.c_int32 * B.DEFINES[f"{self.ENTRY.upper()}_OFFSETS"])()
        nbytes = int(getattr(lib, f"{self.ENTRY}_state_bytes")(*args, self._desc_ref, offsets))
        if nbytes <= 0:
            raise ValueError(f"{self.ENTRY}_state_bytes refused this shape")
        self._offsets, self._nbytes = list(offsets), nbytes
        self._state = torch.zeros(nbytes, dtype=torch.uint8, device=self.agent.device)
        self._state_h = self._pin(torch.zeros(nbytes, dtype=torch.uint8))
        desc.state = self._state.data_ptr()

    # ------------------------------------------------------------------------------------------
    @classmethod
    def _check(cls, rc: int, what: str) -> None:
        if rc == B.DEFINES["DTQN_ERR_CONFIG"]:
            raise NotImplementedError(f"{what}: this {cls.COVERAGE} is outside the device-resident {cls.WHAT}'s coverage")
        if rc != 0:
            raise RuntimeError(f"{what} failed with DTQN status {rc}")

    def _call(self, name: str, *more) -> None:
        """`<ENTRY>_<name>(net, [replay,] descriptor, *more, stream)`, checked."""
        lib, *args = self._lib_args()
        fn = f"{self.ENTRY}_{name}"
        self._check(getattr(lib, fn)(*args, self._desc_ref, *more, self.agent.engine._stream()), fn)

    def _sync(self) -> None:
        if self.agent.device.type == "cuda":
            self.agent._main_stream.synchronize()

    def _throttle(self) -> None:
        """Never more than RUN_AHEAD vector steps in front of the device: before a step is enqueued, wait for the one issued RUN_AHEAD
        steps ago (its status record is then in pinned memory)."""
        if self._events is not None and self._issued >= len(self._events):       # (the emulation runs every launch to completion)
            self._events[self._issued % len(self._events)].synchronize()

    def _issue(self) -> None:
        """A vector step has been enqueued: its event, the other block."""
        if self._events is not None:
            self._events[self._issued % len(self._events)].record(self.agent._main_stream)
        self._issued += 1
        self._cur ^= 1

    def _poll(self, order: str, tag_hi: Optional[int] = None) -> dict:
        """The newest complete status record (no blocking) -> counters: every granule carries the tag of one launch (and that tag's
        high half is `tag_hi`, where given); a record older than the one already seen (by counter `order`) is ignored."""
        snap = self._status_np.copy()
        tags = snap[:, 1]
        if tags[0] != 0 and (tags == tags[0]).all() and (tag_hi is None or int(tags[0]) >> 16 == tag_hi):
            words = snap[:, 0].astype(np.uint64)
            vals = (words[0::2] | (words[1::2] << np.uint64(32))).astype(np.uint64)
            got = {k: int(v) for j, (k, v) in enumerate(zip(self.COUNTERS, vals.view(np.int64))) if j != self.RETURN_SUM}
            got[self.COUNTERS[self.RETURN_SUM]] = float(vals.view(np.float64)[self.RETURN_SUM])
            if got[order] >= self._seen[order]:
                self._seen = got
        return dict(self._seen)

    # ---- state access (tests, sync) -----------------------------------------------------------------
    def _section(self, raw: np.ndarray, k: int, nbytes: int, dtype) -> np.ndarray:
        return raw[self._offsets[k]:self._offsets[k] + nbytes].view(dtype)

    def _views(self, raw: np.ndarray, **own) -> SimpleNamespace:
        """Named numpy views of a host copy of the state: the common sections, the two actor blocks and the subclass's `own`."""
        N, L, O = self.n, self.L, self.O
        blocks = []
        for k in (self.BLOCK_SECTION, self.BLOCK_SECTION + 1):
            obs_b, act_b = N * L * O * 4, (N * L + 3) & ~3
            base = self._offsets[k]
            blocks.append(SimpleNamespace(obs=raw[base:base + obs_b].view(np.float32).reshape(N, L, O),
                                          actions=raw[base + obs_b:base + obs_b + N * L].reshape(N, L),
                                          lens=raw[base + obs_b + act_b:base + obs_b + act_b + 4 * N].view(np.int32)))
        last = self._section(raw, self.LAST_SECTION, 4 * N * LAST_INTS, np.int32).reshape(N, LAST_INTS)
        return SimpleNamespace(
            raw=raw, counters=self._section(raw, 0, 8 * len(self.COUNTERS), np.int64),
            env_f64=self._section(raw, 1, 32 * N, np.float64).reshape(N, 4),
            env_i32=self._section(raw, 2, 4 * N * ENV_INTS, np.int32).reshape(N, ENV_INTS), elapsed=self._section(raw, 3, 4 * N, np.int32),
            ep_ret=self._section(raw, 4, 8 * N, np.float64), last=last, reward=last[:, 7].view(np.float32), blocks=blocks,
            block=blocks[self._cur], **own)

    def get_state(self) -> SimpleNamespace:
        """A host copy of the whole device state as named numpy views (include/dtqn_hip.h lists the sections); `block` is the context
        block the next step reads.  Memory: env_i32[i] = current card | hidden values | shown table.  POMDP: env_i32[i] = state |
        observation, env_f64[i] = the recorded uniforms (u_state, u_obs of the last step | of the reset that started the episode)."""
        self._call("get_state", _ptr(self._state_h))
        self._sync()
        return self._views(self._state_h.numpy().copy())

    def set_state(self, state: SimpleNamespace) -> None:
        """Write a state obtained from get_state (and edited in place) back to the device."""
        self._state_h.numpy()[:] = state.raw
        self._note_state(state)                          # n_max must go on bounding every live-row count
        self._call("set_state", _ptr(self._state_h))
        self._sync()

    def q_rows(self) -> np.ndarray:
        """Tests: the Q rows the last step's actions were taken from, [N][A] (the lengths are those of the block that step read)."""
        N, A = self.n, self.A
        if not self.agent.engine.actor_net.tiled:
            return self._q_last.cpu().numpy().reshape(N, A).copy()
        st = self.get_state()
        n_max = self._last_n_max()
        lens = st.blocks[self._cur ^ 1].lens
        q = self._q_d.cpu().numpy()[:N * n_max * A].reshape(N, n_max, A)
        return np.stack([q[i, lens[i] - 1] for i in range(N)])
