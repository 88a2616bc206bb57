"""DRQN baseline with the reference's constructor, forward signature and state_dict layout (dtqn/networks/drqn.py:9-66 on
dtqn/networks/dqn.py:8-52), backed by ONE flat fp32 buffer that the gfx950 LSTM kernels read directly (include/dtqn_hip.h, DrqnNet).

Like dtqn_amd.networks.DTQN the module is a parameter container plus a `forward`: every nn.Parameter is a view into `self.flat`, so
`state_dict()` / `load_state_dict()` / `parameters()` behave like the reference's and a state dict moves between the two
implementations.  Under grad mode the forward is a torch.autograd.Function whose backward is dtqn_drqn_backward; with and without a
graph Q is the same, bit for bit (the same kernels).  There is no eager fallback: the forward runs on the engine or raises.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _binding as B
from .. import engine
from .dtqn import _attach


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class DRQN(nn.Module):
    """Deep Recurrent Q-Network (https://arxiv.org/pdf/1507.06527.pdf).  Arguments as in the reference (drqn.py:12-22); `action_dim` is
    accepted and unused there too.  `context_len` (keyword, default 512) bounds the rows of one forward."""

    def __init__(self, obs_dim: int, num_actions: int, embed_per_obs_dim: int, action_dim: int, inner_embed: int,
                 is_discrete_env: bool, obs_vocab_size: Optional[int] = None, context_len: int = 512, _test_lib=None, **kwargs):
        super().__init__()
        self._lib = _test_lib if _test_lib is not None else engine.get_lib()
        self.obs_dim, self.num_actions, self.discrete, self.inner_embed = obs_dim, num_actions, bool(is_discrete_env), inner_embed
        self.net = B.make_drqn_net(self._lib, obs_dim=obs_dim, num_actions=num_actions, embed_per_obs_dim=embed_per_obs_dim,
                                   action_dim=action_dim, inner_embed=inner_embed, context_len=context_len, discrete=is_discrete_env,
                                   vocab_sizes=int(obs_vocab_size) if is_discrete_env else 0)
        self.flat = torch.zeros(self.net.n_theta, dtype=torch.float32)
        self._table = B.drqn_param_table(self.net)
        self._views = {}
        for key, (off, shape) in self._table.items():
            p = nn.Parameter(self.flat[off:off + int(np.prod(shape))].view(shape))
            self._views[key] = (p, off, shape)
            _attach(self, key, p)
        self._ws = None
        self.reset_parameters()

    @torch.no_grad()
    def reset_parameters(self) -> None:
        """DRQN.__init__ (drqn.py:33-36): nn.LSTM keeps torch's default U(-1 / sqrt(D), 1 / sqrt(D)) -- init_weights (utils/torch_utils.py)
        touches Linear and Embedding only: N(0, 0.02) weights, zero Linear biases."""
        bound = 1.0 / float(np.sqrt(self.inner_embed))
        for key, (p, off, shape) in self._views.items():
            if key.startswith("lstm."):
                p.uniform_(-bound, bound)
            elif key.endswith("bias"):
                p.zero_()
            else:
                p.normal_(mean=0.0, std=0.02)

    def _apply(self, fn, recurse=True):
        """Module.to()/cuda()/float(): move the flat buffer once and re-point every view at it."""
        super()._apply(fn, recurse)
        self.flat = fn(self.flat).contiguous()
        for key, (p, off, shape) in self._views.items():
            p.data = self.flat[off:off + int(np.prod(shape))].view(shape)
        self._ws = None
        return self

    def _grad_params(self):
        return [(p, off) for off, p in sorted((off, p) for (p, off, shape) in self._views.values())]

    def _stream(self, dev):
        return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None

    def _prepare(self, obss, hidden_states, episode_lengths):
        dev = self.flat.device
        if dev.type != "cuda" and not getattr(self, "_allow_cpu", False):
            raise engine.EngineUnavailable("DRQN.forward runs on the gfx950 engine only: move the module to a ROCm device")
        assert obss.dim() == 3 and obss.size(2) == self.obs_dim, f"Obs dim is incorrect. Expected {self.obs_dim} got {tuple(obss.shape[2:])}"
        Bn, n = int(obss.size(0)), int(obss.size(1))
        assert n <= self.net.ctx_len, "Cannot forward, the sequence is longer than the network's context"
        o = obss.detach().to(device=dev, dtype=torch.float32).contiguous()
        lens = h0 = c0 = None
        if hidden_states is not None:
            h0 = hidden_states[0].detach().to(device=dev, dtype=torch.float32).reshape(Bn, self.inner_embed).contiguous()
            c0 = hidden_states[1].detach().to(device=dev, dtype=torch.float32).reshape(Bn, self.inner_embed).contiguous()
        else:
            if episode_lengths is None:
                raise ValueError("DRQN.forward needs hidden_states (one observation at a time) or episode_lengths (a padded batch)")
            lens = np.ascontiguousarray(torch.as_tensor(episode_lengths).detach().cpu().numpy().reshape(-1), dtype=np.int32)
            if lens.shape[0] != Bn:
                raise ValueError(f"episode_lengths holds {lens.shape[0]} entries for a batch of {Bn}")
            if lens.min() < 1 or lens.max() > n:
                # pack_padded_sequence's own refusal (drqn.py:52-57)
                raise RuntimeError("Length of all samples has to be greater than 0 and at most the padded length, "
                                   f"but found an element in 'lengths' that is outside 1..{n}")
        return dev, Bn, n, o, lens, h0, c0

    def _run(self, o, lens, h0, c0, Bn, n, dev, train: bool, ws: Optional[torch.Tensor] = None):
        need = int(self._lib.dtqn_drqn_workspace_floats(ctypes.byref(self.net), Bn, n, 1 if train else 0))
        if need <= 0:
            raise RuntimeError("dtqn_drqn_workspace_floats: this call is not covered")
        if ws is None:
            if train:
                ws = torch.empty(need, dtype=torch.float32, device=dev)          # owned by this forward's graph
            else:
                if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
                    self._ws = None
                    self._ws = torch.empty(need, dtype=torch.float32, device=dev)
                ws = self._ws
        q = torch.empty((Bn, n, self.num_actions), dtype=torch.float32, device=dev)
        h = torch.empty((1, Bn, self.inner_embed), dtype=torch.float32, device=dev)
        c = torch.empty_like(h)
        lp = None if lens is None else lens.ctypes.data_as(ctypes.c_void_p)
        if train:
            rc = self._lib.dtqn_drqn_forward_train(ctypes.byref(self.net), _ptr(self.flat), _ptr(o), lp, Bn, n, _ptr(q), _ptr(h), _ptr(c), _ptr(ws),
                                                   self._stream(dev))
        else:
            rc = self._lib.dtqn_drqn_forward(ctypes.byref(self.net), _ptr(self.flat), _ptr(o), lp, _ptr(h0), _ptr(c0), Bn, n, _ptr(q), _ptr(h),
                                             _ptr(c), _ptr(ws), self._stream(dev))
        if rc != 0:
            raise RuntimeError(f"dtqn_drqn_forward{'_train' if train else ''} failed with DTQN status {rc}")
        return q, h, c, ws

    def forward(self, obss: torch.Tensor, actions: Optional[torch.Tensor] = None,
                hidden_states: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, episode_lengths=None):
        """obss [B, seq, obs_dim] (float, or integer tokens for discrete envs); `actions` is ignored, as in the reference.
        hidden_states (h, c), each [1, B, D]: every row is live and the state is carried in and out (acting, one observation at a time).
        Otherwise episode_lengths [B]: a padded batch; rows at or beyond a sequence's length have LSTM output 0 and the returned state
        is the one after the last live row.  Returns (Q [B, seq, A], (h, c)) with h, c [1, B, D].
        With grad mode on, a parameter that requires grad and no hidden_states, Q carries a graph whose backward is the HIP backward;
        h and c never do."""
        dev, Bn, n, o, lens, h0, c0 = self._prepare(obss, hidden_states, episode_lengths)
        params = self._grad_params()
        if torch.is_grad_enabled() and hidden_states is None and any(p.requires_grad for p, _ in params):
            runner = _DrqnRunner(self, o, lens, Bn, n, dev)
            q = _DrqnForward.apply(runner, *[p for p, _ in params])
            return q, (runner.h, runner.c)
        with torch.no_grad():
            q, h, c, _ = self._run(o, lens, h0, c0, Bn, n, dev, train=False)
        return q, (h, c)


class _DrqnRunner:
    """One differentiable forward: its inputs as the kernels read them and the record workspace it owns."""

    def __init__(self, module: DRQN, o, lens, Bn, n, dev):
        self.m, self.o, self.lens, self.Bn, self.n, self.dev = module, o, lens, Bn, n, dev
        self.ws = self.h = self.c = None

    def forward(self):
        q, self.h, self.c, self.ws = self.m._run(self.o, self.lens, None, None, self.Bn, self.n, self.dev, train=True)
        return q

    def backward(self, dq):
        m = self.m
        dq = dq.detach().to(device=self.dev, dtype=torch.float32).contiguous()
        grad = torch.empty(m.net.n_trainable, dtype=torch.float32, device=self.dev)
        rc = m._lib.dtqn_drqn_backward(ctypes.byref(m.net), _ptr(m.flat), _ptr(self.o), self.Bn, self.n, _ptr(dq), _ptr(self.ws), _ptr(grad),
                                       m._stream(self.dev))
        if rc != 0:
            raise RuntimeError(f"dtqn_drqn_backward failed with DTQN status {rc}")
        self.ws = None
        return grad


class _DrqnForward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, runner: _DrqnRunner, *params):
        ctx.runner = runner
        return runner.forward()

    @staticmethod
    @once_differentiable
    def backward(ctx, dq):
        runner = ctx.runner
        grad = runner.backward(dq)
        outs = [grad[off:off + p.numel()].view(p.shape) if ctx.needs_input_grad[1 + i] else None
                for i, (p, off) in enumerate(runner.m._grad_params())]
        return (None, *outs)
