"""DTQN network object with the reference's constructor, forward signature and state_dict layout
(dtqn/networks/dtqn.py:16-218), backed by ONE flat fp32 device buffer that the gfx950 kernels
read directly.

The module is a parameter CONTAINER plus a `forward`: every nn.Parameter is a view
into `self.flat` (layout: include/dtqn_hip.h, DtqnNet), so `state_dict()` / `load_state_dict()` /
`parameters()` behave like the reference's -- a policy / target `state_dict` saved by either implementation loads
in the other (the FULL training checkpoints do not: the reference pickles joblib / torch-optimizer objects, dtqn_amd
writes plain arrays) --, while the engine
sees a single contiguous theta.  DtqnAgent.train() does not go through autograd: it runs the fused HIP
update on these same buffers.  `DTQN(..., autograd=True)` makes `forward` differentiable for losses written in
torch (_DtqnForward: the HIP backward of dtqn_backward_dq behind a torch.autograd.Function; with `set_dropout_seed` a train-mode
module applies its dropout there too, dtqn_forward_train_drop / dtqn_backward_dq_drop).  `DTQN(..., capture_attention=True)`
leaves the attention weights on the module after every forward, as the reference does (`transformer_layers[i].alpha`, and
`attn_weights` with a bag: dtqn_attn_weights over the records of dtqn_forward_train).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Union

import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _binding as B
from .. import engine


class _Node(nn.Module):
    """Anonymous container used to reproduce the reference's dotted state_dict keys."""


class _Layers(_Node):
    """`transformer_layers`: indexable and sized like the reference's nn.Sequential (dtqn.py:120-131); children "0", "1", ..."""

    def _ordered(self):
        return [self._modules[k] for k in sorted(self._modules, key=int)]

    def __len__(self) -> int:
        return len(self._modules)

    def __iter__(self):
        return iter(self._ordered())

    def __getitem__(self, idx):
        return self._ordered()[idx]


def _attach(root: nn.Module, dotted: str, param: nn.Parameter) -> None:
    parts = dotted.split(".")
    mod = root
    for name in parts[:-1]:
        if name not in mod._modules:
            mod.add_module(name, _Layers() if (mod is root and name == "transformer_layers") else _Node())
        mod = mod._modules[name]
    mod.register_parameter(parts[-1], param)


def _img_check_every() -> int:
    import os
    try:
        return max(0, int(os.environ.get("DTQN_IMG_CHECK_EVERY", "64")))
    except ValueError:
        return 64


class DTQN(nn.Module):
    """Deep Transformer Q-Network.  Arguments as in the reference (dtqn.py:19-59); `pos` defaults
    to "learned" (the reference's default value 1 is rejected by its own PosEnum)."""

    def __init__(self, obs_dim: int, num_actions: int, embed_per_obs_dim: int, action_dim: int,
                 inner_embed_size: int, num_heads: int, num_layers: int, history_len: int, dropout: float = 0.0,
                 gate: str = "res", identity: bool = False, pos: Union[str, int] = "learned", discrete: bool = False,
                 vocab_sizes: Optional[Union[np.ndarray, int]] = None, bag_size: int = 0, autograd: bool = False,
                 capture_attention: bool = False, _test_lib=None, **kwargs):
        super().__init__()
        # opt-in: callers of the no-grad forward use its output directly (a tensor that requires grad would break .numpy())
        self._autograd = bool(autograd)
        # opt-in: a capturing forward keeps the training records (dtqn_forward_train) to read the attention weights from
        self._capture = bool(capture_attention)
        image = tuple(int(v) for v in obs_dim) if isinstance(obs_dim, (tuple, list, torch.Size)) else None
        if image is not None and len(image) == 2:
            image = (1,) + image                      # representations.py:88-92: H x W means one channel
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout}")     # nn.Dropout's own check
        if pos not in B.POS:
            raise ValueError(f"{pos!r} is not a valid PosEnum")        # PosEnum(pos) in the reference (dtqn.py:101)
        self._lib = _test_lib if _test_lib is not None else engine.get_lib()
        self.obs_dim, self.discrete, self.history_len, self.bag_size = (image if image is not None else obs_dim), discrete, history_len, bag_size
        self.image = image
        self.dropout_p = float(dropout)
        # set_dropout_seed: off by default (a forward without keep-mask keys runs without dropout, whatever self.training says)
        self._drop_seed, self._drop_step = None, 0
        self.num_actions = num_actions
        self.net = B.make_net(self._lib, obs_dim=1 if image is not None else obs_dim, image=image, num_actions=num_actions, embed_per_obs_dim=embed_per_obs_dim,
                              action_dim=action_dim, inner_embed_size=inner_embed_size, num_heads=num_heads,
                              num_layers=num_layers, history_len=history_len, gate=gate, identity=identity, pos=pos,
                              discrete=discrete, vocab_sizes=int(vocab_sizes) if discrete else 0, dropout=dropout,
                              bag_size=bag_size)
        net = self.net
        flat = np.zeros(net.n_theta, dtype=np.float32)
        self._lib.dtqn_net_fill_frozen(ctypes.byref(net), flat.ctypes.data_as(ctypes.c_void_p))
        self.flat = torch.from_numpy(flat)
        self._table = B.param_table(net)
        # width-padded network (DtqnNet.d_real): the buffer holds every tensor at the padded width; state_dict() / load_state_dict()
        # speak the reference's shapes (`_real_shapes`), parameters() are the buffer's own views
        self._real_shapes = {k: shp for k, (_, shp) in B.param_table(net, net.d_real).items()} if net.d_real else None
        self._views = {}
        seen = {}
        for key, (off, shape) in self._table.items():
            trainable = off < net.n_trainable
            if off in seen:                    # shared GRU gate: one Parameter under every layer prefix
                p = seen[off]
            else:
                p = nn.Parameter(self.flat[off:off + int(np.prod(shape))].view(shape), requires_grad=trainable)
                seen[off] = p
                self._views[key] = (p, off, shape)
            _attach(self, key, p)
        # the reference keeps the causal mask as a frozen Parameter per layer (transformer.py:49-53);
        # the kernels never read it, it exists for state_dict compatibility
        mask = torch.triu(torch.ones(history_len, history_len), diagonal=1)
        mask[mask.bool()] = -float("inf")
        for l in range(num_layers):
            _attach(self, f"transformer_layers.{l}.attn_mask", nn.Parameter(mask.clone(), requires_grad=False))
        # storage for the attention weights (transformer.py:46, dtqn.py:135), written by capturing forwards only; `attn_weights`
        # appears with the first capturing forward of a bag network, and `bag_attn_weights` stays None, as in the reference
        for layer in self.transformer_layers:
            layer.alpha = None
        self.bag_attn_weights = None
        self.reset_parameters()

    def set_autograd(self, flag: bool) -> "DTQN":
        """Switch the differentiable forward on or off (see forward)."""
        self._autograd = bool(flag)
        return self

    def set_capture_attention(self, flag: bool) -> "DTQN":
        """Switch attention capture on or off (see forward)."""
        self._capture = bool(flag)
        return self

    def set_dropout_seed(self, seed: Optional[int], step: int = 0) -> "DTQN":
        """Train-mode dropout for forwards called on the module itself.  Once a seed is set, every forward of a module in train mode
        with dropout > 0 -- differentiable or not -- draws the engine's keep masks for (seed, step) and advances step by one; the
        backward of a differentiable forward recomputes the masks of ITS forward.  eval() forwards draw none and leave the counter
        alone.  `set_dropout_seed(None)` turns it off again; setting the same (seed, step) replays the same masks."""
        if seed is None:
            self._drop_seed, self._drop_step = None, 0
        else:
            if int(step) < 0:
                raise ValueError(f"dropout step has to be >= 0, but got {step}")
            self._drop_seed, self._drop_step = int(seed) & 0xFFFFFFFF, int(step)
        return self

    def _dropout_keys(self, _train_dropout) -> Optional[tuple]:
        """(seed, step) of this forward's keep masks, or None: the caller's keys, else the module's own counter in train mode."""
        if self.dropout_p <= 0.0:
            return None
        if _train_dropout is not None:
            return int(_train_dropout[0]) & 0xFFFFFFFF, int(_train_dropout[1]) & 0x7FFFFFFF
        if self._drop_seed is None or not self.training:
            return None
        keys = (self._drop_seed, self._drop_step & 0x7FFFFFFF)
        self._drop_step += 1
        return keys

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset_parameters(self) -> None:
        """utils/torch_utils.py:4-15 as applied by DTQN.__init__ (dtqn.py:156): N(0, 0.02) weights of
        Linear / Embedding / MultiheadAttention, zero biases, LayerNorm (1, 0); the learned position
        table is a bare Parameter and stays 0 (position_encodings.py:41-43)."""
        for key, (p, off, shape) in self._views.items():
            if key == "position_embedding.position_encoding":
                continue
            if self.image is not None and key.startswith("obs_embedding.observation_embedding.") and int(key.split(".")[2]) <= 8:
                # nn.Conv2d is not touched by init_weights (utils/torch_utils.py:4-15): it keeps torch's default,
                # kaiming_uniform(a = sqrt 5) = U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for weight and bias alike
                w_shape = self._views[key.rsplit(".", 1)[0] + ".weight"][2]
                bound = 1.0 / float(np.sqrt(w_shape[1] * 9))
                p.uniform_(-bound, bound)
            elif "layernorm" in key:
                p.fill_(1.0 if key.endswith("weight") else 0.0)
            elif key.endswith("bias"):
                p.zero_()
            else:
                p.normal_(mean=0.0, std=0.02)
        self._zero_padding()

    @torch.no_grad()
    def _zero_padding(self) -> None:
        """Width-padded network: everything outside the reference-shaped part of each tensor is zero (and stays zero under training:
        include/dtqn_hip.h, d_real)."""
        if self._real_shapes is None:
            return
        for key, (p, off, shape) in self._views.items():
            real_shape = self._real_shapes[key]
            if tuple(real_shape) != tuple(shape):
                real = B.unpad_param(self.net, key, p.data, real_shape).clone()
                p.data.zero_()
                p.data.copy_(B.pad_param(self.net, key, real, tuple(shape)))

    def state_dict(self, *args, **kwargs):
        sd = super().state_dict(*args, **kwargs)
        if self._real_shapes is not None:           # the reference's shapes (slices of the buffer; the stacked in_proj tensors as copies)
            prefix = kwargs.get("prefix", args[1] if len(args) > 1 else "")
            for key, real_shape in self._real_shapes.items():
                if prefix + key in sd:
                    sd[prefix + key] = B.unpad_param(self.net, key, sd[prefix + key], real_shape)
        return sd

    def load_state_dict(self, state_dict, *args, **kwargs):
        if self._real_shapes is not None:
            state_dict = dict(state_dict)
            for key, (off, shape) in self._table.items():
                v = state_dict.get(key)
                if v is not None and tuple(v.shape) == tuple(self._real_shapes[key]) and tuple(v.shape) != tuple(shape):
                    state_dict[key] = B.pad_param(self.net, key, v.detach(), tuple(shape))
        return super().load_state_dict(state_dict, *args, **kwargs)

    def _apply(self, fn, recurse=True):
        """Module.to()/cuda()/float(): move the flat buffer once and re-point every view at it."""
        super()._apply(fn, recurse)
        self.flat = fn(self.flat)
        if not self.flat.is_contiguous():
            self.flat = self.flat.contiguous()
        for key, (p, off, shape) in self._views.items():
            p.data = self.flat[off:off + int(np.prod(shape))].view(shape)
        return self

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _forward_images(self, obss: torch.Tensor, dev, _train_dropout=None) -> torch.Tensor:
        """obss [B, seq, C, H, W] (uint8 pixels; the reference casts them to float unscaled) -> Q [B, seq, A]: the convolutional
        embedding (dtqn_img_encode) in front of the row-block forward on precomputed embeddings."""
        from ..image import ImageEncoder
        if dev.type != "cuda" and not getattr(self, "_allow_cpu", False):
            raise engine.EngineUnavailable("DTQN.forward runs on the gfx950 engine only: move the module to a ROCm device")
        Bn, seq = int(obss.size(0)), int(obss.size(1))
        if obss.dtype != torch.uint8:
            # the encoder's first layer gathers uint8 pixels (the reference's replay and context hold images as uint8 and the
            # network sees their float VALUES, dtqn/agents/dtqn.py:199): integral values in 0..255 of any dtype are accepted,
            # anything else (normalised 0..1 images, negative values) would be silently truncated or wrapped by a cast
            # Checked where it costs nothing to ask: host-side inputs every time (no device round trip), device-side inputs on the
            # first such call only (the check is a full pass over the pixels and a blocking read-back: not for the actor's hot path)
            # Device-side inputs afterwards: every DTQN_IMG_CHECK_EVERY-th call (default 64; 1 = every call, 0 = first call only), so a
            # caller that starts feeding normalised images later is still told, at a bounded cost
            n_seen = getattr(self, "_img_range_calls", 0)
            every = _img_check_every()
            if obss.device.type == "cpu" or n_seen == 0 or (every > 0 and n_seen % every == 0):
                o = obss.to(torch.float32)
                if not bool(((o >= 0) & (o <= 255) & (o == o.round())).all()):
                    raise ValueError("image observations must be integral pixel values in 0..255 (uint8 in the replay and the context)")
            if obss.device.type != "cpu":
                self._img_range_calls = n_seen + 1
        imgs = obss.to(device=dev).to(torch.uint8).reshape(Bn * seq, -1).contiguous()
        enc = getattr(self, "_img_enc", None)
        if enc is None or enc.device != dev:
            enc = self._img_enc = ImageEncoder(self._lib, self.net, dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
        tokens = Bn * seq
        idx = torch.arange(tokens, dtype=torch.int32, device=dev)
        xemb = torch.empty(tokens, self.net.d_model, dtype=torch.float32, device=dev)
        enc.prep(self.flat, stream)
        enc.encode(self.flat, imgs, idx, tokens, enc.act_buffer(tokens, "infer"), xemb, idx, stream=stream)
        need = self._lib.dtqn_forward_workspace_floats(ctypes.byref(self.net), Bn)
        ws = getattr(self, "_tiled_ws", None)
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = self._tiled_ws = torch.empty(need, dtype=torch.float32, device=dev)
        q = torch.empty((Bn, seq, self.num_actions), dtype=torch.float32, device=dev)
        td_ = _train_dropout if (_train_dropout is not None and self.dropout_p > 0.0) else None
        cp = lambda t: ctypes.c_void_p(t.data_ptr())
        rc = self._lib.dtqn_forward_tiled_pre(ctypes.byref(self.net), cp(self.flat), cp(xemb), None, Bn, seq, cp(q), cp(ws), 1 if td_ else 0,
                                              int(td_[0]) & 0xFFFFFFFF if td_ else 0, int(td_[1]) & 0xFFFFFFFF if td_ else 0, stream)
        if rc != 0:
            raise RuntimeError(f"dtqn_forward_tiled_pre failed with DTQN status {rc}")
        return q

    def forward(self, obss: torch.Tensor, actions: Optional[torch.Tensor] = None,
                bag_obss: Optional[torch.Tensor] = None, bag_actions: Optional[torch.Tensor] = None,
                _train_dropout: Optional[tuple] = None) -> torch.Tensor:
        """obss [B, seq, obs_dim] (float, or integer tokens for discrete envs), actions [B, seq, 1]
        -> Q [B, seq, num_actions].  No autograd graph, unless the module was built with autograd=True (or set_autograd(True)),
        grad mode is on and a trainable parameter or a continuous `obss` requires grad: then Q is the output of a
        torch.autograd.Function whose backward is the HIP backward (parameters' .grad accumulate as usual; obss.grad for
        continuous observations).  Both compute the same Q, bit for bit.  Dropout is applied only to a forward that has keep-mask
        keys: `_train_dropout=(seed, step)` (the agent's train-mode forwards), or the module's own counter once set_dropout_seed was
        called and the module is in train mode; the differentiable and the no-grad forward draw the same masks for the same keys
        (row-block kernels for both; a whole-sequence shape runs such a forward on its row-block twin).
        With capture_attention=True (or set_capture_attention(True)) every forward also stores, detached, on the device:
        transformer_layers[i].alpha [B, seq, seq], each layer's causal attention weights averaged over heads, and with a bag
        attn_weights [B, seq, bag_size], the bag attention averaged over heads.  Q is the same, bit for bit, as with capture off.
        Image networks and train mode with dropout > 0 (the reference would return post-dropout weights) are refused."""
        if self._capture:
            self._capture_check(_train_dropout)
        keys = self._dropout_keys(_train_dropout)
        if self._autograd and torch.is_grad_enabled():
            if self.image is not None:
                raise NotImplementedError("DTQN autograd: image observations are not covered by the differentiable forward "
                                          "(the fused TD update trains image networks)")
            params = self._grad_params()
            obs_grad = obss.requires_grad and not self.discrete
            if obs_grad or any(p.requires_grad for p in params):
                runner = _GradRunner(self, obss, actions, bag_obss, bag_actions, keys)
                q = _DtqnForward.apply(runner, obss, *params)
                if self._capture:          # the records the backward will read: no extra forward
                    self._store_attention(runner.net, runner.ws, runner.Bn, runner.n)
                return q
        if self._capture:
            return self._forward_capture(obss, actions, bag_obss, bag_actions)
        if keys is not None and self.image is None and self.bag_size == 0:
            return self._forward_dropout(obss, actions, keys)
        return self._forward_nograd(obss, actions, bag_obss, bag_actions, keys)

    def _capture_check(self, _train_dropout) -> None:
        if self.image is not None:
            raise NotImplementedError("DTQN attention capture: image networks are not covered (their forward keeps no attention records)")
        if self.dropout_p > 0.0 and (self.training or _train_dropout is not None):
            raise NotImplementedError("DTQN attention capture: train mode with dropout > 0 is not covered (the reference would return the "
                                      "post-dropout weights); call eval() first")

    @torch.no_grad()
    def _forward_capture(self, obss, actions, bag_obss, bag_actions) -> torch.Tensor:
        """No-grad forward through dtqn_forward_train into a record workspace this module keeps, then the attention weights."""
        runner = _GradRunner(self, obss, actions, bag_obss, bag_actions)
        need = int(self._lib.dtqn_grad_workspace_floats(ctypes.byref(self._grad_net()), runner.Bn, runner.n))
        ws = getattr(self, "_capture_ws", None)
        if need > 0 and (ws is None or ws.numel() < need or ws.device != runner.dev):
            ws = self._capture_ws = None            # (the old one goes before the new one is made)
            ws = self._capture_ws = torch.zeros(need, dtype=torch.float32, device=runner.dev)
        q = runner.forward(ws)
        self._store_attention(runner.net, runner.ws, runner.Bn, runner.n)
        runner.ws = None
        return q

    @torch.no_grad()
    def _forward_dropout(self, obss, actions, keys) -> torch.Tensor:
        """No-grad train-mode forward of a network without bag or images: the differentiable forward's kernels and masks
        (dtqn_forward_train_drop) into a record workspace this module keeps; nothing reads the records."""
        runner = _GradRunner(self, obss, actions, None, None, keys)
        need = int(self._lib.dtqn_grad_workspace_floats(ctypes.byref(self._grad_net()), runner.Bn, runner.n))
        ws = getattr(self, "_drop_ws", None)
        if need > 0 and (ws is None or ws.numel() < need or ws.device != runner.dev):
            ws = self._drop_ws = None            # (the old one goes before the new one is made)
            ws = self._drop_ws = torch.zeros(need, dtype=torch.float32, device=runner.dev)
        q = runner.forward(ws)
        runner.ws = None
        return q

    def _store_attention(self, net, ws: torch.Tensor, Bn: int, n: int) -> None:
        dev = ws.device
        alpha = torch.empty((self.net.num_layers, Bn, n, n), dtype=torch.float32, device=dev)
        bag = torch.empty((Bn, n, self.bag_size), dtype=torch.float32, device=dev) if self.bag_size > 0 else None
        cp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
        rc = self._lib.dtqn_attn_weights(ctypes.byref(net), cp(ws), Bn, n, cp(alpha), cp(bag), stream)
        if rc != 0:
            raise RuntimeError(f"dtqn_attn_weights failed with DTQN status {rc}")
        for l, layer in enumerate(self.transformer_layers):
            layer.alpha = alpha[l]
        if bag is not None:
            self.attn_weights = bag

    def _grad_params(self, with_offsets: bool = False):
        """Every trainable Parameter once (the shared GRU gate is one Parameter under several keys), in buffer order."""
        views = sorted((off, p) for (p, off, shape) in self._views.values() if off < self.net.n_trainable)
        return [(p, off) for off, p in views] if with_offsets else [p for off, p in views]

    def _grad_net(self):
        """The network the differentiable forward runs on: the net itself (row-block) or its row-block twin (whole-sequence
        shapes; same theta layout)."""
        if self.net.tiled:
            return self.net
        twin = getattr(self, "_twin", None)
        if twin is None:
            twin = B.DtqnNet()
            if (self._lib.dtqn_net_tiled_twin(ctypes.byref(self.net), ctypes.byref(twin)) != 0 or twin.n_theta != self.net.n_theta
                    or twin.n_trainable != self.net.n_trainable or B.param_table(twin) != B.param_table(self.net)):
                raise RuntimeError("DTQN autograd: the row-block twin of this whole-sequence network could not be built")
            self._twin = twin
        return twin

    @torch.no_grad()
    def _forward_nograd(self, obss: torch.Tensor, actions: Optional[torch.Tensor] = None,
                        bag_obss: Optional[torch.Tensor] = None, bag_actions: Optional[torch.Tensor] = None,
                        _train_dropout: Optional[tuple] = None) -> torch.Tensor:
        seq = obss.size(1)
        assert seq <= self.history_len, "Cannot forward, history is longer than expected."
        # images: obs_dim is the (C, H, W) shape of one observation (dtqn.py:175-179)
        obs_dim = tuple(obss.size()[2:]) if obss.dim() > 3 else obss.size(2)
        if self.image is not None and obss.dim() == 4 and self.image[0] == 1:
            obs_dim = (1,) + obs_dim                  # an H x W observation is one channel (representations.py:88-92)
        assert obs_dim == self.obs_dim, f"Obs dim is incorrect. Expected {self.obs_dim} got {obs_dim}"
        dev = self.flat.device
        if self.image is not None:
            return self._forward_images(obss, dev, _train_dropout)
        if dev.type != "cuda" and not getattr(self, "_allow_cpu", False):
            raise engine.EngineUnavailable("DTQN.forward runs on the gfx950 engine only: move the module to a ROCm device")
        o = obss.to(device=dev, dtype=torch.float32).contiguous()
        a = None
        if self.net.action_dim > 0:
            a = actions.to(device=dev).reshape(obss.size(0), seq).to(torch.uint8).contiguous()
        q = torch.empty((obss.size(0), seq, self.num_actions), dtype=torch.float32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream) if dev.type == "cuda" else None
        if self.net.tiled:      # contexts / widths beyond one workgroup's LDS (and bag networks): row-block tiled kernels + a workspace
            need = self._lib.dtqn_forward_workspace_floats(ctypes.byref(self.net), int(obss.size(0)))
            ws = getattr(self, "_tiled_ws", None)
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = self._tiled_ws = torch.empty(need, dtype=torch.float32, device=dev)
            cp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
            if self.bag_size > 0:
                # bag_obss [B, bag_size, obs_dim], bag_actions [B, bag_size, 1] (dtqn.py:158-164,201-214)
                assert bag_obss is not None and bag_obss.size(1) == self.bag_size, "bag_obss must be [B, bag_size, obs_dim]"
                bo = bag_obss.to(device=dev, dtype=torch.float32).contiguous()
                ba = None
                if self.net.action_dim > 0:
                    ba = bag_actions.to(device=dev).reshape(obss.size(0), self.bag_size).to(torch.uint8).contiguous()
                # _train_dropout = (seed, step): a train-mode forward of the agent (acting, bag eviction) with dropout > 0
                td_ = _train_dropout if (_train_dropout is not None and self.dropout_p > 0.0) else None
                rc = self._lib.dtqn_forward_bag(ctypes.byref(self.net), cp(self.flat), cp(o), cp(a), cp(bo), cp(ba), int(obss.size(0)), int(seq),
                                                cp(q), cp(ws), 1 if td_ else 0, int(td_[0]) & 0xFFFFFFFF if td_ else 0,
                                                int(td_[1]) & 0xFFFFFFFF if td_ else 0, stream)
                if rc != 0:
                    raise RuntimeError(f"dtqn_forward_bag failed with DTQN status {rc}")
                return q
            rc = self._lib.dtqn_forward_tiled(ctypes.byref(self.net), cp(self.flat), cp(o), cp(a), int(obss.size(0)), int(seq), cp(q), cp(ws), stream)
            if rc != 0:
                raise RuntimeError(f"dtqn_forward_tiled failed with DTQN status {rc}")
            return q
        rc = self._lib.dtqn_forward(ctypes.byref(self.net), ctypes.c_void_p(self.flat.data_ptr()),
                                    ctypes.c_void_p(o.data_ptr()), None if a is None else ctypes.c_void_p(a.data_ptr()),
                                    int(obss.size(0)), int(seq), ctypes.c_void_p(q.data_ptr()), stream)
        if rc != 0:
            raise RuntimeError(f"dtqn_forward failed with DTQN status {rc}")
        return q


class _GradRunner:
    """One differentiable forward: the inputs as the kernels read them and the record workspace this forward owns (so the graph
    stays valid whatever other forwards run before its backward)."""

    def __init__(self, module: DTQN, obss, actions, bag_obss, bag_actions, keys: Optional[tuple] = None):
        m = module
        # (seed, step) of this forward's keep masks, kept for its backward; None: no dropout (step -1 in the C ABI)
        self.seed, self.step = keys if keys is not None else (0, -1)
        seq = obss.size(1)
        assert seq <= m.history_len, "Cannot forward, history is longer than expected."
        assert obss.dim() == 3 and obss.size(2) == m.obs_dim, f"Obs dim is incorrect. Expected {m.obs_dim} got {obss.size(2)}"
        dev = m.flat.device
        if dev.type != "cuda" and not getattr(m, "_allow_cpu", False):
            raise engine.EngineUnavailable("DTQN.forward runs on the gfx950 engine only: move the module to a ROCm device")
        self.m, self.dev, self.Bn, self.n = m, dev, int(obss.size(0)), int(seq)
        self.obs_device, self.obs_dtype = obss.device, obss.dtype
        self.o = obss.detach().to(device=dev, dtype=torch.float32).contiguous()
        self.a = None
        if m.net.action_dim > 0:
            self.a = actions.detach().to(device=dev).reshape(self.Bn, seq).to(torch.uint8).contiguous()
        self.bo = self.ba = None
        if m.bag_size > 0:
            assert bag_obss is not None and bag_obss.size(1) == m.bag_size, "bag_obss must be [B, bag_size, obs_dim]"
            self.bo = bag_obss.detach().to(device=dev, dtype=torch.float32).contiguous()
            if m.net.action_dim > 0:
                self.ba = bag_actions.detach().to(device=dev).reshape(self.Bn, m.bag_size).to(torch.uint8).contiguous()
        self.inputs = (obss, actions, bag_obss, bag_actions)
        self.ws = None

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream) if self.dev.type == "cuda" else None

    def _args(self):
        cp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        return cp(self.o), cp(self.a), cp(self.bo), cp(self.ba)

    def forward(self, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ws: a zeroed-once workspace of at least dtqn_grad_workspace_floats floats to keep the records in (None: a new one)."""
        m = self.m
        net = self.net = m._grad_net()
        need = int(m._lib.dtqn_grad_workspace_floats(ctypes.byref(net), self.Bn, self.n))
        if need <= 0:
            raise RuntimeError("dtqn_grad_workspace_floats: this network is not covered by the differentiable forward")
        self.ws = torch.zeros(need, dtype=torch.float32, device=self.dev) if ws is None else ws
        q = torch.empty((self.Bn, self.n, m.num_actions), dtype=torch.float32, device=self.dev)
        rc = m._lib.dtqn_forward_train_drop(ctypes.byref(net), ctypes.c_void_p(m.flat.data_ptr()), *self._args(), self.Bn, self.n,
                                            ctypes.c_void_p(q.data_ptr()), ctypes.c_void_p(self.ws.data_ptr()), self.seed, self.step,
                                            self._stream())
        if rc != 0:
            raise RuntimeError(f"dtqn_forward_train_drop failed with DTQN status {rc}")
        if net is not m.net and self.step < 0:
            # whole-sequence shapes: the records come from the row-block twin, Q from the kernels the no-grad forward runs
            # (the two families agree to rounding, not bit for bit).  Under dropout Q stays the twin's: Q and the records the
            # backward reads then come from the same masks, drawn once
            obss, actions, bag_obss, bag_actions = self.inputs
            q = m._forward_nograd(obss, actions, bag_obss, bag_actions)
        self.inputs = None                  # the backward reads the kernels' copies (o, a, bo, ba) only
        return q

    def backward(self, dq: torch.Tensor, want_obs: bool):
        m = self.m
        net = m._grad_net()
        dq = dq.detach().to(device=self.dev, dtype=torch.float32).contiguous()
        grad = torch.zeros(m.net.n_trainable, dtype=torch.float32, device=self.dev)
        dobs = torch.empty_like(self.o) if want_obs else None
        cp = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
        rc = m._lib.dtqn_backward_dq_drop(ctypes.byref(net), cp(m.flat), *self._args(), self.Bn, self.n, cp(dq), cp(self.ws), cp(grad),
                                          cp(dobs), self.seed, self.step, self._stream())
        if rc != 0:
            raise RuntimeError(f"dtqn_backward_dq_drop failed with DTQN status {rc}")
        self.ws = None                      # once_differentiable: the records are not read again
        if dobs is not None:
            dobs = dobs.to(device=self.obs_device, dtype=self.obs_dtype)
        return grad, dobs


class _DtqnForward(torch.autograd.Function):
    """Q = DTQN.forward(obss, ...) with every unique trainable Parameter as an input; backward = dtqn_backward_dq_drop with the
    forward's own (seed, step), which travel in ctx with the runner."""

    @staticmethod
    def forward(ctx, runner: _GradRunner, obss, *params):
        ctx.runner = runner
        ctx.dropout_keys = (runner.seed, runner.step)
        return runner.forward()

    @staticmethod
    @once_differentiable
    def backward(ctx, dq):
        runner = ctx.runner
        want_obs = ctx.needs_input_grad[1] and not runner.m.discrete
        grad, dobs = runner.backward(dq, want_obs)
        outs = [grad[off:off + p.numel()].view(p.shape) if ctx.needs_input_grad[2 + i] else None
                for i, (p, off) in enumerate(runner.m._grad_params(with_offsets=True))]
        return (None, dobs, *outs)
