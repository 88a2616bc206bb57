"""The image encoder's kernels (dtqn_amd/csrc/dtqn_image.hip) driven stand-alone -- dtqn_img_prep / dtqn_img_encode / dtqn_img_backward
through dtqn_amd.image.ImageEncoder, no transformer, replay or TD engine -- against torch on the CPU in float64, layer by layer
(docs/image_encoder_tests.md).

The yardstick is the one of grad_f64_helpers / q_f64_helpers: every group is measured at its own scale s = max(group max,
phi * tensor max) of the float64 value, the bound is what torch's own float32 evaluation achieves on the same inputs (D32, floored
at 2^-24, refused above 2^-8) times one margin.  The gradient references are evaluated under the ENGINE's ReLU patterns (y > 0 in
its activation workspace), so that the engine, the fp32 and the float64 reference differentiate one function."""
import ctypes
import time

import numpy as np
import torch

from dtqn_amd import _binding as B
from dtqn_amd.image import ImageEncoder
from oracle import dtqn_oracle as O

from grad_f64_helpers import PHI, U32, scaled
from helpers import pack_theta, unpack_flat
from q_f64_helpers import D32_CEILING

# The smallest power of two that is at least twice the worst engine / D32 measured over every check that goes through judge(), on the
# emulation and on the MI355X together: 3.09 (G11 "b" on the device, the first convolution's bias); tables: docs/image_encoder_tests.md.
MARGIN = 8.0

PRE = "obs_embedding.observation_embedding."
CONV_KEYS = [(PRE + f"{2 * i}.weight", PRE + f"{2 * i}.bias") for i in range(5)]
LIN_KEYS = (PRE + "11.weight", PRE + "11.bias")
ENC_KEYS = [k for pair in CONV_KEYS for k in pair] + list(LIN_KEYS)
SENTINEL_BITS = 0x7FC5A5A5          # a quiet NaN with a payload: whoever reads it poisons its result, whoever keeps it keeps these bits

# name -> image, tokens, d_model, seed, and the launch plan the case exists for (asserted by check_plan from the net's fields and the
# launch arithmetic of dtqn_image.hip restated in launch_plan, so that a case cannot silently stop covering its branch).
CASES = {
    "interior_patch": dict(image=(3, 40, 40), tokens=21, D=64, seed=11,
                           plan=dict(maps=((20, 20), (20, 20), (10, 10), (10, 10), (5, 5)), k1=32, c1_rows=8400, c1_splits=2,
                                     patch_grid=((3, 3), (2, 2), (2, 2), (1, 1)), lds_splits=(47, 21, 21, 5), lds_empty_splits=(9, 0, 0, 0),
                                     fwd_tiles=(7, 7, 2, 2, 1), last_tile_px=(16, 16, 36, 36, 25),
                                     classes={2: ((10, 10),) * 4, 4: ((5, 5),) * 4}, lin_tiles=1, lin_last=21)),
    "odd_nonsquare": dict(image=(1, 37, 27), tokens=5, D=128, seed=12,
                          plan=dict(maps=((19, 14), (19, 14), (10, 7), (10, 7), (5, 4)), k1=16, c1_rows=1330, c1_splits=1,
                                    patch_grid=((3, 2), (2, 1), (2, 1), (1, 1)), lds_splits=(7, 2, 2, 1), lds_empty_splits=(1, 0, 0, 0),
                                    fwd_tiles=(5, 5, 2, 2, 1), last_tile_px=(10, 10, 6, 6, 20),
                                    classes={2: ((10, 7), (10, 7), (9, 7), (9, 7)), 4: ((5, 4), (5, 3), (5, 4), (5, 3))}, lin_tiles=1, lin_last=5)),
    "two_channel": dict(image=(2, 24, 48), tokens=4, D=64, seed=13,
                        plan=dict(maps=((12, 24), (12, 24), (6, 12), (6, 12), (3, 6)), k1=32, c1_rows=1152, c1_splits=1,
                                  patch_grid=((2, 3), (1, 2), (1, 2), (1, 1)), lds_splits=(6, 2, 2, 1), lds_empty_splits=(0, 0, 0, 0),
                                  fwd_tiles=(5, 5, 2, 2, 1), last_tile_px=(32, 32, 8, 8, 18),
                                  classes={2: ((6, 12),) * 4, 4: ((3, 6),) * 4}, lin_tiles=1, lin_last=4)),
    "token_tiles_d256": dict(image=(3, 16, 16), tokens=130, D=256, seed=14,
                             plan=dict(maps=((8, 8), (8, 8), (4, 4), (4, 4), (2, 2)), k1=32, c1_rows=8320, c1_splits=2,
                                       patch_grid=((1, 1), (1, 1), (1, 1), (1, 1)), lds_splits=(32, 32, 32, 32), lds_empty_splits=(6, 6, 6, 6),
                                       fwd_tiles=(1, 1, 1, 1, 1), last_tile_px=(64, 64, 16, 16, 4),
                                       classes={2: ((4, 4),) * 4, 4: ((2, 2),) * 4}, lin_tiles=3, lin_last=2)),
    "one_token": dict(image=(3, 9, 9), tokens=1, D=64, seed=15,
                      plan=dict(maps=((5, 5), (5, 5), (3, 3), (3, 3), (2, 2)), k1=32, c1_rows=25, c1_splits=1,
                                patch_grid=((1, 1), (1, 1), (1, 1), (1, 1)), lds_splits=(1, 1, 1, 1), lds_empty_splits=(0, 0, 0, 0),
                                fwd_tiles=(1, 1, 1, 1, 1), last_tile_px=(25, 25, 9, 9, 4),
                                classes={2: ((3, 3), (3, 2), (2, 3), (2, 2)), 4: ((2, 2), (2, 1), (1, 2), (1, 1))}, lin_tiles=1, lin_last=1)),
}


# --------------------------------------------------------------------------- the launch plan, restated
def layers_of(net):
    """(cin, cout, stride, hi, wi, ho, wo) of the five convolutions: img_layer() of dtqn_image.hip from the net's fields."""
    return [(net.img_c, 64, 2, net.img_h, net.img_w, net.img_h1, net.img_w1), (64, 64, 1, net.img_h1, net.img_w1, net.img_h1, net.img_w1),
            (64, 64, 2, net.img_h1, net.img_w1, net.img_h3, net.img_w3), (64, 128, 1, net.img_h3, net.img_w3, net.img_h3, net.img_w3),
            (128, 128, 2, net.img_h3, net.img_w3, net.img_h5, net.img_w5)]


def launch_plan(net, tokens):
    """What dtqn_img_encode / dtqn_img_backward launch for `tokens` tokens: img_conv_fwd, img_conv_dgrad, img_splits and img_wgrad_plan
    restated (same integer arithmetic)."""
    Ls = layers_of(net)
    up = lambda a, b: (a + b - 1) // b
    plan = dict(maps=tuple((L[5], L[6]) for L in Ls), k1=int(net.img_k1))
    plan["fwd_tiles"] = tuple(up(L[5] * L[6], 64) for L in Ls)
    plan["last_tile_px"] = tuple(L[5] * L[6] - 64 * (up(L[5] * L[6], 64) - 1) for L in Ls)
    rows = tokens * Ls[0][5] * Ls[0][6]
    plan["c1_rows"] = rows
    plan["c1_splits"] = min(2048 // 1, max(1, rows // 4096))              # img_splits(rows, groups = 1 tap x 1 x 1)
    grid, splits, empty = [], [], []
    for cin, cout, _, _, _, ho, wo in Ls[1:]:
        py, px = up(ho, 8), up(wo, 8)
        patches = tokens * py * px
        sp = min(512 // ((cout // 64) * (cin // 64)), max(1, patches // 4))
        per = up(patches, sp)
        grid.append((py, px)); splits.append(sp); empty.append(sp - up(patches, per))
    plan["patch_grid"], plan["lds_splits"], plan["lds_empty_splits"] = tuple(grid), tuple(splits), tuple(empty)
    plan["classes"] = {l: tuple(((Ls[l][3] - (c >> 1) + 1) // 2, (Ls[l][4] - (c & 1) + 1) // 2) for c in range(4)) for l in (2, 4)}
    plan["lin_tiles"], plan["lin_last"] = up(tokens, 64), tokens - 64 * (up(tokens, 64) - 1)
    return plan


def check_plan(name, net, tokens):
    """The case still reaches the branches it exists for."""
    want, have = CASES[name]["plan"], launch_plan(net, tokens)
    bad = {k: (have[k], want[k]) for k in want if have[k] != want[k]}
    assert not bad, (name, "the launch plan of this case moved (have, want)", bad)
    return have


# --------------------------------------------------------------------------- the case: parameters, pixels, lists
def case_cfg(name):
    spec = CASES[name]
    C, H, W = spec["image"]
    return O.NetCfg(obs_dim=C * H * W, num_actions=4, inner_embed_size=spec["D"], num_heads=4, num_layers=1, history_len=8, image=spec["image"])


def case_net(lib, cfg):
    return B.make_net(lib, obs_dim=1, image=cfg.image, num_actions=cfg.num_actions, inner_embed_size=cfg.inner_embed_size,
                      num_heads=cfg.num_heads, num_layers=cfg.num_layers, history_len=cfg.history_len)


def case_inputs(name):
    """Host arrays of a case.  Every token first gets a frame of its own (a permutation); then a few LIVE tokens are pointed at
    another live token's frame (repeated frames), so that the frames of the dead tokens (dsrc -1) belong to them alone.  dst0 / dst1:
    two different permutations of the rows of output arrays with 4 rows more than tokens, about a quarter of the entries -1 each;
    dxemb rows are placed by a third permutation with a stride of D + 24 floats behind an offset of 8 (multiples of 4: the kernels
    load 16 bytes)."""
    spec = CASES[name]
    C, H, W = spec["image"]
    T, D = spec["tokens"], spec["D"]
    rng = np.random.default_rng(spec["seed"])
    frames = rng.integers(0, 256, size=(T + 1, C * H * W), dtype=np.uint8)           # frame T is the spare the dead tokens' test draws on
    index = rng.permutation(T).astype(np.int32)
    n_dead = int(round(T / 5))
    dead = set(rng.choice(T, size=n_dead, replace=False).tolist()) if n_dead else set()
    if T > 128:                                    # -1 in every token tile of the Linear, and as the last token
        dead |= {5, 70, T - 2, T - 1}
    live = np.array([t for t in range(T) if t not in dead], dtype=np.int64)
    pairs = []
    if len(live) >= 3:
        pick = rng.choice(live, size=2 * max(1, len(live) // 8), replace=False)
        pairs = [(int(a), int(b)) for a, b in pick.reshape(-1, 2)]
        for a, b in pairs:
            index[b] = index[a]
    rows = T + 4
    dst0, full1 = rng.permutation(rows)[:T].astype(np.int32), rng.permutation(rows)[:T].astype(np.int32)
    dst1 = full1.copy()
    if T > 1:
        dst0[rng.choice(T, size=max(1, T // 4), replace=False)] = -1
        dst1[rng.choice(T, size=max(1, T // 4), replace=False)] = -1
        both = int(np.argmax(dst0 >= 0))                 # at least one token is named by both lists
        dst1[both] = full1[both]
    if T > 128:
        dst0[T - 1] = -1
        dst1[64] = -1
    stride, base = D + 24, 8
    dxemb = rng.standard_normal(base + T * stride + 8).astype(np.float32)
    slot = rng.permutation(T)
    dsrc = (base + slot * stride).astype(np.int32)
    for t in dead:
        dsrc[t] = -1
    return dict(frames=frames, index=index, dead=sorted(dead), pairs=pairs, dst0=dst0, dst1=dst1, rows=rows, dxemb=dxemb, dsrc=dsrc,
                tokens=T, D=D, image=(C, H, W))


def sentinel(n, device):
    return torch.full((int(n),), SENTINEL_BITS, dtype=torch.int32, device=device).view(torch.float32)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


class Harness:
    """Net, ImageEncoder and device buffers of one case; every call of the encoder's C ABI the tests make goes through here."""

    def __init__(self, lib, name, device="cpu"):
        self.name, self.device = name, torch.device(device)
        self.cfg = case_cfg(name)
        self.net = case_net(lib, self.cfg)
        self.inp = case_inputs(name)
        self.T, self.D = self.inp["tokens"], self.inp["D"]
        self.params = O.init_params(self.cfg, seed=CASES[name]["seed"], perturb=True)
        dev = self.device
        self.theta = torch.from_numpy(pack_theta(self.net, self.params)).to(dev)
        self.enc = ImageEncoder(lib, self.net, dev)
        self.lib = lib
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.frames, self.index = to(self.inp["frames"]), to(self.inp["index"])
        self.dst0, self.dst1, self.dsrc, self.dxemb = to(self.inp["dst0"]), to(self.inp["dst1"]), to(self.inp["dsrc"]), to(self.inp["dxemb"])
        self.act = torch.empty(int(lib.dtqn_img_act_floats(ctypes.byref(self.net), self.T)), dtype=torch.float32, device=dev)
        self.enc.prep(self.theta, self.stream())
        self.canonical = False          # the workspace holds the maps of the case's own token list and frames
        self.grad_bits = None           # the bits of the first backward on them (NaN in gact / wpart before it)

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self.device.type == "cuda" else None

    def sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    def encode(self, index=None, dst0=None, dst1=None, two=True, frames=None):
        """NaN into the activation workspace, then dtqn_img_encode -> (out0, out1) [rows, D], sentinel where no dst names a row."""
        self.act.fill_(float("nan"))
        out0, out1 = sentinel(self.inp["rows"] * self.D, self.device), sentinel(self.inp["rows"] * self.D, self.device)
        self.enc.encode(self.theta, self.frames if frames is None else frames, self.index if index is None else index, self.T, self.act,
                        out0, self.dst0 if dst0 is None else dst0, out1 if two else None, (self.dst1 if dst1 is None else dst1) if two else None,
                        stream=self.stream())
        self.sync()
        self.canonical = index is None and frames is None
        return out0.view(self.inp["rows"], self.D), out1.view(self.inp["rows"], self.D)

    def backward(self, dsrc=None, nan_fill=True, frames=None):
        """dtqn_img_backward on the maps of the last encode -> the flat gradient buffer (n_theta floats, sentinel where nothing is written).
        nan_fill: NaN into gact and wpart first (else they keep what the previous call left)."""
        net_ref = ctypes.byref(self.net)
        if nan_fill or self.enc._gact is None:
            self.enc._gact = torch.full((int(self.lib.dtqn_img_gact_floats(net_ref, self.T)),), float("nan"), dtype=torch.float32, device=self.device)
            self.enc._wpart = torch.full((int(self.lib.dtqn_img_wpart_floats(net_ref)),), float("nan"), dtype=torch.float32, device=self.device)
        grad = sentinel(self.net.n_theta, self.device)
        self.enc.backward(self.theta, self.frames if frames is None else frames, self.index, self.T, self.act, self.dxemb,
                          self.dsrc if dsrc is None else dsrc, grad, stream=self.stream())
        self.sync()
        return grad

    def maps(self):
        """The five post-ReLU feature maps in the activation workspace, [T, ho wo, cout] each (NHWC)."""
        act, out, pos = self.act.cpu().numpy(), [], 0
        for _, co, _, _, _, ho, wo in layers_of(self.net):
            n = self.T * ho * wo * co
            out.append(act[pos:pos + n].reshape(self.T, ho * wo, co))
            pos += n
        assert pos == act.size
        return out


# --------------------------------------------------------------------------- the reference
def conv_stack(p, x, masks=None):
    """O.embed_images restated with every layer kept: -> (post-activation maps [T, C, h, w], pre-activations, embedding [T, D]).
    masks: the ReLU is replaced by multiplication with these patterns (the reference then differentiates the engine's function)."""
    maps, pres = [], []
    for i, (_, _, s) in enumerate(O.IMG_CHANS):
        t = torch.nn.functional.conv2d(x, p[CONV_KEYS[i][0]], p[CONV_KEYS[i][1]], stride=s, padding=1)
        x = torch.relu(t) if masks is None else t * masks[i].to(t.dtype)
        pres.append(t.detach()); maps.append(x)
    return maps, pres, x.flatten(1) @ p[LIN_KEYS[0]].t() + p[LIN_KEYS[1]]


def pixels_of(inp, frames=None):
    C, H, W = inp["image"]
    fr = inp["frames"] if frames is None else frames
    return torch.from_numpy(fr[inp["index"]].reshape(inp["tokens"], C, H, W).astype(np.float32))


def nhwc(t):
    """[T, C, h, w] -> [T, h w, C] float64 / float32 numpy, the engine's layout"""
    a = t.detach().numpy()
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(a.shape[0], a.shape[2] * a.shape[3], a.shape[1])


def forward_reference(cfg, params, inp):
    """fp32 and float64 torch forwards (own ReLU) of the case -> {32 / 64: (maps NHWC, embedding)}; the fp32 one is checked to be
    O.embed_images bit for bit."""
    x = pixels_of(inp)
    p32 = {k: params[k] for k in ENC_KEYS}
    p64 = {k: v.double() for k, v in p32.items()}
    with torch.no_grad():
        m32, _, e32 = conv_stack(p32, x)
        m64, pre64, e64 = conv_stack(p64, x.double())
        assert torch.equal(e32, O.embed_images(params, cfg, x.unsqueeze(0))[0]), "conv_stack is not the oracle's embed_images"
    return {32: ([nhwc(m) for m in m32], e32.numpy()), 64: ([nhwc(m) for m in m64], e64.numpy()), "pre64": pre64, "masks32": [m > 0 for m in m32]}


def mask_disagreements(masks, pres):
    """(count, worst |pre-activation| / layer scale) of the places where a ReLU pattern differs from the sign of the pre-activation."""
    n, worst = 0, 0.0
    for m, t in zip(masks, pres):
        flips = (t > 0) != m
        n += int(flips.sum())
        if flips.any():
            worst = max(worst, float(t.abs()[flips].max() / t.abs().max()))
    return n, worst


def check_masks(masks, pres, what):
    """The rule of test_image_golden.check_image_gradient_f64: at most max(2, n_relu // 20000) disagreements between the given ReLU
    patterns and the float64 signs, none at a pre-activation above 2e-5 of the layer's scale."""
    n_relu = sum(int(m.numel()) for m in masks)
    n, worst = mask_disagreements(masks, pres)
    assert n <= max(2, n_relu // 20000) and worst <= 2e-5, (what, "ReLU patterns against the float64 signs", n, n_relu, worst)
    return dict(flips=n, n_relu=n_relu, worst=worst)


def gradient_reference(params, inp, masks, dtype):
    """d/d(parameters) of sum_t <dxemb row of t, embedding of t> over the live tokens, the ReLUs replaced by `masks`, in `dtype`;
    parameters, pixels and dxemb widened exactly.  -> ({key: array}, pre-activations)"""
    T, D = inp["tokens"], inp["D"]
    dx = np.zeros((T, D), dtype=np.float32)
    for t in range(T):
        if inp["dsrc"][t] >= 0:
            dx[t] = inp["dxemb"][inp["dsrc"][t]:inp["dsrc"][t] + D]
    p = {k: params[k].detach().to(dtype).clone().requires_grad_(True) for k in ENC_KEYS}
    _, pres, emb = conv_stack(p, pixels_of(inp).to(dtype), masks)
    g = torch.autograd.grad((emb * torch.from_numpy(dx).to(dtype)).sum(), [p[k] for k in ENC_KEYS])
    return {k: v.numpy() for k, v in zip(ENC_KEYS, g)}, pres


def engine_masks(h: "Harness"):
    """y > 0 in the engine's activation workspace, NHWC -> NCHW booleans (test_image_golden.image_conv_masks for a plain token list)"""
    out = []
    for m, (_, co, _, _, _, ho, wo) in zip(h.maps(), layers_of(h.net)):
        out.append(torch.from_numpy(np.ascontiguousarray(m.reshape(h.T, ho, wo, co).transpose(0, 3, 1, 2)) > 0))
    return out


# --------------------------------------------------------------------------- groups and figures
def param_groups(key, shape):
    """(shape the tensor is viewed in, [(group, index)]) of an encoder tensor: the tiles a workgroup or wave unit of the weight-gradient
    kernels owns.  Convolutions 2..5: (tap, 64 of cout, 64 of cin); the first: (input channel, tap); biases: 64-channel blocks;
    the Linear's weight [D, 128 P] (column c P + p): one group per spatial position p; its bias: one tensor."""
    i = ENC_KEYS.index(key)
    if key == LIN_KEYS[0]:
        P = shape[1] // 128
        return (shape[0], 128, P), [(f"{key}[pos {p}]", (slice(None), slice(None), p)) for p in range(P)]
    if key == LIN_KEYS[1]:
        return tuple(shape), [(key, ())]
    if i % 2 == 1:
        return tuple(shape), [(f"{key}[{b * 64}:]", (slice(b * 64, b * 64 + 64),)) for b in range(shape[0] // 64)]
    co, ci = shape[0], shape[1]
    if i == 0:
        return (co, ci, 9), [(f"{key}[ci {c}, tap {t}]", (slice(None), c, t)) for c in range(ci) for t in range(9)]
    return (co, ci, 9), [(f"{key}[tap {t}, co {a * 64}:, ci {b * 64}:]", (slice(a * 64, a * 64 + 64), slice(b * 64, b * 64 + 64), t))
                         for t in range(9) for a in range(co // 64) for b in range(ci // 64)]


def param_group_errors(have, ref, phi=PHI):
    """{group: |have - ref| / s} over the encoder's tensors, s = max(group max, phi * tensor max) of `ref` (float64)"""
    errs = {}
    for key in ENC_KEYS:
        r = np.asarray(ref[key], dtype=np.float64)
        hv = np.asarray(have[key], dtype=np.float64)
        assert hv.shape == r.shape, (key, hv.shape, r.shape)
        view, groups = param_groups(key, r.shape)
        r, hv = r.reshape(view), hv.reshape(view)
        tmax = float(np.abs(r).max())
        assert tmax > 0.0, ("an encoder tensor whose float64 gradient is zero altogether", key)
        for name, idx in groups:
            e, _ = scaled(float(np.abs(hv[idx] - r[idx]).max()), float(np.abs(r[idx]).max()), tmax, phi)
            errs[name] = float(e)
    return errs


def forward_group_errors(have_maps, have_emb, ref_maps, ref_emb, emb_rows=None, phi=PHI):
    """{group: error / s}: per (layer, token), per (layer, token, last 64-pixel tile) where a token has more than one tile, and per
    embedding row.  emb_rows: boolean [T], the embedding rows `have_emb` holds (a token no dst names has none)."""
    errs = {}
    for l, (hv, r) in enumerate(zip(have_maps, ref_maps)):
        r = np.asarray(r, dtype=np.float64)
        d = np.abs(np.asarray(hv, dtype=np.float64) - r)
        tmax = float(np.abs(r).max())
        e, _ = scaled(d.max(axis=(1, 2)), np.abs(r).max(axis=(1, 2)), tmax, phi)
        for t in range(r.shape[0]):
            errs[f"conv {l + 1} token {t}"] = float(e[t])
        lo = 64 * ((r.shape[1] + 63) // 64 - 1)
        if lo > 0:
            e, _ = scaled(d[:, lo:].max(axis=(1, 2)), np.abs(r[:, lo:]).max(axis=(1, 2)), tmax, phi)
            for t in range(r.shape[0]):
                errs[f"conv {l + 1} token {t} last tile"] = float(e[t])
    r = np.asarray(ref_emb, dtype=np.float64)
    e, _ = scaled(np.abs(np.asarray(have_emb, dtype=np.float64) - r).max(axis=1), np.abs(r).max(axis=1), float(np.abs(r).max()), phi)
    for t in range(r.shape[0]):
        if emb_rows is None or emb_rows[t]:
            errs[f"embedding token {t}"] = float(e[t])
    return errs


def judge(eng, e32, what, margin=None, assert_=True):
    """D32 = the fp32 reference's worst group (floor 2^-24, ceiling 2^-8: beyond it the pair of references is broken); every group of
    the engine within margin * D32.  -> figures"""
    margin = MARGIN if margin is None else margin
    d32 = max(max(e32.values()), U32)
    assert d32 <= D32_CEILING, ("the fp32 and the float64 reference disagree", what, d32, max(e32, key=e32.get))
    assert all(np.isfinite(v) for v in eng.values()), ("non-finite engine value", what, [g for g, v in eng.items() if not np.isfinite(v)][:8])
    worst = max(eng, key=eng.get)
    fig = dict(d32=d32, d32_group=max(e32, key=e32.get), rel_err=eng[worst], group=worst, over_d32=eng[worst] / d32, groups=len(eng))
    print(f"[image encoder f64] {what}: engine / D32 = {fig['over_d32']:.3f} at {worst!r}; D32 = {d32:.3e} at {fig['d32_group']!r}; {len(eng)} groups")
    if assert_:
        bad = {g: (e, e / d32) for g, e in eng.items() if e > margin * d32}
        assert not bad, ("groups beyond margin * D32 of the float64 value (error / s, error / D32)", what, fig, dict(list(bad.items())[:12]))
    return fig


def check_param_groups(got, g64, g32, what, assert_=True):
    """got, g64, g32: {key: reference-shaped array} holding at least the encoder's tensors, the three under the same ReLU patterns:
    every per-tap / per-tile group (param_groups) of `got` within MARGIN * D32 of float64 at the group's scale."""
    return judge(param_group_errors(got, g64), param_group_errors(g32, g64), what, assert_=assert_)


# --------------------------------------------------------------------------- the checks
def token_embeddings(inp, out0, out1):
    """[T, D] rows of the embedding as the two output arrays hold them, and which tokens have one"""
    T, D = inp["tokens"], inp["D"]
    emb, have = np.zeros((T, D), dtype=np.float32), np.zeros(T, dtype=bool)
    for t in range(T):
        for o, d in ((out0, inp["dst0"]), (out1, inp["dst1"])):
            if d[t] >= 0 and not have[t]:
                emb[t], have[t] = o[d[t]], True
    return emb, have


def check_forward(h: "Harness", ref):
    """Every layer's map and every embedding row against float64; the exact properties of the output lists."""
    inp, T = h.inp, h.T
    # a permuted token list first (identity destinations), so that the workspace ends up holding the case's own order
    perm = np.random.default_rng(CASES[h.name]["seed"] + 100).permutation(T)
    ident = torch.arange(T, dtype=torch.int32, device=h.device)
    outp, _ = h.encode(index=h.index[torch.from_numpy(perm).to(h.device)].contiguous(), dst0=ident, two=False)
    embp = outp.cpu()
    t0 = time.perf_counter()
    out0, out1 = h.encode()
    print(f"[image encoder f64] {h.name}: encode {1e3 * (time.perf_counter() - t0):.2f} ms")
    out0, out1 = out0.cpu(), out1.cpu()
    b0, b1, bp = bits(out0), bits(out1), bits(embp)
    for o, d, nm in ((b0, inp["dst0"], "out0"), (b1, inp["dst1"], "out1")):
        named = np.zeros(inp["rows"], dtype=bool)
        named[d[d >= 0]] = True
        assert np.all(o[~named] == SENTINEL_BITS), (h.name, nm, "a row no dst names was written", np.argwhere(~named & (o != SENTINEL_BITS).any(axis=1)).ravel()[:8])
        assert np.all(o[named] != SENTINEL_BITS), (h.name, nm, "a named row kept the sentinel")
    both = [t for t in range(T) if inp["dst0"][t] >= 0 and inp["dst1"][t] >= 0]
    assert both, "the case names no token in both lists"
    for t in both:
        assert np.array_equal(b0[inp["dst0"][t]], b1[inp["dst1"][t]]), (h.name, "token", t, "differs between the two output arrays")
    assert np.all(bp[T:] == SENTINEL_BITS)
    # rows of the permuted run: row j is token perm[j]
    row_of = {int(perm[j]): j for j in range(T)}
    for t in range(T):
        for o, d in ((b0, inp["dst0"]), (b1, inp["dst1"])):
            if d[t] >= 0:
                assert np.array_equal(o[d[t]], bp[row_of[t]]), (h.name, "token", t, "changes its bits with its place in the token list")
    for a, b in inp["pairs"]:
        assert np.array_equal(bp[row_of[a]], bp[row_of[b]]), (h.name, "tokens", a, b, "hold the same frame and differ")
    emb = embp.numpy()[:T][[row_of[t] for t in range(T)]]            # every token's row, in the case's order
    maps = h.maps()
    assert all(np.isfinite(m).all() for m in maps), (h.name, "NaN of the workspace fill left in a feature map")
    eng = forward_group_errors(maps, emb, *ref[64])
    e32 = forward_group_errors(*ref[32], *ref[64])
    return judge(eng, e32, f"{h.name} forward")


def check_gradients(h: "Harness", ref, assert_=True):
    """dtqn_img_backward against the float64 gradient under the engine's own ReLU patterns, group by group; the sentinel outside the
    encoder's tensors.  -> figures"""
    if not h.canonical:
        h.encode()
    masks = engine_masks(h)
    fig_m = check_masks(masks, ref["pre64"], f"{h.name} engine")
    t0 = time.perf_counter()
    grad = h.backward()
    h.seconds_backward = time.perf_counter() - t0
    gb = h.grad_bits = bits(grad)
    tab = B.param_table(h.net)
    owned = np.zeros(h.net.n_theta, dtype=bool)
    for k in ENC_KEYS:
        owned[tab[k][0]:tab[k][0] + int(np.prod(tab[k][1]))] = True
    assert np.all(gb[~owned] == SENTINEL_BITS), (h.name, "dtqn_img_backward wrote outside the encoder's tensors", np.argwhere(~owned & (gb != SENTINEL_BITS)).ravel()[:8])
    got = unpack_flat(h.net, grad.cpu().numpy(), ENC_KEYS)
    g64, pre = gradient_reference(h.params, h.inp, masks, torch.float64)
    g32, _ = gradient_reference(h.params, h.inp, masks, torch.float32)
    check_masks(masks, pre, f"{h.name} engine, masked float64 forward")
    fig = check_param_groups(got, g64, g32, f"{h.name} gradients", assert_=assert_)
    fig["masks"] = fig_m
    return fig


def check_exact(h: "Harness"):
    """Against the bits of the first backward (NaN in gact and wpart, and in the workspace before the encode): the same call on the
    buffers as that run left them; other pixels under the dead tokens; every token dead."""
    if not h.canonical:
        h.encode()
    if h.grad_bits is None:
        h.grad_bits = bits(h.backward())
    gb = h.grad_bits
    assert np.array_equal(bits(h.backward(nan_fill=False)), gb), (h.name, "dtqn_img_backward depends on what gact / wpart held")
    tab = B.param_table(h.net)
    if h.inp["dead"]:
        frames = h.inp["frames"].copy()
        for t in h.inp["dead"]:
            frames[h.inp["index"][t]] = h.inp["frames"][h.T][::-1] if t % 2 else h.inp["frames"][h.T]
        fr = torch.from_numpy(frames).to(h.device)
        h.encode(frames=fr)
        g2 = bits(h.backward(frames=fr))
        diff = {k: int(np.count_nonzero(g2[tab[k][0]:tab[k][0] + int(np.prod(tab[k][1]))] != gb[tab[k][0]:tab[k][0] + int(np.prod(tab[k][1]))])) for k in ENC_KEYS}
        assert not any(diff.values()), (h.name, "the pixels of a token whose dsrc is -1 reach the gradient", diff)
    # (whatever maps the workspace holds by now: with no live token nothing of them may arrive)
    g0 = h.backward(dsrc=torch.full_like(h.dsrc, -1)).cpu().numpy()
    for k in ENC_KEYS:
        v = g0[tab[k][0]:tab[k][0] + int(np.prod(tab[k][1]))]
        assert np.all(v == 0.0), (h.name, k, "not exactly zero with every dsrc at -1", int(np.count_nonzero(v != 0.0)))


class CaseRun:
    """One case shared by its tests: the plan (asserted at construction), the references, and each check at most once.  A check does
    not depend on the verdict of another: each one encodes or runs the first backward itself where no earlier one has."""

    def __init__(self, lib, name, device="cpu"):
        t0 = time.perf_counter()
        self.h = Harness(lib, name, device)
        self.plan = check_plan(name, self.h.net, self.h.T)
        self.ref = forward_reference(self.h.cfg, self.h.params, self.h.inp)
        self.reference_masks = check_masks(self.ref["masks32"], self.ref["pre64"], f"{name} fp32 reference")
        self.seconds = time.perf_counter() - t0

    def _timed(self, fn, *args):
        t0 = time.perf_counter()
        try:
            return fn(*args)
        finally:
            self.seconds += time.perf_counter() - t0
            print(f"[image encoder f64] {self.h.name}: {self.seconds:.2f} s in this case so far")

    def forward(self):
        return self._timed(check_forward, self.h, self.ref)

    def gradients(self):
        fig = self._timed(check_gradients, self.h, self.ref)
        h, m = self.h, fig["masks"]
        print(f"[image encoder f64] {h.name}: backward {1e3 * h.seconds_backward:.2f} ms; mask disagreements engine {m['flips']} / "
              f"fp32 reference {self.reference_masks['flips']} of {m['n_relu']} (cap {max(2, m['n_relu'] // 20000)})")
        return fig

    def exact(self):
        self._timed(check_exact, self.h)
