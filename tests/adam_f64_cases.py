"""Cases of the optimizer launches against the float64 reference of adam_f64_helpers.py, shared by the CPU-emulation tests
(test_emu_adam_f64.py) and their -m gpu twins (test_gpu_adam_f64.py).  Every case is one or a few isolated launches on the smallest
nets that reach every code path:
  d64     history 8, width 64, batch 2: partial last block, at most 256 norm partials;
  d128    width 128 (the net of adam_batched_cases' norm_parts_remainder_loop): more than 256 partials;
  sin48   width 48 padded to 64 with sinusoidal positions: width padding inside the trainable part, a frozen tail behind it.
The worst error / bound of each case goes to the parity report under adam_f64_<case>."""
import ctypes

import numpy as np
import torch

import adam_f64_helpers as H
from adam_f64_helpers import Hyper
from helpers import make_td_case, padding_mask, parity_report
from oracle import dtqn_oracle as O

NETS = {
    "d64": dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=8),
    "d128": dict(obs_dim=3, num_actions=3, inner_embed_size=128, num_heads=8, num_layers=2, history_len=8),
    "sin48": dict(obs_dim=3, num_actions=3, inner_embed_size=48, num_heads=6, num_layers=1, history_len=8, pos="sin"),
}
_ENGINES = {}


def engine(lib, device, name, batch=2):
    key = (id(lib), device, name, batch)
    if key not in _ENGINES:
        cfg = O.NetCfg(**NETS[name])
        gpu = device != "cpu"
        net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=11, batch=batch, T=12, n_eps=10, mask=-5, device=device, test_lib=not gpu)
        n = eng.net.n_trainable
        assert n % 4 == 0 and n % H.OPT_BLOCK != 0, "float4 loads; a partial last block"
        if name == "d64":
            assert eng.n_norm_blocks <= 256
        if name == "d128":
            assert eng.n_norm_blocks > 256
        if name == "sin48":
            assert eng.net.n_theta > n and padding_mask(eng.net).any()
            # the two frozen tails differ, so a copy that runs past the trainable part shows
            eng.theta_tgt[n:] += 1.0
        _ENGINES[key] = (eng, padding_mask(eng.net))
    return _ENGINES[key]


def _report(name, ratios):
    parity_report("adam_f64_" + name, {k: float(v) for k, v in ratios.items()})


def _run(lib, device, netname, name, seed, k, hp=Hyper(), tuf=10_000, **kw):
    eng, pad = engine(lib, device, netname)
    ratios, inp, out = H.run_case(eng, seed, k, hp, tuf, pad=pad, what=name, **kw)
    _report(name, ratios)
    return eng, ratios, inp, out


# ---- step index: bit patterns of the squaring loop, the underflow of beta^k, bc1 = 1 exactly, tuf = 10000 at k = 10000 and 9999
STEP_KS = (1, 2, 3, 7, 8, 1000, 1023, 1024, 9999, 10000, 65535, 65536, 10 ** 6)


def run_step_index(lib, device, k):
    eng, r, inp, out = _run(lib, device, "d64", f"k{k}", 100 + k % 997, k, r64=True)
    assert out["stats"][10] == (1.0 if k % 10_000 == 0 else 0.0)
    if k >= 65535:
        assert np.float32(1.0 - float(np.float32(0.9)) ** k) == 1.0          # bc1 = 1 exactly


def run_step_index_other_nets(lib, device, netname, k):
    _run(lib, device, netname, f"{netname}_k{k}", 200 + k, k, r64=True)


# ---- clip
CLIPS = (0.5, 1.0, 10.0)
REGIMES = {"below": 1e-3, "just_below": 1.0 - 5e-7, "just_above": 1.0 + 5e-7, "above_1e6": None, "above_1e15": None}


def run_clip(lib, device, netname, clip, regime):
    hp = Hyper(clip=clip)
    target = {"above_1e6": 1e6, "above_1e15": 1e15}.get(regime) or clip * REGIMES[regime]
    name = f"{netname}_clip{clip}_{regime}"
    eng, r, inp, out = _run(lib, device, netname, name, 300 + int(clip * 10), 5, hp, scaled_norm=target)
    norm = float(out["stats"][1])
    assert abs(norm - target) <= (H.NORM_RTOL + 1e-6 if regime.startswith("just") else 1e-3) * target
    if regime == "below":
        assert out["stats"][8] == 1.0                                          # the factor is exactly 1
    if regime.startswith("above"):
        assert out["stats"][8] < 1e-4 and np.isfinite(out["stats"][1])


def run_zero_gradient(lib, device):
    """An all-zero gradient.  From m = v = 0 nothing moves: theta, m, v bit-unchanged.  From a trajectory's m, v both decay as the
    reference's do, and theta follows the reference (torch's Adam still steps along exp_avg when the gradient is zero)."""
    eng, pad = engine(lib, device, "d64")
    n = eng.net.n_trainable
    inp = H.synth_inputs(n, 41, pad=pad, k=1, zero_grad=True)
    out = H.launch_step(eng, inp, 1, Hyper(), 10_000)
    r = H.check_step(eng, inp, out, 1, Hyper(), 10_000, what="zero_grad_k1")
    assert out["stats"][1] == 0.0 and out["stats"][8] == 1.0
    assert np.array_equal(H.bits(out["theta_pol"][:n]), H.bits(inp["theta"])) and not out["m"].any() and not out["v"].any()
    _report("zero_grad_k1", r)
    inp = H.synth_inputs(n, 42, pad=pad, k=6, zero_grad=True)
    out = H.launch_step(eng, inp, 6, Hyper(), 10_000)
    r = H.check_step(eng, inp, out, 6, Hyper(), 10_000, what="zero_grad_k6")
    live = inp["m"] != 0
    assert live.any() and (np.abs(out["m"][live]) < np.abs(inp["m"][live])).all() and (out["v"][inp["v"] > H.TINY] < inp["v"][inp["v"] > H.TINY]).all()
    _report("zero_grad_k6", r)


def run_grad_scale(lib, device, gs, clipped):
    """grad_scale = 1 / world is how data parallel reaches the kernel: norm, factor and step are the reference's on g * grad_scale."""
    hp = Hyper(grad_scale=gs)
    name = f"grad_scale{gs}_{'clipped' if clipped else 'unclipped'}"
    eng, r, inp, out = _run(lib, device, "d64", name, 500, 4, hp, scaled_norm=30.0 if clipped else 0.01)
    # the same gradient, whatever the scale: the reported norm carries it
    assert abs(float(out["stats"][1]) - (30.0 if clipped else 0.01)) <= 1e-4 * (30.0 if clipped else 0.01)
    assert (out["stats"][8] < 1.0) == clipped


HYPERS = [(lr, b, e) for lr in (3e-4, 1e-3) for b in ((0.9, 0.999), (0.8, 0.99)) for e in (1e-8, 1e-6)]


def run_hyper(lib, device, lr, betas, eps):
    hp = Hyper(lr=lr, beta1=betas[0], beta2=betas[1], eps=eps)
    _run(lib, device, "d64", f"lr{lr}_b{betas[0]}_{betas[1]}_eps{eps}", 600, 7, hp, r64=True)


def run_tiny(lib, device, k):
    """Gradients of 1e-20: g^2 is subnormal, the step is eps-dominated.  (The norm of subnormal squares carries no relative
    precision, so the 2e-6 norm check does not apply; the reference takes the engine's norm as everywhere.)"""
    eng, r, inp, out = _run(lib, device, "d64", f"tiny_k{k}", 700 + k, k, gmag=1e-20)
    assert out["stats"][8] == 1.0 and out["stats"][1] < 1e-15


# ---- target copy
def run_target_copy(lib, device):
    eng, pad = engine(lib, device, "sin48")
    n = eng.net.n_trainable
    for k, tuf in ((2, 2), (4, 2), (3, 2), (4, 0), (10_000, 10_000), (9_999, 10_000)):
        inp = H.synth_inputs(n, 800 + k, pad=pad, k=k)
        out = H.launch_step(eng, inp, k, Hyper(), tuf)
        r = H.check_step(eng, inp, out, k, Hyper(), tuf, what=f"target_k{k}_tuf{tuf}")     # the copy / no copy is checked inside
        assert out["stats"][10] == (1.0 if tuf and k % tuf == 0 else 0.0)
        _report(f"target_k{k}_tuf{tuf}", r)
    # a skipped update (sticky flag of an earlier non-finite norm) at k % tuf == 0: no copy, nothing written
    inp = H.synth_inputs(n, 899, pad=pad, k=4)
    out = H.launch_step(eng, inp, 4, Hyper(), 2, poisoned=True)
    assert out["stats"][11] == 3.0 and out["stats"][10] == 0.0 and out["sc"][1] == 3 and out["sc"][3] == 1
    assert np.array_equal(H.bits(out["theta_tgt"]), H.bits(out["before"]["theta_tgt"]))
    assert np.array_equal(H.bits(out["theta_pol"]), H.bits(out["before"]["theta_pol"]))
    assert np.array_equal(H.bits(out["m"]), H.bits(inp["m"])) and np.array_equal(H.bits(out["v"]), H.bits(inp["v"]))
    eng.step_counter[3] = 0


def run_target_sync(lib, device):
    """dtqn_target_sync copies all n_theta floats bit-exactly (the frozen tail too), and leaves the source alone."""
    eng, pad = engine(lib, device, "sin48")
    nth = eng.net.n_theta
    rng = np.random.Generator(np.random.PCG64(5))
    src = rng.standard_normal(nth).astype(np.float32)
    src[::97] = np.float32(1e-41)                                # denormals and negative zeros are bits like any other
    src[1::97] = np.float32(-0.0)
    keep_pol, keep_tgt = eng.theta_pol.clone(), eng.theta_tgt.clone()
    eng.theta_pol.copy_(torch.from_numpy(src))
    eng.theta_tgt.fill_(3.0)
    eng.target_sync()
    assert np.array_equal(H.bits(H._np(eng.theta_tgt)), H.bits(src)) and np.array_equal(H.bits(H._np(eng.theta_pol)), H.bits(src))
    eng.theta_pol.copy_(keep_pol)
    eng.theta_tgt.copy_(keep_tgt)


# ---- prescribed-gradient trajectory
def run_trajectory(lib, device, steps=64):
    """Consecutive launches without teacher forcing: the engine's f32 state against the reference's own f64 state.  Each step's
    gradient is seeded and independent of theta, so errors add and do not amplify: at every step m, v, theta are within the SUM
    of the per-step bounds so far."""
    eng, pad = engine(lib, device, "d64")
    n = eng.net.n_trainable
    hp = Hyper()
    h32 = hp.f32()
    inp = H.synth_inputs(n, 900, pad=pad, k=1)
    rng = np.random.Generator(np.random.PCG64(901))
    scale = 10.0 ** rng.uniform(-8.0, 0.0, n) * (~inp["dead"])
    H.set_hyper(eng, hp, 10_000)
    eng.theta_pol[:n].copy_(torch.from_numpy(inp["theta"]))
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.step_counter.copy_(torch.tensor([0, 0, int(eng.step_counter[2]), 0], dtype=torch.int32))
    th, m, v = (inp["theta"].astype(np.float64), np.zeros(n), np.zeros(n))
    acc = [np.zeros(n), np.zeros(n), np.zeros(n)]
    worst = {"theta": 0.0, "m": 0.0, "v": 0.0}
    for k in range(1, steps + 1):
        g = (scale * rng.standard_normal(n)).astype(np.float32)
        g[rng.random(n) < 0.05] = 0.0
        eng.grad.copy_(torch.from_numpy(g))
        eng.recompute_gradnorm()
        eng.clip_adam()
        norm = float(eng.stats[1])
        want = H.ref_norm(g, 1.0)
        assert abs(norm - want) <= H.NORM_RTOL * want and int(eng.step_counter[1]) == k
        ref = H.ref_step(th, m, v, g, norm, k, h32)
        bnd = H.step_bounds(th, m, v, g, ref, norm, k, h32)
        got = (H._np(eng.theta_pol)[:n], H._np(eng.adam_m), H._np(eng.adam_v))
        for i, key in enumerate(("theta", "m", "v")):
            acc[i] += bnd[i]
            r = H.worst_ratio(got[i], ref[i], acc[i])
            worst[key] = max(worst[key], r)
            assert r <= 1.0, (k, key, r)
        th, m, v = ref
        eng.step_counter[0] = eng.step_counter[1]                    # what the weight-gradient launch of the next update does
    worst["steps"] = steps
    _report("trajectory", worst)


# ---- the launches in front of the optimizer
def run_reduce(lib, device):
    """dtqn_reduce_kernel: grad bit-equal to the f32 sum over the engine's own splits in split order, the norm partials, the zeroed
    tail, the published step count."""
    probe, _ = engine(lib, device, "sin48")
    batch = 2048 // probe.net.lp + 1
    eng, pad = engine(lib, device, "sin48", batch=batch)
    assert lib.dtqn_td_wgrad_is_direct(eng._net_ref, batch) == 0 and eng.n_split >= 1
    n, S = eng.net.n_trainable, eng.n_split
    rng = np.random.Generator(np.random.PCG64(31))
    gs = (10.0 ** rng.uniform(-8.0, 0.0, (S, n)) * rng.standard_normal((S, n))).astype(np.float32)
    eng.gsplit.copy_(torch.from_numpy(gs.reshape(-1)))
    eng.grad.fill_(-5.0)
    eng.norm_partial.fill_(7.0)
    eng.step_counter.copy_(torch.tensor([7, 41, 0, 0], dtype=torch.int32))
    assert lib.dtqn_td_reduce(eng._net_ref, eng._td_ref, eng._stream()) == 0
    want = np.zeros(n, dtype=np.float32)
    for s in range(S):
        want = want + gs[s]
    got = H._np(eng.grad)
    assert np.array_equal(H.bits(got), H.bits(want))
    r = H.check_norm_partials(H._np(eng.norm_partial), want, eng.n_norm_blocks, "reduce")
    sc = H._np(eng.step_counter)
    assert sc[0] == 41 and sc[1] == 41
    _report("reduce", {"partials": r, "n_split": S})


def run_gradnorm(lib, device, netname):
    eng, pad = engine(lib, device, netname)
    n = eng.net.n_trainable
    for seed, zero in ((51, False), (52, True)):
        inp = H.synth_inputs(n, seed, pad=pad, zero_grad=zero)
        eng.grad.copy_(torch.from_numpy(inp["g"]))
        eng.norm_partial.fill_(7.0)
        eng.recompute_gradnorm()
        p = H._np(eng.norm_partial)
        r = H.check_norm_partials(p, inp["g"], eng.n_norm_blocks, netname)
        if zero:
            assert not p.any()
        else:
            _report(f"gradnorm_{netname}", {"partials": r})


def run_xreduce(lib, device, world):
    """dtqn_xreduce_kernel in one process: `world` gradient buffers and flag words on the one device, every flag already at `gen`, so
    no block ever waits (own_flag NULL; a short time-out as a second safeguard)."""
    eng, pad = engine(lib, device, "d64")
    n = eng.net.n_trainable
    dev = eng.device
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rng = np.random.Generator(np.random.PCG64(60 + world))
    g = (10.0 ** rng.uniform(-8.0, 0.0, (world, n)) * rng.standard_normal((world, n))).astype(np.float32)
    gen = 5
    bufs = [torch.from_numpy(g[r]).to(dev) for r in range(world)]
    flags = torch.full((world,), gen, dtype=torch.int32, device=dev)
    gptr = torch.tensor([b.data_ptr() for b in bufs], dtype=torch.int64, device=dev)
    fptr = torch.tensor([flags.data_ptr() + 4 * r for r in range(world)], dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    gsum = torch.full((n,), -5.0, dtype=torch.float32, device=dev)
    eng.norm_partial.fill_(7.0)
    eng.td.xch_timeout_ms = 50
    try:
        assert lib.dtqn_td_xreduce(eng._net_ref, eng._td_ref, vp(gptr), vp(fptr), world, gen, vp(gsum), vp(status), None, eng._stream()) == 0
        got = H._np(gsum)
    finally:
        eng.td.xch_timeout_ms = 0
    want = np.zeros(n, dtype=np.float32)
    for r in range(world):
        want = want + g[r]
    assert int(status.item()) == 0 and (H._np(flags) == gen).all()
    assert np.array_equal(H.bits(got), H.bits(want))
    r = H.check_norm_partials(H._np(eng.norm_partial), want, eng.n_norm_blocks, f"xreduce{world}")
    _report(f"xreduce_world{world}", {"partials": r})


# ---- the bounds themselves, on the host: an independent f32 restatement stays inside them for the inputs of every case above
def host_case_inputs():
    """(name, n, k, hyper, synth kwargs) of every isolated-step case, without an engine."""
    n = 20000          # element-wise: the size adds nothing
    for k in STEP_KS:
        yield f"k{k}", n, 100 + k % 997, k, Hyper(), {}
    for clip in CLIPS:
        for regime in REGIMES:
            target = {"above_1e6": 1e6, "above_1e15": 1e15}.get(regime) or clip * REGIMES[regime]
            yield f"clip{clip}_{regime}", n, 300 + int(clip * 10), 5, Hyper(clip=clip), dict(scaled_norm=target)
    for gs in (1.0, 0.5, 0.125):
        for clipped in (False, True):
            yield f"gs{gs}_{clipped}", n, 500, 4, Hyper(grad_scale=gs), dict(scaled_norm=30.0 if clipped else 0.01)
    for lr, b, e in HYPERS:
        yield f"hyper_{lr}_{b}_{e}", n, 600, 7, Hyper(lr=lr, beta1=b[0], beta2=b[1], eps=e), {}
    for k in (1, 2):
        yield f"tiny_k{k}", n, 700 + k, k, Hyper(), dict(gmag=1e-20)
    yield "zero_grad_k6", n, 42, 6, Hyper(), dict(zero_grad=True)


def run_host_restatement():
    worst = {}
    for name, n, seed, k, hp, kw in host_case_inputs():
        h32 = hp.f32()
        inp = H.synth_inputs(n, seed, k=k, hp=h32, **kw)
        norm = float(np.float32(H.ref_norm(inp["g"], h32.grad_scale)))
        th, m, v = H.adam_f32_numpy(inp["theta"], inp["m"], inp["v"], inp["g"], norm, k, h32)
        r, _, _ = H.check_against_r32h(inp["theta"], inp["m"], inp["v"], inp["g"], norm, k, h32, th, m, v, what=name)
        worst[name] = r
    return worst
