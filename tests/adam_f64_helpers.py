"""float64 reference, derived bounds and an isolated-launch harness for the optimizer launches (dtqn_amd/csrc/dtqn_optim.hip), shared by
the CPU-emulation tests (test_emu_adam_f64.py), their -m gpu twins (test_gpu_adam_f64.py) and helpers.check_td_updates.

Reference: torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam.step on float64 CPU tensors.  clip_grad_norm_ is
get_total_norm + clip_grads_with_norm_ (torch/nn/utils/clip_grad.py); the two halves are called separately so that the ENGINE's
reported norm (stats[1]) feeds the reference's clip factor: the norm's summation error and the step's rounding are judged apart.

Two flavours of hyperparameters:
  R32h  the f32-rounded values the engine holds in DtqnTd (the C ABI carries floats): the kernel's contract, the tight bounds below;
  R64h  the exact Python doubles.  The kernel deviates from it by construction (1.0f - 0.999f is 1.3e-5 away from 0.001 in relative
        terms: visible in exp_avg_sq, nearly cancelled in theta).  Bound: 2 x |R32h - R64h| on the same inputs + the R32h bound.

Bounds are counts of f32 roundings times U = 2^-24 (the relative error of one rounding to nearest), written next to their use."""
from dataclasses import dataclass

import numpy as np
import torch

U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)          # smallest normal f32: absolute floor where a denormal may be flushed
NORM_RTOL = 2e-6                                 # < 24 dependent additions of positive terms + the square root: 25 U = 1.5e-6
OPT_BLOCK = 1024


@dataclass(frozen=True)
class Hyper:
    lr: float = 3e-4
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    clip: float = 1.0
    grad_scale: float = 1.0

    def f32(self):
        """What the engine holds after the C ABI rounded every field to float."""
        return Hyper(*(float(np.float32(x)) for x in (self.lr, self.beta1, self.beta2, self.eps, self.clip, self.grad_scale)))


def hyper_of(eng) -> Hyper:
    td = eng.td
    return Hyper(float(td.lr), float(td.beta1), float(td.beta2), float(td.eps), float(td.grad_norm_clip), float(td.grad_scale))


def set_hyper(eng, hp: Hyper, tuf=None):
    td = eng.td
    td.lr, td.beta1, td.beta2, td.eps, td.grad_norm_clip, td.grad_scale = hp.lr, hp.beta1, hp.beta2, hp.eps, hp.clip, hp.grad_scale
    if tuf is not None:
        td.target_update_frequency = int(tuf)


# --------------------------------------------------------------------------- #
# reference
# --------------------------------------------------------------------------- #
def ref_norm(g, grad_scale) -> float:
    """The total norm clip_grad_norm_ computes, of g * grad_scale, in float64."""
    return float(torch.nn.utils.get_total_norm([torch.from_numpy(np.asarray(g, dtype=np.float64)) * grad_scale]))


def clip_factor(norm: float, clip: float) -> float:
    return min(1.0, clip / (norm + 1e-6))


def ref_step(theta, m, v, g, norm, k, hp: Hyper):
    """One update in float64: clip with the given total norm, then torch.optim.Adam.step as step number k.
    Returns (theta, exp_avg, exp_avg_sq) as float64 arrays."""
    f64 = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))
    p = torch.nn.Parameter(f64(theta))
    p.grad = f64(g) * hp.grad_scale
    torch.nn.utils.clip_grads_with_norm_([p], hp.clip, torch.tensor(float(norm), dtype=torch.float64))
    opt = torch.optim.Adam([p], lr=hp.lr, betas=(hp.beta1, hp.beta2), eps=hp.eps)
    opt.state[p] = {"step": torch.tensor(float(k - 1)), "exp_avg": f64(m), "exp_avg_sq": f64(v)}
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == float(k)
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def step_bounds(theta_old, m_old, v_old, g, ref, norm, k, hp: Hyper, m_acc=None, v_acc=None):
    """Element-wise bounds of |kernel - reference| for one step, hp being the f32-rounded hyperparameters of both.
    m_acc / v_acc: the m and v bounds in force when theta's sensitivity is taken (default: this step's own)."""
    th_ref, m_ref, v_ref = ref
    gc = np.abs(np.asarray(g, dtype=np.float64) * (clip_factor(norm, hp.clip) * hp.grad_scale))
    # m = m + (g * coef - m) * (1 - b1): the product g * coef, the subtraction, the product, the sum; 1 - b1 is exact (Sterbenz).
    # (An active clip factor carries two roundings of its own, norm + 1e-6f and the quotient: they reach m weighted by 1 - b1 <= 0.2,
    # and the sum over all roundings is u [6 (1 - b1) |g'| + (1 + 3 (1 - b1)) |m|] <= 1.2 u |g'| + 1.6 u |m|: inside 4 U either way.)
    # U is the RELATIVE error of a rounding in the normal range only.  Below the smallest normal f32 a rounding is absolute (half of
    # 2^-149 with gradual underflow, the whole value where denormals are flushed): the operands m and g' flushed cost at most
    # b1 TINY + (1 - b1) TINY, the result flushed TINY more, so 2 TINY covers either denormal mode.  (A gradient of 1.4e-45, the
    # smallest subnormal, leaves m = 1.4e-46 in the reference and a correctly rounded 0 in f32: no relative bound holds there.)
    m_b = 4 * U * (np.abs(np.asarray(m_old, dtype=np.float64)) + gc) + 2 * TINY
    # v = v * b2 + (1 - b2) * g' * g': v * b2 (1), g * coef counted twice in the square (2), the two products (2), the sum (1): 6 U v.
    # That count takes the clip factor as exact.  It is when it is 1 (and grad_scale a power of two); an ACTIVE factor is
    # clip / (norm + 1e-6f): two more roundings, common to every element, doubled by the square -> 4 U on the (1 - b2) g'^2 term.
    # With v_old = 0 (k = 1) that term is all of v: the correct kernel reaches 6.6 U there, so the count of 6 alone was wrong.
    clipped = hp.clip / (norm + 1e-6) < 1.0 + 4 * U
    v_b = 6 * U * v_ref + (4 * U * (1.0 - hp.beta2) * gc * gc if clipped else 0.0) + TINY
    ma, va = (m_b if m_acc is None else m_acc), (v_b if v_acc is None else v_acc)
    bc1, bc2s = 1.0 - hp.beta1 ** k, np.sqrt(1.0 - hp.beta2 ** k)
    step_size = hp.lr / bc1
    # sensitivity of lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps) to m within +/- ma and v within +/- va: the two extreme quotients
    # (equal to the first-order term where that is valid, and still a bound where v is as small as its floor)
    am = np.abs(m_ref)
    q = am / (np.sqrt(v_ref) / bc2s + hp.eps)
    q_hi = (am + ma) / (np.sqrt(np.maximum(v_ref - va, 0.0)) / bc2s + hp.eps)
    q_lo = np.maximum(am - ma, 0.0) / (np.sqrt(v_ref + va) / bc2s + hp.eps)
    sens = step_size * np.maximum(q_hi - q, q - q_lo)
    # theta: the final subtraction rounds to half an ulp of the result; in the step: bc1 -> f32, lr / bc1, sqrt(bc2) -> f32, sqrtf(v),
    # / bc2_sqrt, + eps, m / denom, * step_size = 8 roundings, 12 allowed
    half_ulp = 0.5 * np.spacing(np.abs(th_ref).astype(np.float32)).astype(np.float64)
    th_b = half_ulp + 12 * U * np.abs(th_ref - np.asarray(theta_old, dtype=np.float64)) + sens
    return th_b, m_b, v_b


def adam_f32_numpy(theta, m, v, g, norm, k, hp: Hyper):
    """An independent plain-numpy float32 restatement of clip + Adam (the textbook form, not the kernel's): it must stay inside every
    bound against R32h before anything is asked of the device."""
    f = np.float32
    b1, b2 = f(hp.beta1), f(hp.beta2)
    coef = min(f(1.0), f(hp.clip) / (f(norm) + f(1e-6))) * f(hp.grad_scale)
    gc = np.asarray(g, dtype=f) * f(coef)
    m = np.asarray(m, dtype=f) * b1 + (f(1.0) - b1) * gc
    v = np.asarray(v, dtype=f) * b2 + (f(1.0) - b2) * (gc * gc)
    bc1, bc2 = f(1.0 - float(b1) ** k), f(1.0 - float(b2) ** k)
    mhat, vhat = m / bc1, v / bc2
    theta = np.asarray(theta, dtype=f) - f(hp.lr) * (mhat / (np.sqrt(vhat) + f(hp.eps)))
    return theta, m, v


def worst_ratio(got, ref, bound) -> float:
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(np.asarray(got, dtype=np.float64) - ref) / bound
    r = np.where(np.abs(np.asarray(got, dtype=np.float64) - ref) == 0.0, 0.0, r)       # 0 / 0: exact where nothing is allowed
    return float(r.max()) if r.size else 0.0


def check_against_r32h(theta_old, m_old, v_old, g, norm, k, hp: Hyper, got_theta, got_m, got_v, what=""):
    """Assert one step's theta, m, v within the bounds of R32h (hp: the engine's own f32-rounded hyperparameters); the worst
    error / bound of each."""
    ref = ref_step(theta_old, m_old, v_old, g, norm, k, hp)
    th_b, m_b, v_b = step_bounds(theta_old, m_old, v_old, g, ref, norm, k, hp)
    r = {"theta": worst_ratio(got_theta, ref[0], th_b), "m": worst_ratio(got_m, ref[1], m_b), "v": worst_ratio(got_v, ref[2], v_b)}
    assert r["m"] <= 1.0, (what, "adam_f64: exp_avg outside 4 U (|m| + |g coef|) + 2 tiny", r)
    assert r["v"] <= 1.0, (what, "adam_f64: exp_avg_sq outside 6 U v (+ 4 U (1 - b2) g'^2 when clipped) + tiny", r)
    assert r["theta"] <= 1.0, (what, "adam_f64: theta outside half an ulp + 12 U |step| + sensitivity", r)
    return r, ref, (th_b, m_b, v_b)


# --------------------------------------------------------------------------- #
# synthetic inputs
# --------------------------------------------------------------------------- #
def synth_inputs(n, seed, *, pad=None, k=2, hp: Hyper = Hyper(), scaled_norm=None, gmag=None, zero_grad=False):
    """Seeded inputs of one isolated step.  Per-element scales log-uniform over eight decades; the gradient is scale * N(0, 1) with
    about 5 % exact zeros; m, v are what three float64 Adam steps on gradients of the same scales leave (zeros for k = 1); theta spans
    1e-3 .. 1e1.  About 1 % of the elements, and the width padding `pad`, hold exact zeros in g, m, v (theta 0 in the padding).
    scaled_norm: rescale g so that ||g|| * grad_scale is this value.  gmag: every non-zero |g| is this value (eps-dominated case)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    scale = 10.0 ** rng.uniform(-8.0, 0.0, n)
    dead = rng.random(n) < 0.01
    if pad is not None:
        dead |= pad
    g = scale * rng.standard_normal(n)
    if gmag is not None:
        g = np.sign(g) * gmag
    g[rng.random(n) < 0.05] = 0.0
    g[dead] = 0.0
    if zero_grad:
        g[:] = 0.0
    if scaled_norm is not None:
        g *= scaled_norm / (ref_norm(g.astype(np.float32), hp.grad_scale))
        g *= scaled_norm / (ref_norm(g.astype(np.float32), hp.grad_scale))      # once more after the rounding to f32
    m, v = np.zeros(n), np.zeros(n)
    if k > 1:
        s = (gmag if gmag is not None else scale) * (~dead)
        for t in range(1, 4):
            gt = s * rng.standard_normal(n)
            _, m, v = ref_step(np.zeros(n), m, v, gt, 0.0, t, hp)
    theta = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3.0, 1.0, n)
    if pad is not None:
        theta[pad] = 0.0
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"theta": f(theta), "m": f(m), "v": f(v), "g": f(g), "dead": dead}


# --------------------------------------------------------------------------- #
# isolated launches
# --------------------------------------------------------------------------- #
def _np(t):
    return t.detach().cpu().numpy().copy()


def block_sumsq(g, n_blocks):
    """float64 sums of squares of the optimizer blocks (1024 elements each)."""
    sq = np.zeros(n_blocks * OPT_BLOCK)
    sq[:g.size] = np.asarray(g, dtype=np.float64) ** 2
    return sq.reshape(n_blocks, OPT_BLOCK).sum(1)


def check_norm_partials(partials, g, n_blocks, what=""):
    """partials[b] within the norm bound of the float64 block sums (as norms: the relative error of a square root is half that of
    its argument), the tail beyond the grid zero."""
    want = np.sqrt(block_sumsq(g, n_blocks))
    got = np.sqrt(partials[:n_blocks].astype(np.float64))
    assert (np.abs(got - want) <= NORM_RTOL * want).all(), (what, float(np.abs(got / np.where(want > 0, want, 1) - 1).max()))
    assert not partials[n_blocks:].any(), (what, "norm_partial behind the grid is not zero")
    d = np.abs(got - want)[want > 0] / (NORM_RTOL * want[want > 0])
    return float(d.max()) if d.size else 0.0


def launch_step(eng, inp, k, hp: Hyper, tuf, *, poisoned=False, theta_tgt=None):
    """Write the inputs of one optimizer step into the engine, run dtqn_td_gradnorm + dtqn_td_clip_adam, return everything they left."""
    n = eng.net.n_trainable
    eng.grad.copy_(torch.from_numpy(inp["g"]))
    eng.adam_m.copy_(torch.from_numpy(inp["m"]))
    eng.adam_v.copy_(torch.from_numpy(inp["v"]))
    eng.theta_pol[:n].copy_(torch.from_numpy(inp["theta"]))
    if theta_tgt is not None:
        eng.theta_tgt.copy_(torch.from_numpy(theta_tgt))
    # the kernel takes k = step_counter[0] + 1; in an update the weight-gradient launch publishes [0], here the test does
    eng.step_counter.copy_(torch.tensor([k - 1, k - 1, int(eng.step_counter[2]), 1 if poisoned else 0], dtype=torch.int32))
    set_hyper(eng, hp, tuf)
    eng.norm_partial.fill_(7.0)                                   # sentinel: the launch owns every entry
    before = {"theta_pol": _np(eng.theta_pol), "theta_tgt": _np(eng.theta_tgt), "sc": _np(eng.step_counter)}
    eng.recompute_gradnorm()
    partials = _np(eng.norm_partial)
    eng.clip_adam()
    out = {"theta_pol": _np(eng.theta_pol), "theta_tgt": _np(eng.theta_tgt), "m": _np(eng.adam_m), "v": _np(eng.adam_v),
           "stats": _np(eng.stats), "sc": _np(eng.step_counter), "partials": partials, "before": before}
    out["ring"] = eng.stats_ring_np[(int(out["sc"][2]) - 1) % eng.RING_SLOTS].copy()
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_step(eng, inp, out, k, hp: Hyper, tuf, *, what="", check_norm=True, r64: Hyper = None):
    """Everything one applied step leaves, against R32h (and R64h where r64 gives the exact doubles).  hp: as set on the engine."""
    n = eng.net.n_trainable
    hp = hp.f32()
    st, sc, before = out["stats"], out["sc"], out["before"]
    norm = float(st[1])
    ratios = {}
    if check_norm:
        ratios["partials"] = check_norm_partials(out["partials"], inp["g"], eng.n_norm_blocks, what)
        want = ref_norm(inp["g"], hp.grad_scale)
        assert abs(norm - want) <= NORM_RTOL * want, (what, norm, want)
        ratios["norm"] = abs(norm - want) / (NORM_RTOL * want) if want > 0 else 0.0
    # the clip factor as reported: norm + 1e-6f, the quotient, the minimum: 2 roundings (+ 1e-6f against 1e-6: 1e-6 U relative), 3 allowed
    cf = clip_factor(norm, hp.clip)
    assert abs(float(st[8]) - cf) <= 3 * U * cf, (what, float(st[8]), cf)
    sync = tuf > 0 and k % tuf == 0
    assert st[9] == float(k) and st[10] == (1.0 if sync else 0.0) and st[11] == 0.0, (what, st[9:12])
    assert sc[0] == k - 1 and sc[1] == k and sc[2] == before["sc"][2] + 1 and sc[3] == 0, (what, sc)
    # the host ring: twelve {value, tag = call index} granules, the values of stats[]
    assert (out["ring"][:, 1] == np.float32(sc[2])).all() and np.array_equal(bits(out["ring"][:, 0]), bits(st)), (what, out["ring"])
    r, ref, bnd = check_against_r32h(inp["theta"], inp["m"], inp["v"], inp["g"], norm, k, hp, out["theta_pol"][:n], out["m"], out["v"], what)
    ratios.update(r)
    if r64 is not None:
        # the distance between the two references on these inputs, computed on the host, times 2, plus the R32h bound
        ref64 = ref_step(inp["theta"], inp["m"], inp["v"], inp["g"], norm, k, r64)
        for i, (name, got) in enumerate((("theta", out["theta_pol"][:n]), ("m", out["m"]), ("v", out["v"]))):
            dist = np.abs(ref64[i] - ref[i])
            rr = worst_ratio(got, ref64[i], 2.0 * dist + bnd[i])
            assert rr <= 1.0, (what, "adam_f64: outside the R64h bound", name, rr)
            ratios["r64_" + name] = rr
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(ref64[i] != 0, dist / np.abs(ref64[i]), 0.0)
            ratios["r32h_r64h_rel_" + name] = float(rel.max())
    # exact zeros stay exact zeros (width padding and the dead elements): nothing moves where g = m = v = 0
    dead = inp["dead"]
    assert not out["m"][dead].any() and not out["v"][dead].any(), what
    assert np.array_equal(bits(out["theta_pol"][:n][dead]), bits(inp["theta"][dead])), what
    # the frozen tail (sinusoidal positions) is nobody's to write; the target moves only at a hard sync, and only its trainable part
    assert np.array_equal(bits(out["theta_pol"][n:]), bits(before["theta_pol"][n:])), what
    assert np.array_equal(bits(out["theta_tgt"][n:]), bits(before["theta_tgt"][n:])), what
    if sync:
        assert np.array_equal(bits(out["theta_tgt"][:n]), bits(out["theta_pol"][:n])), what
    else:
        assert np.array_equal(bits(out["theta_tgt"]), bits(before["theta_tgt"])), what
    return ratios


def run_case(eng, seed, k, hp: Hyper = Hyper(), tuf=10_000, *, pad=None, what="", r64=False, **synth):
    """One isolated step from synthetic inputs, checked; returns the worst error / bound figures."""
    assert eng.net.n_trainable % 4 == 0, "the float4 loads of the optimizer launches rely on it"
    inp = synth_inputs(eng.net.n_trainable, seed, pad=pad, k=k, hp=hp.f32(), **synth)
    out = launch_step(eng, inp, k, hp, tuf)
    return check_step(eng, inp, out, k, hp, tuf, what=what, r64=hp if r64 else None, check_norm=synth.get("gmag") is None), inp, out
