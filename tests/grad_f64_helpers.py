"""Gradients of a kernel against the oracle's float64 evaluation, tensor by tensor and group by group (docs/grad_f64_tests.md).

The flat comparison of helpers.check_td_updates measures every entry against the single largest entry of the whole gradient, which
leaves the small tensors (biases, gates) and every small entry unobserved.  Here every tensor -- and, where the rows of a tensor have
scales of their own, every group of rows -- is measured at its OWN scale against the float64 gradient, and the bound is what the
fp32 oracle itself achieves on the same inputs (D32), times one margin for the whole suite."""
import numpy as np

from dtqn_amd import _binding as B
from oracle import dtqn_oracle as O

from helpers import unpack_flat

# One floor and one margin for the whole suite; how they were chosen and the measured ratios: docs/grad_f64_tests.md.
PHI = 2.0 ** -4
MARGIN = 16.0
U32 = 2.0 ** -24          # a correctly rounded float32 result is already this far (relatively) from the float64 one: the floor of D32

TOTALS = [0.0, 0]         # seconds spent in / number of float64 evaluations + checks, this process


def groups_of(cfg: O.NetCfg, key: str, shape):
    """[(group name, index into the reference-shaped tensor, selected)]: the parts of one tensor whose gradients have scales of their
    own.  selected: the group is a row that receives a term only when the batch selects it (a token, an action, a position), so a
    gradient of exactly zero means that no term exists; the other groups are sums over every token, where zero is a cancellation."""
    if key == "position_embedding.position_encoding":                                        # [1, L, D]: per position
        return [(f"{key}[pos {i}]", (0, i), True) for i in range(shape[1])]
    if key == "action_embedding.embedding.0.weight":                                         # [A, a]: per (previous) action
        return [(f"{key}[action {i}]", (i,), True) for i in range(shape[0])]
    if cfg.discrete and cfg.image is None and key == "obs_embedding.observation_embedding.0.weight":     # [V, e]: per vocabulary row
        return [(f"{key}[token {i}]", (i,), True) for i in range(shape[0])]
    if cfg.discrete and cfg.image is None and key == "obs_embedding.observation_embedding.2.weight":     # [D, O e]: per observation slot
        e = cfg.embed_per_obs_dim
        return [(f"{key}[slot {j}]", (slice(None), slice(j * e, (j + 1) * e)), False) for j in range(cfg.obs_dim)]
    if key.endswith("in_proj_weight") or key.endswith("in_proj_bias"):                        # [3 D, ...]: the q, k and v thirds
        D = shape[0] // 3
        return [(f"{key}[{n}]", (slice(i * D, (i + 1) * D),), False) for i, n in enumerate("qkv")]
    if key in ("ffn.2.weight", "ffn.2.bias"):                                                # the head's last layer: per action
        return [(f"{key}[action {i}]", (i,), True) for i in range(shape[0])]
    return [(key, (), False)]                   # everything else, the shared GRU gate tensors (sum over layers) included: one tensor


def scaled(err_max, ref_max, tmax, phi=PHI):
    """(error / s, s) with s = max(group max, phi * tensor max) of the float64 value: the one scale rule of every float64 check
    (scalars or arrays of groups; image_encoder_helpers.py applies it to feature maps and per-tap gradient tiles)."""
    s = np.maximum(ref_max, phi * tmax)
    return err_max / s, s


def group_errors(cfg: O.NetCfg, got, g64, phi=PHI):
    """got, g64: {trainable key: reference-shaped array}.  -> ({group: max |got - g64| / s}, {group: s}, [structural-zero groups
    in which `got` has a non-zero entry]) with s = max(group max, phi * tensor max) of g64.  A selected row (groups_of) whose float64
    gradient is exactly zero is structural (a token no window holds, an action no loss row selects, a position behind the rows given)
    and carries no error figure: it must be exactly zero; so must a tensor that is zero altogether.  A sum group that is exactly zero in
    float64 inside a non-zero tensor (the q and k thirds of a one-row sequence, whose softmax is the constant 1: torch subtracts a number
    from itself, the kernels subtract dO . O from dP . 1) is measured at the floor like any other cancellation."""
    errs, scales, nonzero = {}, {}, []
    for key in O.trainable_keys(cfg):
        ref = np.asarray(g64[key], dtype=np.float64)
        have = np.asarray(got[key], dtype=np.float64)
        assert have.shape == ref.shape, (key, have.shape, ref.shape)
        tmax = float(np.abs(ref).max())
        for name, idx, selected in groups_of(cfg, key, ref.shape):
            r, h = ref[idx], have[idx]
            gmax = float(np.abs(r).max())
            if gmax == 0.0 and (selected or tmax == 0.0):
                if np.any(h != 0.0):
                    nonzero.append((name, int(np.count_nonzero(h)), float(np.abs(h).max())))
                continue
            e, s = scaled(float(np.abs(h - r).max()), gmax, tmax, phi)
            errs[name], scales[name] = float(e), float(s)
    return errs, scales, nonzero


def check_gradient_f64(cfg: O.NetCfg, net, got_flat, g64, g32, margin=MARGIN, phi=PHI, what=None, assert_=True):
    """got_flat: the engine's flat gradient (engine layout); g64 / g32: {key: tensor} of the float64 and the fp32 oracle, all three
    under the same ReLU masks and argmax choices.  Every group of the engine within margin * D32 of the float64 gradient at the group's
    scale, D32 = the worst such distance of the fp32 oracle over the groups of this case; exactly 0.0 where float64 is zero by structure.
    -> figures: D32, the worst relative error, engine / D32, engine / bound, and the group that set them."""
    keys = O.trainable_keys(cfg)
    n64 = {k: g64[k].detach().numpy() for k in keys}
    assert all(v.dtype == np.float64 for v in n64.values())
    got = unpack_flat(net, np.asarray(got_flat), keys)
    e32, _, z32 = group_errors(cfg, {k: g32[k].detach().numpy() for k in keys}, n64, phi)
    eng, scales, zeng = group_errors(cfg, got, n64, phi)
    d32 = max(max(e32.values()), U32)
    worst = max(eng, key=eng.get)
    fig = {"d32": d32, "d32_group": max(e32, key=e32.get), "rel_err": eng[worst], "group": worst, "over_d32": eng[worst] / d32,
           "over_bound": eng[worst] / (margin * d32), "groups": len(eng), "zero_groups": sum(len(groups_of(cfg, k, n64[k].shape)) for k in keys) - len(eng)}
    if assert_:
        assert not z32, ("the fp32 oracle is non-zero in a group whose float64 gradient is exactly zero", what, z32)
        assert not zeng, ("non-zero gradient in a group whose float64 gradient is exactly zero", what, zeng)
        bad = {g: (e, e / d32) for g, e in eng.items() if e > margin * d32}
        assert not bad, ("gradient groups beyond margin * D32 of the float64 gradient (error / s, error / D32)", what, fig, bad)
    else:
        fig["nonzero_in_zero_groups"] = zeng
    return fig


__all__ = ["PHI", "MARGIN", "U32", "scaled", "groups_of", "group_errors", "check_gradient_f64", "TOTALS"]
