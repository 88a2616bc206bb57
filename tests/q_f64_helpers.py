"""Q-values of a kernel against the oracle's float64 evaluation, row by row (docs/q_f64_tests.md).

The flat comparison `max |Q - ref| <= 1e-4 * max(1, |Q|max)` measures every entry of a Q tensor against the fp32 oracle and against the
single largest entry of the whole tensor; at init-scale weights (|Q| < 1) it is an absolute 1e-4, three to four orders of magnitude
above what a correct forward achieves.  Here every row (b, t) -- the A values of one time step -- is measured at its OWN scale against
the float64 forward, and the bound is what the fp32 oracle itself achieves on the same inputs (D32), times one margin for the whole
suite.  `scale=1.0` is the same yardstick for rows of probabilities (rows that sum to 1)."""
import json
import os
import time

import numpy as np
import torch

from oracle import dtqn_oracle as O

from grad_f64_helpers import U32

# One floor and one margin for the whole suite; how they were chosen and the measured ratios: docs/q_f64_tests.md.
PHI = 2.0 ** -4
MARGIN = 16.0
D32_CEILING = 2.0 ** -8    # see check_q_f64: beyond it the two oracle evaluations are not the same function of the same inputs

TOTALS = [0.0, 0]         # seconds spent in / number of Q checks (the float64 forwards of the standalone sites included), this process


def row_scales(q64, phi=PHI):
    """[B, n]: s[b, t] = max(max_a |q64[b, t]|, phi * max_{t', a} |q64[b]|) -- the floor is per sequence, so that one loud sequence
    does not loosen the rows of the others."""
    a = np.abs(q64)
    return np.maximum(a.max(axis=2), phi * a.max(axis=(1, 2))[:, None])


def _log(what, fig):
    """DTQN_Q64_LOG=<file>: one JSON line per check (the measurement runs behind the tables of docs/q_f64_tests.md)."""
    path = os.environ.get("DTQN_Q64_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"what": repr(what), "test": os.environ.get("PYTEST_CURRENT_TEST", ""), **fig}) + "\n")


def check_q_f64(got, q64, q32, what=None, assert_=True, margin=MARGIN, phi=PHI, rows=None, scale=None, ref_seconds=0.0, d32_floor=0.0, log=True):
    """got, q64, q32: [B, n, A] of the kernel, the float64 and the fp32 oracle on the same inputs.  Every row of `got` within
    margin * D32 * s of the float64 row, s = row_scales(q64), D32 = the worst such distance of the fp32 oracle over the rows of this
    check (not below 2^-24).  rows: boolean [B, n], the rows of `got` that are compared (an actor leaves only the newest one); D32 is
    taken over every row the oracle has.  scale: a fixed row scale instead of row_scales (1.0: rows of probabilities).
    d32_floor: the D32 of the other checks of the same site (check_pooled_f64): a maximum over a handful of rows is a noisy yardstick.
    -> figures: D32, engine / D32, engine / bound, the worst row (b, t), n, the largest asserted absolute bound."""
    t0 = time.perf_counter()
    q64, q32, got = np.asarray(q64), np.asarray(q32), np.asarray(got)
    assert q64.dtype == np.float64, ("the reference of the Q check is not float64", what, q64.dtype)
    assert q64.ndim == 3 and got.shape == q64.shape == q32.shape, (what, got.shape, q64.shape, q32.shape)
    rows = np.ones(q64.shape[:2], dtype=bool) if rows is None else np.asarray(rows, dtype=bool)
    assert rows.shape == q64.shape[:2] and rows.any(), (what, rows.shape)
    assert np.isfinite(q64).all() and np.isfinite(q32).all(), ("non-finite reference row", what)
    assert np.isfinite(got[rows]).all(), ("non-finite row", what, np.argwhere(~np.isfinite(got).all(axis=2) & rows)[:4].tolist())
    s = row_scales(q64, phi) if scale is None else np.full(q64.shape[:2], float(scale))
    assert (s > 0).all(), ("a sequence whose float64 Q is zero altogether", what)
    e32 = np.abs(q32.astype(np.float64) - q64).max(axis=2) / s
    d32 = max(float(e32.max()), U32, d32_floor)
    eng = np.where(rows, np.abs(np.where(rows[..., None], got, 0).astype(np.float64) - q64).max(axis=2) / s, 0.0)
    b, t = np.unravel_index(int(eng.argmax()), eng.shape)
    fig = {"d32": d32, "d32_row": [int(i) for i in np.unravel_index(int(e32.argmax()), e32.shape)], "rel_err": float(eng[b, t]),
           "row": [int(b), int(t)], "n": int(q64.shape[1]), "over_d32": float(eng[b, t] / d32), "over_bound": float(eng[b, t] / (margin * d32)),
           "abs_bound": float(margin * d32 * s[rows].max()), "abs_err": float(np.abs(got.astype(np.float64) - q64)[rows].max()),
           "q_abs_max": float(np.abs(q64).max()), "rows": int(rows.sum())}
    if log:
        _log(what, dict(fig, seconds=ref_seconds + time.perf_counter() - t0))       # (ref_seconds: the references of a standalone forward)
    fig["row_bound"] = margin * d32 * s            # [B, n]: the asserted bound of every row (the statistics inherit it: check_stats_f64)
    # the fp32 oracle passes its own check at margin / 2 by construction (D32 is its worst row).  What can go wrong is the pair itself: a
    # float64 evaluation of other inputs or parameters puts D32 near 1 and would wave everything through.  float32 carries 24 bits; a
    # pair that agrees to fewer than 8 of them (the worst-conditioned family of the suite, GRU + identity at D 128, keeps 11) is no yardstick
    assert (e32 <= 0.5 * margin * d32).all() and float(e32.max()) <= D32_CEILING, ("the fp32 and float64 oracle disagree", what, fig)
    if assert_:
        bad = np.argwhere(eng > margin * d32)
        assert not len(bad), ("Q rows beyond margin * D32 of the float64 forward [b, t, error / s, error / D32]", what, fig,
                              [(int(i), int(j), float(eng[i, j]), float(eng[i, j] / d32)) for i, j in bad[:8]])
    TOTALS[0] += time.perf_counter() - t0
    TOTALS[1] += 1
    return fig


def check_stats_f64(got, ref64, q_h64, t_h64, qt64, bq, bt, gamma, batch, history, what=None, assert_=True):
    """The statistics of one TD update against the float64 evaluation, within bounds that follow from the row bounds of the Q check and
    the float32 arithmetic of the loss and statistics kernels (derivation: docs/q_f64_tests.md).
    got / ref64: {name: value} of the engine and of oracle.td_forward in float64; q_h64, t_h64 [B, history]: the float64 selected Q and
    targets of the loss rows; qt64: the float64 target-network Q the targets were built from; bq, bt [B, history]: the row bounds
    (check_q_f64 row_bound) of q_all and q_next_tgt on the loss rows.  -> {name: |got - ref| / bound}, {name: bound}."""
    u = 2.0 ** -23                                  # one ulp: twice the rounding unit, which covers the second-order terms
    q, y, qt = (np.asarray(a, dtype=np.float64) for a in (q_h64, t_h64, qt64))
    assert q.shape == y.shape == qt.shape == bq.shape == bt.shape == (batch, history), (q.shape, bq.shape, batch, history)
    # y = fl(r + (1 - done) fl(q_tgt gamma32)): the element bound of q_tgt, gamma rounded to float32, two roundings
    by = gamma * bt + (abs(float(np.float32(gamma)) - gamma) + u) * np.abs(qt) + u * np.abs(y)
    d = q - y
    bd = bq + by + u * np.abs(d)                    # diff = fl(q - y)
    # a sum of batch * history terms: <= ceil(history / 64) adds in a lane, a 6-level wave butterfly per sequence (td_loss_wave), then
    # <= ceil(4 batch / 256) adds in a thread, a 6-level butterfly and 4 waves in index order (the statistics block of dtqn_optim.hip),
    # one division: every term passes through at most K roundings, each relative to a partial sum of absolute values
    K = -(-history // 64) + 6 + -(-4 * batch // 256) + 6 + 3 + 1
    mean_of = lambda x, b: float(b.mean() + K * u * (np.abs(x) + b).mean())
    bounds = {"qvalue_max": float(bq.max()), "qvalue_min": float(bq.max()), "target_max": float(by.max()), "target_min": float(by.max()),
              "qvalue_mean": mean_of(q, bq), "target_mean": mean_of(y, by),
              "td_error": float((bd * (2.0 * np.abs(d) + bd)).mean() + (K + 1) * u * ((np.abs(d) + bd) ** 2).mean())}
    over = {k: abs(float(got[k]) - float(ref64[k])) / b for k, b in bounds.items()}
    _log(what, {"stats_over_bound": over, "stats_bound_over_flat": {k: b / (2e-4 * max(1.0, abs(float(ref64[k])))) for k, b in bounds.items()}})
    if assert_:
        bad = {k: (float(got[k]), float(ref64[k]), bounds[k]) for k, v in over.items() if not v <= 1.0}
        assert not bad, ("statistics beyond the bound derived from the row bounds (engine, float64, bound)", what, bad)
    return over, bounds


def widen(t):
    """float32 tensor -> float64, exactly; everything else as it is (td_gradients64 widens the same way)."""
    return t.double() if torch.is_tensor(t) and t.dtype == torch.float32 else t


def oracle_q(cfg: O.NetCfg, params, obs, act, bag=None):
    """(q32, q64) [B, n, A]: O.forward on the float32 parameters, and on the same parameters, positions table and inputs widened
    exactly.  obs: [B, n, O] (tokens, integers where cfg.discrete) or [B, n, C, H, W] pixels; act: [B, n] or [B, n, 1];
    bag: (bag_obs [B, m, O], bag_act [B, m(, 1)]) for a bag network."""
    Bn, n = obs.shape[:2]
    integer = cfg.discrete and cfg.image is None
    as_obs = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.long) if integer else torch.as_tensor(np.asarray(a, dtype=np.float32))
    o = as_obs(obs)
    a = None if act is None else torch.as_tensor(np.asarray(act).astype(np.int64)).reshape(Bn, n, 1)
    kw32, kw64 = {}, {}
    if bag is not None:
        bo, ba = as_obs(bag[0]), torch.as_tensor(np.asarray(bag[1]).astype(np.int64)).reshape(Bn, -1, 1)
        kw32, kw64 = dict(bag_obss=bo, bag_actions=ba), dict(bag_obss=widen(bo), bag_actions=ba)
    with torch.no_grad():
        q32 = O.forward(params, cfg, o, a, **kw32).numpy()
        q64 = O.forward({k: widen(v) for k, v in params.items()}, cfg, widen(o), a, **kw64).numpy()
    return q32, q64


def check_pooled_f64(pool, assert_=True):
    """pool: [(got, q64, q32, rows, what, seconds)] left by check_forward_f64(..., pool=pool) -- the checks of one site (every environment
    of a round, every context length of a case).  D32 is taken over the rows of ALL of them: the checks of such a site hold one to
    three rows each, and a maximum over so few rows varies by 20 to 40 x between draws (docs/q_f64_tests.md).  -> the figures of every check."""
    assert pool
    own = [check_q_f64(got, q64, q32, what=what, assert_=False, rows=rows, log=False)["d32"] for got, q64, q32, rows, what, _ in pool]
    return [check_q_f64(got, q64, q32, what=what, assert_=assert_, rows=rows, ref_seconds=sec, d32_floor=max(own))
            for got, q64, q32, rows, what, sec in pool]


def check_forward_f64(cfg: O.NetCfg, params, obs, act, got, bag=None, rows=None, what=None, assert_=True, pool=None):
    """A standalone forward's Q `got` [B, n, A] against the float64 evaluation of the oracle on the same inputs (one float64 forward
    per call).  rows: see check_q_f64; `got` may be [B, A] with rows=None: the newest row of every sequence (an actor's output).
    pool: a list that collects the check instead of asserting it; check_pooled_f64(pool) then asserts the site as a whole."""
    t0 = time.perf_counter()
    q32, q64 = oracle_q(cfg, params, obs, act, bag)
    got = np.asarray(got)
    if got.ndim == 2:
        full = np.zeros(q64.shape, dtype=got.dtype)
        full[:, -1] = got
        rows = np.zeros(q64.shape[:2], dtype=bool)
        rows[:, -1] = True
        got = full
    TOTALS[0] += time.perf_counter() - t0
    if pool is not None:
        pool.append((got, q64, q32, rows, what, time.perf_counter() - t0))
        return None
    return check_q_f64(got, q64, q32, what=what, assert_=assert_, rows=rows, ref_seconds=time.perf_counter() - t0)


__all__ = ["PHI", "MARGIN", "TOTALS", "row_scales", "check_q_f64", "check_stats_f64", "check_forward_f64", "check_pooled_f64", "D32_CEILING", "oracle_q", "widen"]
