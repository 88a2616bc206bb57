"""The distribution of the device sampler, tested once, on oracle/sampler_oracle.py alone (numpy, no library): the kernels and the
emulation are held bit-equal to that oracle in test_emu_sampler.py / test_gpu_sampler.py, so what holds here holds for them.

Target (the reference buffer's sample / sample_with_bag): episode uniform over [0, n_valid) minus `exclude`; start uniform on
0 .. max(0, len - L) given the episode; bag a uniform bag_size-subset of the rows below the window.  Inputs: sampler_cases.py, named
before anything ran.  Condition: every test below has p >= 1e-4 at every named seed.  Each test is ONE chi-square statistic with one
p-value, except the per-row and per-pair inclusion frequencies of (e) and (f): those are m binomial counts (m = 7, 40 and 780), each
with a two-sided normal-approximation p-value (z^2 against chi-square with 1 degree of freedom; the smallest expected count is 1 148),
combined into one p-value by Bonferroni, min(1, m * min p) -- valid whatever the dependence between the counts, which share their
total.  The p-values of every statistic are printed (pytest -s) and tabulated in docs/sampler_tests.md."""
import functools
import itertools

import numpy as np
import pytest
from scipy.stats import chi2

from oracle import sampler_oracle as S

import sampler_cases as C


def gof(observed, expected):
    """Pearson goodness of fit against a fully specified pmf: (statistic, degrees of freedom, p)."""
    observed, expected = np.asarray(observed, dtype=np.float64).ravel(), np.asarray(expected, dtype=np.float64).ravel()
    assert abs(observed.sum() - expected.sum()) < 1e-6 * expected.sum() and expected.min() >= 5
    stat = float(((observed - expected) ** 2 / expected).sum())
    return stat, observed.size - 1, float(chi2.sf(stat, observed.size - 1))


def independence(table):
    """Pearson test of independence of a two-way table, margins estimated: (statistic, degrees of freedom, p)."""
    table = np.asarray(table, dtype=np.float64)
    expected = np.outer(table.sum(1), table.sum(0)) / table.sum()
    assert expected.min() >= 5
    stat = float(((table - expected) ** 2 / expected).sum())
    df = (table.shape[0] - 1) * (table.shape[1] - 1)
    return stat, df, float(chi2.sf(stat, df))


def bonferroni(counts, n, p):
    """m binomial(n, p) counts -> (largest |z|, m, min(1, m * smallest two-sided p))."""
    counts = np.asarray(counts, dtype=np.float64).ravel()
    z = (counts - n * p) / np.sqrt(n * p * (1 - p))
    return float(np.abs(z).max()), counts.size, float(min(1.0, counts.size * chi2.sf(z ** 2, 1).min()))


def report(name, seed, fig):
    print(f"sampler-stat {name} seed={seed:#x} stat={fig[0]:.3f} df={fig[1]} p={fig[2]:.4f}")
    assert fig[2] >= C.P_MIN, (name, seed, fig)


LIVE = [e for e in range(C.STAT_N_VALID) if e != C.STAT_EXCLUDE]
SPAN = np.maximum(np.asarray(C.STAT_EP_LEN) - C.STAT_L, 0) + 1


@functools.lru_cache(maxsize=None)
def windows(seed):
    """(episode, start) [steps][batch] of every update of the run."""
    step, b = np.arange(C.STAT_STEPS)[:, None], np.arange(C.STAT_BATCH)[None, :]
    e, s = S.window_draw(C.STAT_EP_LEN, C.STAT_N_VALID, C.STAT_EXCLUDE, C.STAT_L, seed, step, b)
    assert e.shape == s.shape == (C.STAT_STEPS, C.STAT_BATCH)
    e.setflags(write=False); s.setflags(write=False)
    return e, s


@functools.lru_cache(maxsize=None)
def bags(seed, which):
    start, bag = C.STAT_BAGS[which]
    rows = S.bag_rows(seed, np.arange(C.STAT_BAG_STEPS)[:, None], np.arange(C.STAT_BATCH)[None, :], start, bag).reshape(-1, bag)
    rows.setflags(write=False)
    return rows


def test_the_inputs_are_the_ones_named():
    assert len(C.STAT_EP_LEN) == C.STAT_N_VALID and int(SPAN[LIVE].sum()) == 59
    assert C.STAT_STEPS * C.STAT_BATCH == 128_000 and int(128_000 / len(LIVE) / SPAN[LIVE].max()) == 556
    assert C.STAT_BAG_STEPS * C.STAT_BATCH == 32_000


@pytest.mark.parametrize("seed", C.STAT_SEEDS)
def test_a_joint_table_of_episode_and_start(seed):
    e, s = windows(seed)
    assert not (e == C.STAT_EXCLUDE).any() and e.min() >= 0 and e.max() < C.STAT_N_VALID and s.min() >= 0 and (s < SPAN[e]).all()
    observed, expected = [], []
    for ep in LIVE:
        observed += list(np.bincount(s[e == ep], minlength=SPAN[ep]))
        expected += [e.size / len(LIVE) / SPAN[ep]] * int(SPAN[ep])
    assert len(observed) == 59
    report("a_joint", seed, gof(observed, expected))


def pair_table(x, y):
    idx = np.full(C.STAT_N_VALID, -1)
    idx[LIVE] = np.arange(len(LIVE))
    t = np.zeros((len(LIVE), len(LIVE)))
    np.add.at(t, (idx[x.ravel()], idx[y.ravel()]), 1)
    return t


@pytest.mark.parametrize("seed", C.STAT_SEEDS)
def test_b_episodes_of_consecutive_steps_are_independent(seed):
    e, _ = windows(seed)
    report("b_step_step+1", seed, independence(pair_table(e[:-1], e[1:])))


@pytest.mark.parametrize("seed", C.STAT_SEEDS)
def test_c_episodes_of_neighbouring_elements_are_independent(seed):
    e, _ = windows(seed)
    report("c_b_b+1", seed, independence(pair_table(e, np.roll(e, -1, axis=1))))


@pytest.mark.parametrize("seed", C.STAT_SEEDS)
def test_d_start_quarter_against_episode(seed):
    """ONE table for all episodes with span >= 2: rows the episode, columns floor(start * 4 / span), against the exact pmf (episode
    uniform, a quarter's share the number of starts that fall into it; cells no start falls into are no cells)."""
    e, s = windows(seed)
    eps = [ep for ep in LIVE if SPAN[ep] >= 2]
    keep = np.isin(e, eps)
    observed, expected = [], []
    for ep in eps:
        share = np.bincount(np.arange(SPAN[ep]) * 4 // SPAN[ep], minlength=4)
        got = np.bincount(s[e == ep] * 4 // SPAN[ep], minlength=4)
        assert (got[share == 0] == 0).all()
        observed += list(got[share > 0])
        expected += list(keep.sum() / len(eps) * share[share > 0] / SPAN[ep])
    # the number of draws that fall on these episodes is itself random: conditioning on it keeps the statistic chi-square, cells - 1
    report("d_quarter", seed, gof(observed, expected))


@pytest.mark.parametrize("seed", C.STAT_SEEDS)
def test_e_small_bags_are_uniform_subsets(seed):
    start, bag = C.STAT_BAGS["e"]
    rows = bags(seed, "e")
    srt = np.sort(rows, axis=1)
    assert (srt[:, 1:] > srt[:, :-1]).all() and srt.min() >= 0 and srt.max() < start
    subsets = {c: i for i, c in enumerate(itertools.combinations(range(start), bag))}
    assert len(subsets) == 35
    counts = np.bincount([subsets[tuple(r)] for r in srt], minlength=35)
    report("e_subsets", seed, gof(counts, np.full(35, len(rows) / 35)))
    report("e_rows", seed, bonferroni(np.bincount(rows.ravel(), minlength=start), len(rows), bag / start))
    # the order of the picks is Floyd's, not uniform: only the subset is compared with the reference


@pytest.mark.parametrize("seed", C.STAT_SEEDS)
def test_f_large_bags_include_rows_and_pairs_evenly(seed):
    start, bag = C.STAT_BAGS["f"]
    rows = bags(seed, "f")
    srt = np.sort(rows, axis=1)
    assert (srt[:, 1:] > srt[:, :-1]).all() and srt.min() >= 0 and srt.max() < start
    member = np.zeros((len(rows), start))
    member[np.arange(len(rows))[:, None], rows] = 1
    report("f_rows", seed, bonferroni(member.sum(0), len(rows), bag / start))
    pairs = (member.T @ member)[np.triu_indices(start, 1)]
    assert pairs.size == 780
    report("f_pairs", seed, bonferroni(pairs, len(rows), bag * (bag - 1) / (start * (start - 1))))


# ---- edge keys ---------------------------------------------------------------------------------------------------------------------------
SCAN = np.arange(1 << 16)


def first_step(hit):
    assert hit.any(), "no key in 65536 steps"
    return int(np.argmax(hit))


def edge_scan():
    """The edge keys of sampler_cases.py, found again: the smallest step at which element EDGE_B of seed EDGE_SEED meets each condition."""
    raw = lambda exclude: S.window_draw(C.EP_LEN, C.N_VALID, exclude, C.L, C.EDGE_SEED, SCAN, C.EDGE_B)
    span = np.maximum(np.asarray(C.EP_LEN) - C.L, 0) + 1
    window = {}
    for name, (exclude, _, _) in C.EDGE_WINDOW.items():
        e, s = raw(exclude)
        hit = {"first_choice": e == 0,
               "last_choice_exclude_outside": e == C.N_VALID - 1,
               "last_choice_exclude_inside": e == C.N_VALID - 1,
               "start_zero_of_33": (span[e] == 33) & (s == 0),
               "start_last_of_33": (span[e] == 33) & (s == 32)}[name]
        k = first_step(hit)
        window[name] = (exclude, k, (int(e[k]), int(s[k])))
    floyd = {}
    for name, (start, bag, j, _) in C.EDGE_FLOYD.items():
        floyd[name] = (start, bag, j, first_step(S.floyd_collisions(C.EDGE_SEED, SCAN, C.EDGE_B, start, bag)[:, j]))
    return window, floyd


def test_the_recorded_edge_keys_are_what_the_scan_finds():
    window, floyd = edge_scan()
    print("sampler-edge windows", window)
    print("sampler-edge floyd", floyd)
    assert window == C.EDGE_WINDOW and floyd == C.EDGE_FLOYD
    assert 33 in (np.maximum(np.asarray(C.EP_LEN) - C.L, 0) + 1) and 0 < C.MID < C.N_VALID - 1
    for start, bag, j, step in floyd.values():       # at a collision the pick IS the bound
        assert S.bag_rows(C.EDGE_SEED, step, C.EDGE_B, start, bag)[j] == start - bag + j


# ---- the oracle's own contract -----------------------------------------------------------------------------------------------------------
def test_oracle_shapes_and_refusals():
    h = S.hash_u32(0xFFFFFFFF, 2 ** 31 - 1, 599, 257)
    assert h.dtype == np.uint64 and int(h) < 2 ** 32
    e, s = S.window_draw([0, 5], 2, 0, 8, 1, 0, np.arange(7))            # one choice left; an empty span
    assert (e == 1).all() and (s == 0).all()
    e, s = S.window_draw([0], 1, 4, 8, 1, 0, np.arange(7))               # exclude outside: the only slot
    assert (e == 0).all() and (s == 0).all()
    with pytest.raises(ValueError):
        S.window_draw([3], 1, 0, 8, 1, 0, 0)
    assert S.bag_rows(1, 2, 3, 2, 4).tolist() == [0, 1, -1, -1] and S.bag_rows(1, 2, 3, 0, 2).tolist() == [-1, -1]
    assert sorted(S.bag_rows(1, 2, 3, 4, 4).tolist()) == [0, 1, 2, 3]    # start == bag_size: Floyd can only return every row
    arrays = C.replay_arrays("float")
    bo, ba = S.gather_bag(arrays, [2, 5], [[3, 0, -1], [-1, 40, 7]], -5.0)
    assert bo.dtype == np.float32 and ba.dtype == np.uint8 and bo.shape == (2, 3, C.O)
    assert (bo[0, 2] == -5).all() and (bo[1, 0] == -5).all() and ba[0, 2] == 0 == ba[1, 0]
    assert (bo[1, 1] == arrays["obss"][5, 40]).all() and ba[1, 1] == arrays["actions"][5, 40] and ba[0, 0] == arrays["actions"][2, 3]


# ---- census of the mixer's input words ---------------------------------------------------------------------------------------------------
CENSUS = dict(seed=12345, steps=1 << 16, elems=64, draws=34)


def census_equal_words(seed, steps, elems, draws, chunk=1 << 12):
    """Number of equal words among all (step < steps, elem < elems, draw < draws) of one seed, counted by sorting.  The low part of a
    word, elem << 20 ^ draw, is below 2^26, so two words can only be equal where the upper 38 bits of step * G agree: the words are
    sorted within each group of steps that share those bits, after the groups themselves were found by sorting -- exact, and 65 536
    values to sort instead of 1.4e8.  (A group of one step holds elems * draws distinct words: its low parts are distinct.)"""
    low = (S.word(0, 0, np.arange(elems)[:, None], np.arange(draws)[None, :])).ravel()
    assert int(low.max()) < 1 << 26 and np.unique(low).size == low.size
    hi = S.word(seed, np.arange(steps), 0, 0) >> np.uint64(26)
    order = np.argsort(hi, kind="stable")
    srt = hi[order]
    same = np.flatnonzero(srt[1:] == srt[:-1])
    equal = 0
    for v in np.unique(srt[same]):                           # groups of more than one step: sort their words outright
        group = order[srt == v]
        w = np.sort(S.word(seed, group[:, None, None], np.arange(elems)[None, :, None], np.arange(draws)[None, None, :]).ravel())
        equal += int((w[1:] == w[:-1]).sum())
    return equal, int(same.size)


def test_census_of_the_key_words():
    """No two keys of a run's first 65 536 updates (64 elements, draws 0 .. 33) enter the mixer as the same word; checked outright, by
    sorting every word, on the first 2 048 steps, where that is 4.5e6 words."""
    s = CENSUS["seed"]
    w = np.sort(S.word(s, np.arange(2048)[:, None, None], np.arange(64)[None, :, None], np.arange(34)[None, None, :]).ravel())
    assert w.size == 2048 * 64 * 34 and int((w[1:] == w[:-1]).sum()) == 0
    equal, shared = census_equal_words(**CENSUS)
    print(f"sampler-census words={CENSUS['steps'] * CENSUS['elems'] * CENSUS['draws']} equal={equal} steps_sharing_upper_bits={shared}")
    assert equal == 0
    # the counter finds what is there: a draw index of 2^20 is element 1, and a group of steps given twice is counted in full
    assert int(S.word(1, 5, 1, 0)) == int(S.word(1, 5, 0, 1 << 20))
    w = np.sort(S.word(s, np.array([3, 3])[:, None, None], np.arange(64)[None, :, None], np.arange(34)[None, None, :]).ravel())
    assert int((w[1:] == w[:-1]).sum()) == 64 * 34
