"""The dropout keep masks as a black box (oracle only, no device, no emulation): every element of one update has a key of its own, and
the masks are Bernoulli(1 - p) and pairwise independent across everything a key is made of.

The parity tests compare kernels and oracle under ONE mask, so a key that two elements share on both sides passes them all.  Here the
masks are seen only through the oracle's rows_keep / attn_keep / bag_keep (dropout_mask_helpers.py); the element index and the hash are
not restated.  docs/dropout_mask_tests.md has the collision counts these tests found and the mutations they reject."""
import numpy as np
import pytest

from oracle import dtqn_oracle as O

from dropout_mask_helpers import HEADS, MAX_LAYERS, WIDTH, Grid, collisions, four_sigma, pairs, signatures, update_grids

CONTEXTS = (256, 257, 320, 512)
PS = (0.1, 0.3, 0.5)
DRAWS = pairs(8)                        # (seed, step) pairs of the distribution tests


@pytest.mark.parametrize("L", CONTEXTS)
def test_every_element_of_an_update_has_its_own_key(L):
    """Signatures of 64 keep decisions at p = 0.5 ((seed, step) pairs of dropout_mask_helpers.pairs): two elements with different keys
    agree on all 64 with probability 2^-64, so over M <= 1e7 elements any equality (chance below M^2 / 2 * 2^-64 < 3e-6) is a shared
    key.  The element set: dropout_mask_helpers.update_grids."""
    labels, sig = signatures(update_grids(L, O.DROP_MAX_BATCH))
    assert 100_000 < labels.size <= 10_000_000
    distinct, shown = collisions(labels, sig)
    print(f"context {L}: {labels.size} elements, {distinct} distinct signatures")
    assert distinct == labels.size, (L, labels.size, distinct, shown)


def test_the_signature_test_sees_a_shared_key():
    """The check itself: one element evaluated under two names is reported, with both names."""
    g = [Grid(O.DROP_ATTN, 0, 0, 0, (0,), (300,), np.arange(301)), Grid(O.DROP_ATTN, 0, 0, 0, (0,), (300,), np.arange(301))]
    g[1].labels = g[1].labels.copy()
    g[1].labels[7] += 1 << 50            # a name no element has: the same key under another name
    labels, sig = signatures(g)
    distinct, shown = collisions(labels, sig)
    assert labels.size == 302 and distinct == 301 and shown[0][0]["element"] == (0, 300, 7)


def _site_grids(L):
    """Whole tensors of the four sites at (layer 1, pass 0, sequence 1)."""
    rows, cols = np.arange(L), np.arange(WIDTH)
    return {"emb": Grid(O.DROP_EMB, 0, 0, 1, rows, cols), "attn": Grid(O.DROP_ATTN, 1, 0, 1, HEADS, rows, rows, causal=True),
            "ffn": Grid(O.DROP_FFN, 1, 0, 1, rows, cols), "bag": Grid(O.DROP_BAG, 0, 0, 1, HEADS[:2], rows, rows)}


def _keep(grid, p, draws=DRAWS):
    return np.concatenate([grid.keep(p, seed, step) for seed, step in draws])


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("L", CONTEXTS)
def test_keep_rate_of_every_site(L, p):
    for name, g in _site_grids(L).items():
        m = _keep(g, p, DRAWS[:2])
        assert abs(m.mean() - (1 - p)) < four_sigma(1 - p, m.size), (name, L, p, m.mean(), m.size)


def _agreement(a, b, p, what):
    """Two masks with different keys agree with probability p^2 + (1 - p)^2, within four binomial sigma at the sample size."""
    assert a.shape == b.shape and a.size > 0
    rate = p * p + (1 - p) * (1 - p)
    got = float((a == b).mean())
    assert abs(got - rate) < four_sigma(rate, a.size), (what, p, got, rate, a.size)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("L", CONTEXTS)
def test_masks_are_independent_across_the_fields_of_a_key(L, p):
    rows, cols = np.arange(L), np.arange(WIDTH)
    sites = _site_grids(L)
    steps = [(seed, step + 1) for seed, step in DRAWS]
    for name, g in sites.items():
        _agreement(_keep(g, p), _keep(g, p, steps), p, (name, L, "consecutive optimizer steps"))
        other = Grid(g.site, g.layer, 1, g.b, *g.ax, causal=g.sel is not None)
        _agreement(_keep(g, p), _keep(other, p), p, (name, L, "the two train-mode passes"))
        other = Grid(g.site, g.layer, g.which, g.b + 1, *g.ax, causal=g.sel is not None)
        _agreement(_keep(g, p), _keep(other, p), p, (name, L, "neighbouring sequences"))
    for site, ax in ((O.DROP_ATTN, (HEADS, rows, rows)), (O.DROP_FFN, (rows, cols))):
        for layer in (0, MAX_LAYERS - 2):
            a, b = Grid(site, layer, 0, 0, *ax), Grid(site, layer + 1, 0, 0, *ax)
            _agreement(_keep(a, p, DRAWS[:2]), _keep(b, p, DRAWS[:2]), p, (site, L, "neighbouring layers", layer))
    a, b = Grid(O.DROP_ATTN, 0, 0, 0, HEADS, rows, rows), Grid(O.DROP_BAG, 0, 0, 0, HEADS, rows, rows)
    _agreement(_keep(a, p, DRAWS[:2]), _keep(b, p, DRAWS[:2]), p, (L, "attention and bag site"))
    _agreement(_keep(sites["emb"], p), _keep(Grid(O.DROP_FFN, 0, 0, 1, rows, cols), p), p, (L, "embedding and FFN site"))


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("L", CONTEXTS[1:])
def test_rows_256_apart_do_not_repeat_each_other(L, p):
    """The two pairs an eight-bit row field would alias: query rows t and t - 256 of neighbouring heads, keys s and s - 256 of
    neighbouring rows.  Every head of the widest network, every row and key from 256 up, both sites."""
    even, hi, full = np.arange(0, 64, 2), np.arange(256, L), np.arange(L)
    hi_even = hi[hi % 2 == 0]
    draws = pairs(64) if L == 257 else DRAWS[:2]        # one row beyond 256: more draws for the sample
    for site in (O.DROP_ATTN, O.DROP_BAG):
        a, b = Grid(site, 0, 0, 0, even, hi, full), Grid(site, 0, 0, 0, even + 1, hi - 256, full)
        _agreement(_keep(a, p, draws), _keep(b, p, draws), p, (site, L, "query rows t and t - 256 of neighbouring heads"))
        a, b = Grid(site, 0, 0, 0, HEADS, hi_even, hi), Grid(site, 0, 0, 0, HEADS, hi_even + 1, hi - 256)
        _agreement(_keep(a, p, draws), _keep(b, p, draws), p, (site, L, "keys s and s - 256 of neighbouring rows"))
