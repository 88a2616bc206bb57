"""The dropout keep masks seen from outside: tests/test_dropout_mask_keys.py asks the oracle's mask functions (rows_keep, attn_keep,
bag_keep) for booleans and never builds an element index or evaluates the hash itself -- a restatement would test itself.

An element of one update is (site, layer, pass, sequence, a, b, c): (row, column, -) at the embedding and FFN sites, (head, query row,
key row) at the attention site, (head, query row, bag entry) at the bag site.  `label` packs that tuple into an int64 of this module's
own making (it only names elements, so that a grid evaluated twice is counted once and a collision can be printed)."""
import itertools

import numpy as np

from oracle import dtqn_oracle as O

K = 64                                  # (seed, step) pairs per signature: two different keys agree on all of them with probability 2^-64
MAX_LAYERS = 8                          # DTQN_MAX_LAYERS (include/dtqn_hip.h; test_surface.py holds the two together)
PASSES = (0, 1)                         # the train-mode passes of a TD update: policy(o), policy(o')
HEADS = (0, 1, 2, 63)                   # d_model 256 at head width 4: 64 heads
WIDTH = 256                             # the widest d_model
SITE_NAMES = {O.DROP_EMB: "emb", O.DROP_ATTN: "attn", O.DROP_FFN: "ffn", O.DROP_BAG: "bag"}


def pairs(k=K):
    """k different (seed, step) pairs: a few seeds, small and large steps."""
    rng = np.random.default_rng(20240)
    out = [(0, 0), (0, 1), (1, 0), (4242, 2), (0xFFFFFFFF, 0xFFFFFFFF), (99, 1000), (99, 1001), (12345, 2 ** 31)]
    while len(out) < k:
        pr = (int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 20)))
        if pr not in out:
            out.append(pr)
    return out[:k]


def edges(L):
    """Rows worth a look at a context of L rows: both ends, and both sides of 256."""
    return sorted({r for r in (0, 1, 2, 3, 127, 128, 254, 255, 256, 257, 258, 319, 320, 383, 384, 510, 511, L - 2, L - 1) if 0 <= r < L})


def label(site, layer, which, b, a, bb, c):
    """int64 name of an element; arrays a, bb, c broadcast."""
    a, bb, c = np.broadcast_arrays(np.asarray(a, dtype=np.int64), np.asarray(bb, dtype=np.int64), np.asarray(c, dtype=np.int64))
    assert 0 <= site < 4 and 0 <= layer < 8 and 0 <= which < 4 and 0 <= b < 2 ** 21
    assert a.min() >= 0 and a.max() < 1024 and bb.min() >= 0 and bb.max() < 1024 and c.min() >= 0 and c.max() < 1024
    head = ((site * 8 + layer) * 4 + which) * 2 ** 21 + b
    return ((head * 1024 + a) * 1024 + bb) * 1024 + c


def unlabel(x):
    x = int(x)
    c, x = x % 1024, x // 1024
    bb, x = x % 1024, x // 1024
    a, x = x % 1024, x // 1024
    b, x = x % 2 ** 21, x // 2 ** 21
    which, x = x % 4, x // 4
    layer, site = x % 8, x // 8
    return {"site": SITE_NAMES[site], "layer": layer, "pass": which, "sequence": b, "element": (a, bb, c)}


class Grid:
    """A block of elements of one (site, layer, pass, sequence): keep(spec) -> flat booleans, labels -> flat int64, in one order."""

    def __init__(self, site, layer, which, b, ax0, ax1, ax2=None, causal=False):
        self.site, self.layer, self.which, self.b = site, layer, which, b
        self.ax = [np.asarray(ax0), np.asarray(ax1)] + ([np.asarray(ax2)] if ax2 is not None else [])
        self.sel = None
        if causal:                      # the live elements of a causal layer: key <= query row
            self.sel = np.broadcast_to(self.ax[2][None, None, :] <= self.ax[1][None, :, None], tuple(len(a) for a in self.ax)).reshape(-1)
        if site in (O.DROP_EMB, O.DROP_FFN):
            lab = label(site, layer, which, b, self.ax[0][:, None], self.ax[1][None, :], 0)
        else:
            lab = label(site, layer, which, b, self.ax[0][:, None, None], self.ax[1][None, :, None], self.ax[2][None, None, :])
        self.labels = lab.reshape(-1) if self.sel is None else lab.reshape(-1)[self.sel]

    def keep(self, p, seed, step):
        spec = O.DropSpec(p, seed, step, self.which)
        if self.site in (O.DROP_EMB, O.DROP_FFN):
            m = O.rows_keep(spec, self.b, self.site, self.layer, self.ax[0], self.ax[1], WIDTH)
        elif self.site == O.DROP_ATTN:
            m = O.attn_keep(spec, self.b, self.layer, *self.ax)
        else:
            m = O.bag_keep(spec, self.b, *self.ax)
        m = np.asarray(m).reshape(-1)
        return m if self.sel is None else m[self.sel]


def update_grids(L, max_batch):
    """The element set of one update at a context of L rows, cut to what a few seconds hold: whole tensors at (layer 0, pass 0,
    sequence 0) -- the causal triangle of HEADS, the bag weights of heads 0 and 1 with a bag as large as the context, embedding and FFN
    output at the widest d_model -- and, for every combination of the extreme layers, both passes and sequences 0, 1 and the largest,
    the sub-grids of edge rows (edges(L)) x edge rows / edge columns at every site."""
    rows, cols = np.arange(L), np.arange(WIDTH)
    g = [Grid(O.DROP_ATTN, 0, 0, 0, HEADS, rows, rows, causal=True),
         Grid(O.DROP_BAG, 0, 0, 0, HEADS[:2], rows, rows),
         Grid(O.DROP_EMB, 0, 0, 0, rows, cols),
         Grid(O.DROP_FFN, 0, 0, 0, rows, cols),
         Grid(O.DROP_FFN, MAX_LAYERS - 1, 0, 0, rows, cols)]
    e = edges(L)
    ec = sorted({0, 1, 2, 3, 63, 64, 127, 128, 254, 255})
    for layer, which, b in itertools.product((0, 1, MAX_LAYERS - 1), PASSES, (0, 1, max_batch - 1)):
        g.append(Grid(O.DROP_ATTN, layer, which, b, HEADS, e, e, causal=True))
        g.append(Grid(O.DROP_FFN, layer, which, b, e, ec))
        if layer == 0:                  # one embedding and one bag branch per network
            g.append(Grid(O.DROP_EMB, 0, which, b, e, ec))
            g.append(Grid(O.DROP_BAG, 0, which, b, HEADS, e, e))
    return g


def signatures(grids, p=0.5, prs=None):
    """-> (labels, signatures): every element of the grids once, with its keep decisions under the K (seed, step) pairs packed into a
    uint64."""
    prs = pairs() if prs is None else prs
    assert len(prs) <= 64
    labels = np.concatenate([g.labels for g in grids])
    sig = np.zeros(labels.size, dtype=np.uint64)
    for k, (seed, step) in enumerate(prs):
        sig |= np.concatenate([g.keep(p, seed, step) for g in grids]).astype(np.uint64) << np.uint64(k)
    labels, first = np.unique(labels, return_index=True)
    return labels, sig[first]


def collisions(labels, sig):
    """-> (number of distinct signatures, a few (element, element) pairs that share one)."""
    order = np.argsort(sig, kind="stable")
    s = sig[order]
    same = np.flatnonzero(s[1:] == s[:-1])
    distinct = s.size - same.size
    shown = [(unlabel(labels[order[i]]), unlabel(labels[order[i + 1]])) for i in same[:4]]
    return distinct, shown


def four_sigma(rate, n):
    return 4.0 * np.sqrt(rate * (1.0 - rate) / n)
