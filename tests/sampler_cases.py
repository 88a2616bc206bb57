"""Inputs of the device-sampler tests, fixed before anything ran: the statistics of tests/test_sampler_reference.py (the oracle alone)
and the kernel cases that test_emu_sampler.py / test_gpu_sampler.py replay through sampler_helpers.py.  docs/sampler_tests.md."""
import numpy as np

# ---- statistics on oracle/sampler_oracle.py (test_sampler_reference.py) ------------------------------------------------------------------
STAT_SEEDS = (0, 5, 12345, 0xFFFFFFFF)
STAT_N_VALID, STAT_EXCLUDE, STAT_L = 11, 3, 8
STAT_EP_LEN = (1, 7, 8, 9, 12, 20, 8, 30, 16, 9, 10)
STAT_BATCH, STAT_STEPS = 32, 4000              # 128 000 window draws per seed; the rarest cell (episode 7, 23 starts) expects 556
STAT_BAG_STEPS = 1000                          # 32 000 bags per seed
STAT_BAGS = {"e": (7, 3), "f": (40, 8)}        # (start, bag_size)
P_MIN = 1e-4

# ---- the replay of the kernel cases -------------------------------------------------------------------------------------------------------
E, T, L, O = 12, 40, 8, 3
EP_LEN = (0, 1, L - 1, L, L + 1, T, 20, 13, L, 33, 12, T)
N_VALID, MID = 12, 5
EXCLUDES = (-1, 0, MID, N_VALID - 1, N_VALID, N_VALID + 5)
BATCHES = (1, 255, 256, 257, 600)              # DTQN_THREADS = 256: 257 and 600 cross a block
STEPS = (0, 1, 2 ** 31 - 1)
SEEDS = (0, 0xFFFFFFFF)
SENTINEL = -77
MAX_BAG = 256                                  # DTQN_MAX_BAG
BAGS = (1, 3, 8)
BIG = dict(E=2, T=300, O=1, ep_len=(300, 297))  # the replay of the bag_size = MAX_BAG case


def bag_starts(bag, t=T):
    """Window starts of the bag cases: the prefix branch, its edge, Floyd at its tightest bound and beyond, the last window of an episode.
    (At bag_size 256 on 300 rows 2 * bag is no row of the replay: the starts above the rows are left out there.)"""
    return sorted({s for s in (0, 1, bag - 1, bag, bag + 1, 2 * bag, t - L) if 0 <= s <= t - L})


# ---- edge keys: the smallest step >= 0 at which element 0 of seed 0 meets the condition, found by test_sampler_reference.edge_scan on the
# oracle (that test repeats the scan and compares).  Windows: the replay above, N_VALID slots.  Bags: (start, bag_size) as named.
EDGE_SEED, EDGE_B = 0, 0
EDGE_WINDOW = {
    # name: (exclude, step, (episode, start) the oracle draws there)
    "first_choice": (-1, 2, (0, 0)),
    "last_choice_exclude_outside": (-1, 3, (11, 14)),
    "last_choice_exclude_inside": (MID, 3, (11, 14)),
    "start_zero_of_33": (-1, 9, (11, 0)),
    "start_last_of_33": (-1, 427, (11, 32)),
}
EDGE_FLOYD = {
    # name: (start, bag_size, j, step)
    "bag3_j1": (7, 3, 1, 4),
    "bag3_last": (7, 3, 2, 3),
    "bag8_j1": (16, 8, 1, 4),
    "bag8_last": (16, 8, 7, 2),
    "bag8_tight_last": (8, 8, 7, 0),
}


def replay_arrays(kind, e=E, t=T, o=O, ep_len=EP_LEN, seed=3):
    """ReplayBuffer.export_arrays()-shaped content: every row distinct, rows behind an episode's end included (the draw never reads them;
    a gather that did would show).  kind "float": observations in (-1, 1); "discrete": integer tokens 0 .. 8 as floats."""
    rng = np.random.default_rng(seed)
    obss = (rng.integers(0, 9, (e, t + 1, o)).astype(np.float32) if kind == "discrete"
            else rng.uniform(-1, 1, (e, t + 1, o)).astype(np.float32))
    return dict(obss=obss, actions=rng.integers(1, 250, (e, t + 1)).astype(np.uint8), rewards=np.zeros((e, t), np.float32),
                dones=np.zeros((e, t), np.uint8), eplens=np.asarray(ep_len, dtype=np.int64))
