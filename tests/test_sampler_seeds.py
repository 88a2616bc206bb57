"""The seeds a run derives from --seed and the rank (run.py) are pairwise distinct.  The window draw keys hash_u32(seed, step, element, k)
and the device rollout keys hash_u32(seed, vstep, env, k) share one function and overlapping draw indices k: with equal seeds an
environment's exploration bits WOULD BE a batch element's episode bits (oracle/sampler_oracle.py restates the function)."""
import itertools

import pytest

import run as runpy
from dtqn_amd.agents.dtqn import dropout_seed_of


@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 31 - 1])
def test_the_seeds_of_a_run_are_pairwise_distinct(seed):
    named = {}
    for rank in range(8):
        named[("sampler", rank)] = runpy.sampler_seed(seed, rank)
        named[("dropout", rank)] = dropout_seed_of(runpy.sampler_seed(seed, rank))
        named[("rollout", rank)] = runpy.rollout_seed(seed, rank)
        for d in range(2):
            named[("evaluator", rank, d)] = runpy.evaluator_seed(seed, rank, d)
    assert len(named) == 8 * 5
    as_u32 = {k: v & 0xFFFFFFFF for k, v in named.items()}            # what the kernels see
    for (ka, a), (kb, b) in itertools.combinations(as_u32.items(), 2):
        assert a != b, (ka, kb, a)
