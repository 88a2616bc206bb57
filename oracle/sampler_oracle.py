"""CPU oracle for the device sampler.  TEST INFRASTRUCTURE ONLY (see oracle/dtqn_oracle.py header).

Plain-numpy restatement of what `--sampler device` draws: which (episode, start) window every batch element of an update trains on,
and which rows below that window make up its bag.  Every function is a pure function of its arguments, in integer arithmetic, so the
kernels are held to it by exact equality (tests/sampler_helpers.py), and its distribution is tested once, on this file alone
(tests/test_sampler_reference.py).

What restates what:

  hash_u32      dtqn_amd/csrc/dtqn_device.hpp, hash_u32: the 64-bit word  seed << 32 ^ step * G ^ elem << 20 ^ draw  (G the 64-bit golden
                ratio, the product taken modulo 2^64) goes through one splitmix64 step -- add G, two xor-shift-multiply rounds, a last
                xor-shift -- and the upper 32 bits of the result are the draw.
  window_draw   dtqn_amd/csrc/dtqn_device.hpp, replay_draw -- called by dtqn_replay_sample_kernel (dtqn_replay.hip) and by the two
                in-forward draw sites of dtqn_forward_body.hpp.  Draw 0 picks the episode among the finished slots [0, n_valid) minus
                `exclude` (a multiply-shift onto the number of choices, then a shift past the excluded slot); draw 1 picks the start on
                {0 .. max(0, len - L)}.  The target is ReplayBuffer.sample of the reference (random.choice over the valid slots, then
                random.randint(0, max(0, len - L))).
  bag_rows      dtqn_amd/csrc/dtqn_replay.hip, dtqn_replay_bag_kernel with rows == NULL: a window with fewer than bag_size rows below
                it takes all of them in order and pads with -1; otherwise Floyd's sampling of bag_size distinct rows of [0, start),
                pick j from draw 2 + j.  The target is the uniform bag_size-subset of ReplayBuffer.sample_with_bag of the reference.
  gather_bag    the copy loop of the same kernel: observation row r and the replay's action row r of the episode, obs_mask and action 0
                in the padding.

`word` is the 64-bit input of the mixer on its own, for the collision census of the key space; `floyd_collisions` says at which picks
bag_rows took the bound because the row was taken, for the search of keys that reach that branch.
"""
from __future__ import annotations

import numpy as np

G = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)


def _u64(x):
    return np.asarray(x).astype(np.uint64)


def word(seed, step, elem, draw):
    """The 64-bit word a key is folded into before it is mixed (arrays broadcast)."""
    with np.errstate(over="ignore"):
        return (_u64(seed) << np.uint64(32)) ^ (_u64(step) * G) ^ (_u64(elem) << np.uint64(20)) ^ _u64(draw)


def hash_u32(seed, step, elem, draw):
    """32 random bits per (seed, step, elem, draw), each a 32-bit unsigned value; arrays broadcast.  Returned as uint64 < 2^32."""
    with np.errstate(over="ignore"):
        z = word(seed, step, elem, draw) + G
        z = (z ^ (z >> np.uint64(30))) * M1
        z = (z ^ (z >> np.uint64(27))) * M2
        z = z ^ (z >> np.uint64(31))
    return z >> np.uint64(32)


def _scale(h, n):
    """Multiply-shift of 32 random bits onto [0, n): floor(h * n / 2^32) (h < 2^32 and n < 2^32, so the product fits 64 bits)."""
    return ((h * _u64(n)) >> np.uint64(32)).astype(np.int64)


def window_draw(ep_len, n_valid, exclude, ctx_len, seed, step, b):
    """(episode, start) of batch element(s) b of update `step`; step and b broadcast against each other."""
    ep_len = np.asarray(ep_len, dtype=np.int64)
    skip = 0 <= exclude < n_valid
    choices = n_valid - (1 if skip else 0)
    if choices < 1:
        raise ValueError("no episode to choose from")
    e = _scale(hash_u32(seed, step, b, 0), choices)
    if skip:
        e = e + (e >= exclude)
    span = np.maximum(ep_len[e] - ctx_len, 0) + 1
    s = _scale(hash_u32(seed, step, b, 1), span)
    return e, s


def bag_rows(seed, step, b, start, bag_size):
    """Rows of the bags of windows that begin at row `start` (one value): int64 [..., bag_size] over the broadcast shape of step and
    b ([bag_size] for scalars), -1 for padding."""
    start, bag_size = int(start), int(bag_size)
    step, b = np.broadcast_arrays(np.asarray(step), np.asarray(b))
    rows = np.full(step.shape + (bag_size,), -1, dtype=np.int64)
    if start < bag_size:
        rows[..., :start] = np.arange(start)
        return rows
    for j in range(bag_size):
        hi = start - bag_size + j                    # Floyd: pick j is uniform on [0, hi], or hi itself where that row is taken
        r = _scale(hash_u32(seed, step, b, 2 + j), hi + 1)
        taken = (rows[..., :j] == r[..., None]).any(axis=-1)
        rows[..., j] = np.where(taken, hi, r)
    return rows


def floyd_collisions(seed, step, b, start, bag_size):
    """bool [..., bag_size]: pick j of bag_rows fell on a row taken before and became the bound (all False in the prefix branch)."""
    start, bag_size = int(start), int(bag_size)
    rows = bag_rows(seed, step, b, start, bag_size)
    hit = np.zeros(rows.shape, dtype=bool)
    if start >= bag_size:
        for j in range(1, bag_size):
            r = _scale(hash_u32(seed, step, b, 2 + j), start - bag_size + j + 1)
            hit[..., j] = (rows[..., :j] == np.asarray(r)[..., None]).any(axis=-1)
    return hit


def gather_bag(arrays, episode, rows, obs_mask):
    """(bag_obs [B][bag][O] float32, bag_actions [B][bag] uint8) of windows in `episode` [B] with bag rows `rows` [B][bag], out of
    ReplayBuffer.export_arrays()-shaped arrays (obss [E][T+1][O], actions [E][T+1])."""
    obss, actions = np.asarray(arrays["obss"]), np.asarray(arrays["actions"])
    episode, rows = np.asarray(episode, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    e = episode[:, None]
    live = rows >= 0
    r = np.where(live, rows, 0)
    bag_obs = np.where(live[:, :, None], obss[e, r], np.float32(obs_mask)).astype(np.float32)
    bag_actions = np.where(live, actions[e, r], 0).astype(np.uint8)
    return bag_obs, bag_actions
