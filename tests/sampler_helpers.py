"""The device sampler against oracle/sampler_oracle.py by exact integer equality: the draw kernels through the C ABI on a DeviceReplay
(no network), and the draw inside the update.  One set of functions taking (lib, device), run on the CPU emulation by
test_emu_sampler.py and on the device by test_gpu_sampler.py.  Inputs: sampler_cases.py.  docs/sampler_tests.md."""
import ctypes

import numpy as np
import torch

from oracle import sampler_oracle as S

import sampler_cases as C

DTQN_OK, DTQN_ERR_ARG = 0, 2
PAD = 8                       # entries behind `batch` in every output array: they keep the sentinel


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream) if torch.device(device).type == "cuda" else None


def make_replay(device, arrays, mask=-5.0):
    from dtqn_amd.learner import DeviceReplay
    e, t1, o = arrays["obss"].shape
    rep = DeviceReplay(e, t1 - 1, o, mask, torch.device(device))
    rep.obs.copy_(torch.from_numpy(arrays["obss"]))
    rep.actions.copy_(torch.from_numpy(arrays["actions"]))
    rep.ep_len.copy_(torch.from_numpy(arrays["eplens"].astype(np.int32)))
    return rep


def counter_of(device, step):
    """A TdEngine-shaped step counter: the optimizer step the draws are keyed by is entry 1; the other entries hold what must not be read."""
    return torch.tensor([77, step, 99, 55], dtype=torch.int32, device=device)


def draw_windows(lib, device, rep, n_valid, exclude, batch, seed, step, counter=None, at=True, ctx_len=C.L):
    """(rc, episode, start) of one launch; the arrays are PAD entries longer than `batch` and start as the sentinel."""
    n = max(batch, 0) + PAD
    e = torch.full((n,), C.SENTINEL, dtype=torch.int32, device=device)
    s = torch.full((n,), C.SENTINEL, dtype=torch.int32, device=device)
    if at:
        rc = lib.dtqn_replay_sample_at(rep.view_ref, n_valid, exclude, ctx_len, batch, seed, step, _p(counter), _p(e), _p(s), _stream(device))
    else:
        rc = lib.dtqn_replay_sample(rep.view_ref, n_valid, exclude, ctx_len, batch, seed, _p(counter), _p(e), _p(s), _stream(device))
    return rc, e.cpu().numpy(), s.cpu().numpy()


def check_windows(lib, device, rep, ep_len, n_valid, exclude, batch, seed, step, *, counter=None, at=True, key_step=None):
    """One launch equals the oracle at every element, and nothing behind `batch` was written.  key_step: the step the draw is keyed by
    where `step` does not say it (step -1: the counter's, or 0 without one)."""
    rc, e, s = draw_windows(lib, device, rep, n_valid, exclude, batch, seed, step, counter, at)
    assert rc == DTQN_OK, (rc, n_valid, exclude, batch, seed, step)
    we, ws = S.window_draw(ep_len, n_valid, exclude, C.L, seed, step if key_step is None else key_step, np.arange(batch))
    where = (n_valid, exclude, batch, seed, step, key_step)
    assert np.array_equal(e[:batch], we), ("episode", where, np.flatnonzero(e[:batch] != we)[:8])
    assert np.array_equal(s[:batch], ws), ("start", where, np.flatnonzero(s[:batch] != ws)[:8])
    assert (e[batch:] == C.SENTINEL).all() and (s[batch:] == C.SENTINEL).all(), where
    return e[:batch], s[:batch]


def edge_steps():
    return sorted({k for _, k, _ in C.EDGE_WINDOW.values()})


def run_window_grid(lib, device, batch):
    """Every exclude x step x seed of sampler_cases.py at one batch, all slots finished; returns the number of launches."""
    rep = make_replay(device, C.replay_arrays("float"))
    n = 0
    for exclude in C.EXCLUDES:
        for step in list(C.STEPS) + edge_steps():
            for seed in C.SEEDS:
                e, _ = check_windows(lib, device, rep, C.EP_LEN, C.N_VALID, exclude, batch, seed, step)
                assert not (e == exclude).any()
                n += 1
    return n


def run_window_small_rings(lib, device):
    """One finished slot with the slot in progress outside it, and two with it inside: one choice in either case."""
    rep = make_replay(device, C.replay_arrays("float"))
    for n_valid, excludes, only in ((1, (-1, 1, 6), None), (2, (0, 1), True)):
        for exclude in excludes:
            for batch in (1, 257):
                for seed in C.SEEDS:
                    for step in C.STEPS:
                        e, _ = check_windows(lib, device, rep, C.EP_LEN, n_valid, exclude, batch, seed, step)
                        assert (e == (0 if only is None else 1 - exclude)).all()


def run_window_edge_keys(lib, device):
    """The recorded keys give the recorded extremes: first and last choice, start 0 and span - 1 of the longest span."""
    rep = make_replay(device, C.replay_arrays("float"))
    for name, (exclude, step, (we, ws)) in C.EDGE_WINDOW.items():
        e, s = check_windows(lib, device, rep, C.EP_LEN, C.N_VALID, exclude, C.EDGE_B + 1, C.EDGE_SEED, step)
        assert (int(e[C.EDGE_B]), int(s[C.EDGE_B])) == (we, ws), name


def run_window_step_counter(lib, device):
    """step -1 reads entry 1 of the counter (dtqn_replay_sample always does), and is step 0 without a counter; an explicit step wins."""
    rep = make_replay(device, C.replay_arrays("float"))
    for seed in C.SEEDS:
        for k in (0, 5, 2 ** 31 - 1):
            ctr = counter_of(device, k)
            check_windows(lib, device, rep, C.EP_LEN, C.N_VALID, C.MID, 257, seed, -1, counter=ctr, key_step=k)
            check_windows(lib, device, rep, C.EP_LEN, C.N_VALID, C.MID, 257, seed, -1, counter=ctr, at=False, key_step=k)
            check_windows(lib, device, rep, C.EP_LEN, C.N_VALID, C.MID, 257, seed, 3, counter=ctr)
            assert ctr.cpu().tolist() == [77, k, 99, 55]
        check_windows(lib, device, rep, C.EP_LEN, C.N_VALID, C.MID, 257, seed, -1, key_step=0)
        check_windows(lib, device, rep, C.EP_LEN, C.N_VALID, C.MID, 257, seed, -1, at=False, key_step=0)


def run_window_refusals(lib, device):
    rep = make_replay(device, C.replay_arrays("float"))
    for n_valid, exclude, batch in ((C.N_VALID, C.MID, 0), (C.N_VALID, C.MID, -3), (1, 0, 4), (0, -1, 4)):
        for at in (True, False):
            rc, e, s = draw_windows(lib, device, rep, n_valid, exclude, batch, 1, 0, at=at)
            assert rc == DTQN_ERR_ARG, (n_valid, exclude, batch, at, rc)
            assert (e == C.SENTINEL).all() and (s == C.SENTINEL).all()


# ---- bags ---------------------------------------------------------------------------------------------------------------------------------
def gather(lib, device, rep, episodes, starts, bag, seed, counter, rows=None):
    """(rc, bag_obs, bag_actions) of one dtqn_replay_gather_bag; the outputs hold PAD windows more than the batch, set to sentinels."""
    batch = len(episodes)
    e = torch.tensor(np.asarray(episodes), dtype=torch.int32, device=device)
    s = torch.tensor(np.asarray(starts), dtype=torch.int32, device=device)
    r = None if rows is None else torch.tensor(np.ascontiguousarray(rows), dtype=torch.int32, device=device)
    nb = max(bag, 1)
    bo = torch.full((batch + PAD, nb, rep.O), float(C.SENTINEL), dtype=torch.float32, device=device)
    ba = torch.full((batch + PAD, nb), 0xEE, dtype=torch.uint8, device=device)
    rc = lib.dtqn_replay_gather_bag(rep.view_ref, _p(e), _p(s), _p(r), batch, bag, seed, _p(counter), _p(bo), _p(ba), _stream(device))
    return rc, bo.cpu().numpy(), ba.cpu().numpy()


def check_bags(lib, device, rep, arrays, episodes, starts, bag, seed, step):
    """Device-drawn bags (rows == NULL) of the given windows equal the oracle's rows gathered by the oracle; step None: no counter."""
    batch = len(episodes)
    rc, bo, ba = gather(lib, device, rep, episodes, starts, bag, seed, None if step is None else counter_of(device, step))
    assert rc == DTQN_OK
    rows = np.stack([S.bag_rows(seed, 0 if step is None else step, b, starts[b], bag) for b in range(batch)])
    for b in range(batch):                  # the oracle's rows are a bag: distinct rows below the window, padding behind them
        live = rows[b][rows[b] >= 0]
        assert len(live) == min(bag, starts[b]) == len(set(live.tolist())) and (live < starts[b]).all()
    wo, wa = S.gather_bag(arrays, episodes, rows, rep.obs_mask)
    where = (bag, seed, step)
    assert np.array_equal(bo[:batch], wo), ("bag_obs", where, np.argwhere(bo[:batch] != wo)[:4])
    assert np.array_equal(ba[:batch], wa), ("bag_actions", where, np.argwhere(ba[:batch] != wa)[:4])
    pad = rows < 0
    assert (bo[:batch][pad] == np.float32(rep.obs_mask)).all() and (ba[:batch][pad] == 0).all()
    assert (bo[batch:] == C.SENTINEL).all() and (ba[batch:] == 0xEE).all(), where
    return rows


def run_bags(lib, device, kind, bag):
    """bag_size 1, 3 or 8 on the replay of the window cases: every start of bag_starts in three episodes, steps by counter and without."""
    arrays = C.replay_arrays(kind)
    rep = make_replay(device, arrays, mask=-5.0 if kind == "float" else 9.0)
    starts = [s for s in C.bag_starts(bag) for _ in range(3)]
    episodes = [(5, 9, 11)[i % 3] for i in range(len(starts))]
    for seed in C.SEEDS:
        for step in (None, 0, 1, 2 ** 31 - 1):
            check_bags(lib, device, rep, arrays, episodes, starts, bag, seed, step)


def run_bags_collision_keys(lib, device):
    """The recorded keys at which Floyd's pick falls on a row taken before: the entry is the bound, as in the oracle."""
    arrays = C.replay_arrays("float")
    rep = make_replay(device, arrays)
    for name, (start, bag, j, step) in C.EDGE_FLOYD.items():
        assert S.floyd_collisions(C.EDGE_SEED, step, C.EDGE_B, start, bag)[j], name
        rows = check_bags(lib, device, rep, arrays, [5, 5, 9, 11], [start] * 4, bag, C.EDGE_SEED, step)
        assert rows[C.EDGE_B][j] == start - bag + j, name


def run_bags_max(lib, device):
    """DTQN_MAX_BAG rows per bag, on a replay of 300-row episodes with one-column observations."""
    big = C.BIG
    arrays = C.replay_arrays("float", e=big["E"], t=big["T"], o=big["O"], ep_len=big["ep_len"], seed=4)
    rep = make_replay(device, arrays)
    starts = [s for s in C.bag_starts(C.MAX_BAG, big["T"]) for _ in range(2)]
    assert {0, 1, C.MAX_BAG - 1, C.MAX_BAG, C.MAX_BAG + 1, big["T"] - C.L} == set(starts)
    episodes = [i % 2 for i in range(len(starts))]
    for seed in C.SEEDS:
        check_bags(lib, device, rep, arrays, episodes, starts, C.MAX_BAG, seed, 1)


def run_bags_refusals(lib, device):
    rep = make_replay(device, C.replay_arrays("float"))
    for bag, batch in ((0, 2), (C.MAX_BAG + 1, 2), (-1, 2), (3, 0)):
        rc, bo, ba = gather(lib, device, rep, [5] * batch, [10] * batch, bag, 1, counter_of(device, 0))
        assert rc == DTQN_ERR_ARG, (bag, batch, rc)
        assert (bo == C.SENTINEL).all() and (ba == 0xEE).all()


def run_bags_host_rows(lib, device, kind):
    """rows != NULL: row r of the first list is the observation, row r of the second list the action -- the replay's action row r."""
    arrays = C.replay_arrays(kind)
    rep = make_replay(device, arrays, mask=-5.0 if kind == "float" else 9.0)
    rng = np.random.default_rng(11)
    for bag in (1, 3, 8, C.L + 25):
        batch = 7
        episodes, starts = rng.integers(0, C.E, batch), rng.integers(0, C.T - C.L + 1, batch)
        rows = rng.integers(-1, C.T + 1, (batch, 2, bag))
        rows[0, :, :] = -1
        rc, bo, ba = gather(lib, device, rep, episodes, starts, bag, 0, None, rows=rows)
        assert rc == DTQN_OK
        wo, _ = S.gather_bag(arrays, episodes, rows[:, 0], rep.obs_mask)
        _, wa = S.gather_bag(arrays, episodes, rows[:, 1], rep.obs_mask)
        assert np.array_equal(bo[:batch], wo) and np.array_equal(ba[:batch], wa), bag
        assert (bo[batch:] == C.SENTINEL).all() and (ba[batch:] == 0xEE).all()


# ---- the draw inside the update -----------------------------------------------------------------------------------------------------------
UPDATE_SEEDS = (12345, 0xFFFFFFFF)
ROW_SPLITS = {"0": 1, "1": 2, "4": 4}          # DTQN_ROW_SPLIT -> workgroups per sequence (TdEngine.row_split)


def run_update_draw(lib, device, split):
    """sample_in_forward + forward_backward leaves the oracle's (episode, start) pairs in ep_idx / start: the whole-sequence forward
    with 1, 2 and 4 workgroups per sequence (the caller has set DTQN_ROW_SPLIT), and the row-block path (DTQN_FORCE_TILED=1), which
    draws through the sample kernel.  The smallest record these paths share: context 50 in 64 rows, batch 4."""
    from helpers import make_td_case
    from oracle import dtqn_oracle as O
    cfg = O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=1, history_len=50)
    test_lib = torch.device(device).type == "cpu"
    net, _, host, eng, rep = make_td_case(lib, cfg, seed=4, batch=4, T=90, n_eps=9, mask=-5, device=device, test_lib=test_lib)
    if split == "tiled":
        assert net.tiled == 1
    else:
        assert net.tiled == 0 and eng.row_split == ROW_SPLITS[split]
    ep_len = rep.ep_len.cpu().numpy()
    assert np.array_equal(ep_len, host.episode_lengths)
    for seed in UPDATE_SEEDS:
        for step, exclude in ((0, 3), (7, 0), (2 ** 31 - 1, 8)):
            eng.step_counter[1] = step
            eng.ep_idx.fill_(exclude)           # a slot the draw never returns (and one the backward may read, were it left standing)
            eng.start.zero_()
            eng.sample_in_forward(9, exclude, seed)
            eng.forward_backward(rep)
            we, ws = S.window_draw(ep_len, 9, exclude, cfg.history_len, seed, step, np.arange(4))
            idx = eng._idx_dev.cpu().numpy()
            assert np.array_equal(idx[0], we) and np.array_equal(idx[1], ws), (split, seed, step, idx, we, ws)
            assert bool(torch.isfinite(eng.grad).all())


def run_pipelined_draw(lib, device):
    """dtqn_td_update_pipelined at draw_step = k trains on the oracle's pairs of step k, and the target pass it computes ahead for update
    k + 1 read the oracle's pairs of step k + 1: the target Q that update k + 1 then uses (it takes the pass computed ahead: the
    pipeline's `used` count says so) equals, bit for bit, the target pass run inline on the oracle's pairs of k + 1 handed in from the
    host.  Read where check_td_updates(pipelined=True) reads: _idx_dev and q3 behind eng.update()."""
    from helpers import make_td_case
    from oracle import dtqn_oracle as O
    cfg = O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50)
    test_lib = torch.device(device).type == "cpu"
    net, _, host, eng, rep = make_td_case(lib, cfg, seed=12, batch=3, T=120, n_eps=8, mask=-5, device=device, test_lib=test_lib)
    assert eng.enable_pipeline(lambda: 0) and eng._pipe["ride"]
    ep_len, seed, exclude, Bn, L = rep.ep_len.cpu().numpy(), 0xFFFFFFFF, 3, 3, cfg.history_len
    tgt0 = eng.theta_tgt.clone()
    for k in range(3):
        eng.ep_idx.fill_(exclude)               # a slot the draw never returns
        eng.start.zero_()
        eng.sample_in_forward(8, exclude, seed)
        eng.update(rep)
        we, ws = S.window_draw(ep_len, 8, exclude, L, seed, k, np.arange(Bn))
        idx = eng._idx_dev.cpu().numpy()
        assert np.array_equal(idx[0], we) and np.array_equal(idx[1], ws), (k, idx, we, ws)
        assert (eng._pipe["used"], eng._pipe["inline"]) == (k, 1) and int(eng.step_counter[1]) == k + 1
        if k == 0:
            continue
        # update k used the pass computed ahead by update k - 1.  The same pass inline, on the oracle's windows:
        assert torch.equal(eng.theta_tgt, tgt0)
        view = lambda: eng.q3.cpu().numpy().reshape(3, Bn, net.lp, net.ap)[2, :, :L, :cfg.num_actions].copy()
        ahead = view()
        eng.q3.view(3, -1)[2].fill_(float("nan"))
        eng.set_indices(we, ws)
        # (a launch of fewer than three passes only runs on windows it draws itself: all three, in the four row slices of the pass ahead)
        rc = lib.dtqn_td_forward_part(eng._net_ref, rep.view_ref, eng._td_ref, 0, 3, 4, k, eng._stream())
        assert rc == DTQN_OK
        inline = view()
        assert np.isfinite(ahead).all() and np.array_equal(ahead, inline), (k, np.abs(ahead - inline).max())
        # and on any other windows the target Q differs: the comparison can tell
        eng.set_indices(we, (ws + 1) % (np.maximum(ep_len[we] - L, 0) + 1) if (ep_len[we] > L).any() else ws)
        assert lib.dtqn_td_forward_part(eng._net_ref, rep.view_ref, eng._td_ref, 0, 3, 4, k, eng._stream()) == DTQN_OK
        assert (ep_len[we] > L).any() and not np.array_equal(view(), ahead)


def run_bag_agent_draw(lib, device):
    """A bag network behind the agent (the `bag` shape of q_f64_cases.py: width 64, context 20, bag 5; sampler "device"): after
    agent.train() the engine's windows are the oracle's and bag_obs / bag_actions are the oracle's rows gathered by the oracle.
    lib: the emulation library, or None for the hipcc-built engine on `device`."""
    from oracle import dtqn_oracle as O
    from test_bag_golden import make_bag_agent
    cfg = O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, history_len=20, bag_size=5)
    meta = dict(seed=9, B=4, T=60, n_eps=10, mask=-5.0)
    agent = make_bag_agent(lib, cfg, meta, O.init_params(cfg, seed=9, perturb=True), O.init_params(cfg, seed=10, perturb=True), device)
    agent.sampler, agent.sample_seed = "device", 12345
    rng, rb = np.random.default_rng(9), agent.replay_buffer
    for n in (60, 22, 27, 20, 5, 41, 24, 60, 33, 26):           # windows that start below row 5 (bags that are a prefix) and far above it
        obs = rng.uniform(-1, 1, (n + 1, cfg.obs_dim)).astype(np.float32)
        rb.store_obs(obs[0])
        for t in range(n):
            rb.store(obs[t + 1], int(rng.integers(0, cfg.num_actions)), float(rng.integers(-1, 2)), t == n - 1, t + 1)
        rb.flush()
    prefix = floyd = 0
    for it in range(4):
        n_valid, exclude = rb.valid_range()
        assert (n_valid, exclude) == (10, 10) and int(agent.engine.step_counter[1]) == it
        agent.train()
        eng, arrays = agent.engine, rb.export_arrays()
        we, ws = S.window_draw(arrays["eplens"], n_valid, exclude, cfg.history_len, agent.sample_seed, it, np.arange(meta["B"]))
        assert np.array_equal(eng.ep_idx.cpu().numpy(), we) and np.array_equal(eng.start.cpu().numpy(), ws), it
        rows = np.stack([S.bag_rows(agent.sample_seed, it, b, ws[b], cfg.bag_size) for b in range(meta["B"])])
        wo, wa = S.gather_bag(arrays, we, rows, meta["mask"])
        assert np.array_equal(eng.bag_obs.cpu().numpy(), wo) and np.array_equal(eng.bag_actions.cpu().numpy(), wa), it
        prefix += int((ws < cfg.bag_size).sum())
        floyd += int((ws >= cfg.bag_size).sum())
    assert prefix > 0 and floyd > 0
