"""The prologue of the four-slice backward chain (dtqn_backward.hip: loss rows loaded unconditionally in front of the prefetch batch,
every dq row written by the loss wave itself, head.2 staged through LDS) as the pipelined update runs it, on the CPU emulation.
Each case is the smallest shape that reaches one path of that prologue; the device half is tests/test_gpu_bwd_prologue.py.

  ctx50            context 50, history 50, 3 actions: the top slice (rows 48 .. 63) has two live rows
  ctx48, ctx33     the uppermost slice (ctx48) / the uppermost slice and all but one row of the next (ctx33) hold no live row: every
                   unconditional load of those lanes lands on its stand-in (the window's first row)
  hist10           loss rows 40 .. 49 straddle slices 2 and 3; slices 0 and 1 own none and still publish zero dq rows and the
                   statistics partials of an empty slice
  A5               five actions: a Q row is two float4s (AP = 8)
  ties             head.2 weights zero and equal biases in the policy network, distinct target biases: Q_pol(o') is an exact tie in every
                   row, torch.argmax takes index 0, and any other choice shows in y (statistics and gradients)
  NaN rewards      the reward rows no window can reach are NaN; the same updates from the same state with and without them give the same
                   bits -- a stand-in or padding row dropped by a product instead of a select would spread the NaN"""
import numpy as np
import pytest
import torch

from dtqn_amd import _binding as B
from oracle import dtqn_oracle as O

from helpers import make_td_case, check_td_updates, pack_theta

BASE = dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50)
# name -> (network, loss history (None: the context), batch, updates)
CASES = {
    "ctx50": (BASE, None, 3, 2),
    "ctx48": (dict(BASE, history_len=48), None, 2, 2),
    "ctx33": (dict(BASE, history_len=33), None, 2, 2),
    "hist10": (BASE, 10, 3, 2),
    "A5": (dict(BASE, num_actions=5), None, 2, 2),
}


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


def make_case(lib, kw, history, batch, seed=31, **where):
    """A pipelined four-slice case: the update the benchmark times, at a small batch."""
    cfg = O.NetCfg(**kw)
    net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=seed, batch=batch, T=cfg.history_len + 20, n_eps=batch + 6, mask=-5,
                                               history=history, **where)
    assert net.lp == 64 and eng.row_split == 4 and eng.enable_pipeline(lambda: 0) and eng._pipe["ride"]
    return cfg, net, oracle, host, eng, rep


def run_case(lib, name, **where):
    kw, history, batch, updates = CASES[name]
    cfg, net, oracle, host, eng, rep = make_case(lib, kw, history, batch, **where)
    w = check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=updates, pipelined=True)
    assert w["pipeline"]["used"] >= updates - 1, w["pipeline"]      # the pass computed ahead was what the loss read


def run_ties(lib, **where):
    cfg, net, oracle, host, eng, rep = make_case(lib, BASE, None, 2, **where)
    with torch.no_grad():
        oracle.pol["ffn.2.weight"].zero_()
        oracle.pol["ffn.2.bias"].fill_(0.25)
        oracle.tgt["ffn.2.bias"].copy_(torch.tensor([0.5, -0.75, 1.5]))
    eng.theta_pol.copy_(torch.from_numpy(pack_theta(net, oracle.pol)))
    eng.theta_tgt.copy_(torch.from_numpy(pack_theta(net, oracle.tgt)))
    check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1, pipelined=True)
    L, A = cfg.history_len, cfg.num_actions
    q3 = eng.q3.cpu().numpy().reshape(3, eng.batch, net.lp, net.ap)[:, :, :L, :A]
    assert (q3[1] == np.float32(0.25)).all()                         # the tie is exact, in every row
    assert np.ptp(q3[2], axis=-1).min() > 0.5                        # ... and the choice matters


def unreachable_reward_rows(host, ctx):
    """[slots][T] mask of the reward rows behind every episode's last step that no window of the context reaches: a window starts at
    most at max(0, len - ctx), and the window of an episode shorter than the context reads that episode's (zero) padding up to ctx."""
    T = host.rewards.shape[1]
    return np.arange(T)[None, :] >= np.maximum(host.episode_lengths.astype(np.int64), ctx)[:, None]


def run_nan_rewards(lib, **where):
    kw, history, batch, updates = CASES["ctx50"]
    out = []
    for poison in (False, True):
        cfg, net, oracle, host, eng, rep = make_case(lib, kw, history, batch, **where)
        if poison:
            m = unreachable_reward_rows(host, cfg.history_len)
            lens = host.episode_lengths[:host.pos[0]]
            assert (m[:host.pos[0]].any(axis=1) | (lens >= m.shape[1])).all()      # behind EVERY stored episode that ends inside its slot
            rep.rewards[torch.from_numpy(m).to(rep.rewards.device)] = float("nan")
            assert bool(torch.isnan(rep.rewards).any())
        n_valid, exclude = min(host.pos[0], host.max_size), host.pos[0] % host.max_size
        stats = []
        for _ in range(updates):
            eng.sample_in_forward(n_valid, exclude, 1234)
            eng.update(rep)
            stats.append(eng.read_stats())
        out.append((stats, [x.detach().cpu().clone() for x in (eng.theta_pol, eng.adam_m, eng.adam_v, eng.grad, eng.q3, eng._idx_dev)]))
    (s0, t0), (s1, t1) = out
    assert s0 == s1 and all(np.isfinite(list(s.values())).all() for s in s0), (s0, s1)
    for a, b in zip(t0, t1):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b)


@pytest.mark.parametrize("name", sorted(CASES))
def test_prologue_paths_vs_oracle(emu, name):
    run_case(emu, name)


def test_exact_ties_take_the_first_maximum(emu):
    run_ties(emu)


def test_nan_rewards_behind_every_episode_change_no_bit(emu):
    run_nan_rewards(emu)
