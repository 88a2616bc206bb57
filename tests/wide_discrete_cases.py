"""Discrete observations beyond the resident embedding-gradient kernel (more than 128 gathered columns, or scatter tables beyond LDS):
the cases shared by the CPU-emulation tests (test_emu_wide_discrete.py) and the -m gpu tests (test_gpu_wide_discrete.py).  Everything goes
through make_td_case / check_td_updates with their tolerances: Q of the three forwards, the flat gradient, statistics, the first Adam step."""
import re

import numpy as np
import pytest
import torch

from dtqn_amd import _binding as B
from oracle import dtqn_oracle as O

from helpers import check_td_updates, fill_device_replay, make_td_case

PANEL, RESIDENT = "tl_embed_bwd_panel_kernel", "tl_embed_bwd_kernel"


def _cfg(tokens, vocab, e=8, d=128, heads=8, ctx=70, **kw):
    return dict(obs_dim=tokens, num_actions=4, embed_per_obs_dim=e, inner_embed_size=d, num_heads=heads, num_layers=1, history_len=ctx,
                discrete=True, vocab_sizes=vocab, **kw)


# (id, network, batch, what it can get wrong)
CASES = [
    ("17x12", _cfg(17, 12), 2, "second panel of 8 columns; second row block with 6 live rows"),
    ("25x12_e6", _cfg(25, 12, e=6), 2, "ke = 150: slots straddle a 128-column boundary, kep != ke"),
    ("6x1000", _cfg(6, 1000, d=64, heads=4), 2, "large vocabulary alone (ke = 48): zero-fill and flush of a wide table partial"),
    ("49x300", _cfg(49, 300, d=256, ctx=130), 1, "four panels, three row blocks"),
    ("20x40_bag", _cfg(20, 40, d=64, heads=4, action_dim=8, bag_size=5), 2, "bag pass adds to the context's partials; action columns in front"),
    ("17x12_dropout", _cfg(17, 12, dropout=0.1), 2, "DROP_EMB mask in front of the new kernel"),
    ("17x12_gru_identity", _cfg(17, 12, gate="gru", identity=True), 2, "the separate-launch backward"),
    ("25x12_ctx50", _cfg(25, 12, d=64, ctx=50), 2, "short context with kep > 3 d_model: placed on the row-block path at construction"),
    ("128x8", _cfg(128, 8, d=64, heads=4, ctx=20), 1, "the admitted bounds themselves (ke = 1024)"),
    ("2x12_e200", _cfg(2, 12, e=200), 2, "a slot wider than a panel: walked in pieces, flushed from several panels at a column offset"),
]
CASE_IDS = [c[0] for c in CASES]
TODAY = _cfg(10, 9)                    # ke = 80 and 10 x 9 x 8 table floats per row group: the resident kernel's ground


def dev_kw(gpu):
    return dict(device="cuda", test_lib=False) if gpu else {}


def td_case(lib, kw, batch, gpu, seed=17):
    cfg = O.NetCfg(**kw)
    net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=seed, batch=batch, T=cfg.history_len + 8, n_eps=3, mask=cfg.vocab_sizes - 1,
                                               **dev_kw(gpu))
    return cfg, net, oracle, host, eng, rep


def launched(err):
    return set(re.findall(r"tl_launch (\w+)", err))


def run_case(lib, case, gpu, capfd):
    """One update against the oracle with the launch trace on (the caller has set DTQN_TL_TRACE=1): the embedding gradient of every case
    runs on the panel kernel and not on the resident one."""
    name, kw, batch, _ = case
    cfg, net, oracle, host, eng, rep = td_case(lib, kw, batch, gpu)
    assert eng.net.tiled == 1 and eng.net.lp == (cfg.history_len + 63) // 64 * 64
    if name == "25x12_ctx50":
        assert net.tiled == 1 and net.lp == 64
    capfd.readouterr()
    check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1)
    if gpu:
        torch.cuda.synchronize()
    names = launched(capfd.readouterr().err)
    assert PANEL in names and RESIDENT not in names, sorted(names)


def run_traced(lib, kw, batch, gpu, capfd):
    """One update with the launch trace on; the set of kernel names it went through."""
    cfg, net, oracle, host, eng, rep = td_case(lib, kw, batch, gpu)
    capfd.readouterr()
    check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1)
    if gpu:
        torch.cuda.synchronize()
    return launched(capfd.readouterr().err)


def run_collisions(lib, fill, gpu):
    """Worst case of the first-occurrence scatter: every row of a block names the same table row (`same`), or one of two (`two`).  One
    update against the oracle, then the same forward + backward twice from the same state: bit-equal Q and gradient."""
    kw = _cfg(17, 12) if fill == "same" else _cfg(17, 2)
    cfg, net, oracle, host, eng, rep = td_case(lib, kw, 2, gpu, seed=23)
    if fill == "same":
        host.obss[...] = 3.0
    else:
        host.obss[...] = np.random.default_rng(5).integers(0, 2, size=host.obss.shape).astype(host.obss.dtype)
    fill_device_replay(rep, host)
    check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1)
    eps, starts = host.sample_indices(eng.batch)
    out = []
    for _ in range(2):
        eng.set_indices(eps, starts)
        eng.forward_backward(rep)
        if gpu:
            torch.cuda.synchronize()
        out.append((eng.q3.clone(), eng.grad.clone()))
    assert torch.isfinite(out[0][1]).all() and float(out[0][1].abs().max()) > 0
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def check_construction(lib):
    """Each bound + 1 is refused by B.make_net, and the message names the three bounds; d_model 32 keeps its own bound."""
    tok, cols, tab = B.DISCRETE_LIMITS
    base = dict(num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=20, discrete=True)
    ok = B.make_net(lib, obs_dim=tok, embed_per_obs_dim=cols // tok, vocab_sizes=tab // (cols // tok), **base)
    assert ok.tiled == 1 and ok.ke == cols
    for kw in (dict(obs_dim=tok + 1, embed_per_obs_dim=1, vocab_sizes=8),                       # 129 tokens
               dict(obs_dim=43, embed_per_obs_dim=24, vocab_sizes=8),                           # ke = 1032
               dict(obs_dim=4, embed_per_obs_dim=8, vocab_sizes=tab // 8 + 1)):                 # vocab * e = 65 544
        with pytest.raises(NotImplementedError) as exc:
            B.make_net(lib, **base, **kw)
        for bound in (tok, cols, tab):
            assert f"<= {bound}" in str(exc.value), str(exc.value)
    with pytest.raises(NotImplementedError):       # d_model 32 lives on the whole-sequence kernels only: kep = 104 > 96 stays refused
        B.make_net(lib, obs_dim=13, embed_per_obs_dim=8, vocab_sizes=8, **dict(base, inner_embed_size=32, history_len=12))
    assert B.make_net(lib, obs_dim=12, embed_per_obs_dim=8, vocab_sizes=8, **dict(base, inner_embed_size=32, history_len=12)).tiled == 0


def run_agent(agent, env):
    """Prepopulate 300 steps, three updates with finite statistics, one greedy action through the actor."""
    import run as runpy
    assert agent.policy_network.net.tiled == 1 and agent.policy_network.net.obs_dim == 20
    runpy.prepopulate(agent, 300, [env])
    theta0 = agent.policy_network.flat.clone()
    agent.context_reset(env.reset())
    for _ in range(3):
        agent.train()
    assert agent.num_train_steps == 3
    for stat in (agent.td_errors, agent.grad_norms, agent.qvalue_max, agent.qvalue_min):
        assert np.isfinite(stat.mean())
    assert not torch.equal(theta0, agent.policy_network.flat)
    action = agent.get_action(0.0)
    assert 0 <= int(action) < env.action_space.n


def memory_env(seed):
    from dtqn_amd.envs.memory_cards import Memory
    from dtqn_amd.envs.time_limit import TimeLimit
    from dtqn_amd.utils.random import set_global_seed
    env = TimeLimit(Memory(num_pairs=10), 50)     # 20 tokens over a vocabulary of 12 (+ the mask): built directly, not through the registry
    set_global_seed(seed, env)
    return env
