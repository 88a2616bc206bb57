"""TD updates under dropout at contexts beyond 256 rows, where the keep-mask key of an attention probability needs the ninth bit of
its query row and key (dtqn_device.hpp drop_attn_idx); shared by tests/test_emu_dropout_long.py (CPU emulation) and
tests/test_gpu_dropout_long.py (device).  Every case is one update of helpers.check_td_updates at batch 2 and p = 0.3 -- the float64
gradient, Q and statistics checks under the oracle's masks -- on full windows (every episode as long as the context, so rows from 256
up are live), and asserts the routing it exists for: the launch trace names the kernel family.

What this binds: a keep decision of the kernels that differs from the oracle's on a probability of ordinary size moves its row of Q
far beyond 16 x D32.  A probability that is negligible is not bound, whatever its mask."""
import numpy as np

from oracle import dtqn_oracle as O

from helpers import check_td_updates, make_td_case

P = 0.3
SEED = 4242
_BASE = dict(obs_dim=3, num_actions=4, num_layers=1, dropout=P)

# name -> (network, batch, what the trace must name, what it must not)
CASES = {
    # tl_attn_kernel / tl_attn_bwd_kernel with query rows and keys from 256 up: heads of 16 on the whole-head tile at 320 padded rows
    "whole_tile_h16": (dict(_BASE, inner_embed_size=64, num_heads=4, history_len=260), 2,
                       ("tl_launch (tl_attn_kernel<", "tl_launch (tl_attn_bwd_kernel<"), ("tl_attn_kb_",)),
    # sixteen heads of 4: odd and even heads, more than eight of them
    "whole_tile_h4": (dict(_BASE, inner_embed_size=64, num_heads=16, history_len=260), 2,
                      ("tl_launch (tl_attn_kernel<", "tl_launch (tl_attn_bwd_kernel<"), ("tl_attn_kb_",)),
    # heads of 32 at 320 padded rows do not fit the tile: tl_attn_kb_* with DROP, the key blocks from the fifth on past 256
    "key_blocked": (dict(_BASE, inner_embed_size=128, num_heads=4, history_len=260), 2,
                    ("tl_attn_kb_kernel<", "tl_attn_kb_dkv_kernel<", "tl_attn_kb_dq_kernel<"), ("tl_launch (tl_attn_kernel<", "tl_launch (tl_attn_bwd_kernel<")),
    # the same kernels at the largest context: query rows and keys up to 511
    "full_context": (dict(_BASE, inner_embed_size=128, num_heads=4, history_len=512), 1,
                     ("tl_attn_kb_kernel<", "tl_attn_kb_dkv_kernel<", "tl_attn_kb_dq_kernel<"), ("tl_launch (tl_attn_kernel<", "tl_launch (tl_attn_bwd_kernel<")),
    # resident bag kernels with query rows from 256 up
    "small_bag": (dict(_BASE, inner_embed_size=64, num_heads=8, history_len=260, bag_size=5), 2,
                  ("tl_launch tl_bag_attn_kernel", "tl_launch tl_bag_attn_bwd_kernel"), ("tl_bag_attn_mfma_",)),
    # a bag the resident tile cannot hold: the matrix-core bag kernels with bag entries from 256 up
    "large_bag": (dict(_BASE, inner_embed_size=64, num_heads=8, history_len=260, bag_size=300), 2,
                  ("tl_bag_attn_mfma_kernel<", "tl_bag_attn_mfma_dkv_kernel<", "tl_bag_attn_mfma_dq_kernel<"),
                  ("tl_launch tl_bag_attn_kernel", "tl_launch tl_bag_attn_bwd_kernel")),
}
ENV = {"DTQN_TL_TRACE": "1"}
AUTOGRAD = "key_blocked"                # the net of the differentiable-forward case (dtqn_forward_train_drop / dtqn_backward_dq_drop)
AUTOGRAD_ROWS, AUTOGRAD_BATCH = 260, 2


def assert_property(name, cfg, net):
    """The shape the case is named for, as dtqn_net_init laid it out."""
    L = cfg.history_len
    assert net.tiled == 1 and net.dropout > 0 and net.ctx_len == L > 256 and net.lp == (L + 63) // 64 * 64, (net.tiled, net.lp)
    want = {"whole_tile_h16": 16, "whole_tile_h4": 4, "key_blocked": 32, "full_context": 32, "small_bag": 8, "large_bag": 8}[name]
    assert net.head_dim == want and net.d_real == 0, (net.head_dim, net.d_real)
    if name == "whole_tile_h4":
        assert net.num_heads == 16
    if name == "small_bag":
        assert net.bag_size == 5
    if name == "large_bag":
        assert net.bag_size == 300 > 256


def assert_trace(name, err):
    _, _, named, absent = CASES[name]
    for k in named:
        assert k in err, (name, k, err[-2000:])
    for k in absent:
        assert k not in err, (name, k, err[-2000:])


def run_case(lib, name, device="cpu", test_lib=True, report_as=None):
    """One update of the case against the oracle -> the worst figures of check_td_updates.  The caller has set ENV and reads the trace."""
    kw, batch, _, _ = CASES[name]
    cfg = O.NetCfg(**kw)
    L = cfg.history_len
    net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=31, batch=batch, T=L + 8, n_eps=3, mask=-5, device=device, test_lib=test_lib,
                                               min_len=L)
    assert_property(name, cfg, eng.net)
    eng.td.dropout_seed = SEED

    def full_windows(it, eps, starts, batch_):
        assert (host.episode_lengths[eps] - starts >= L).all(), (eps, starts)       # rows from 256 up are live in every window
    worst = check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1, on_batch=full_windows, report_as=report_as)
    return worst


def show(name, worst):
    print("dropout beyond 256 rows", name, {k: worst[k] for k in ("q64_over_d32", "q64_d32", "q64_row", "grad64_over_d32", "grad64_group",
                                                                   "stat64_over_bound", "q_abs_err", "q_abs_max", "grad_err_over_max")})


def run_autograd_case(lib, device="cpu"):
    """The differentiable forward of the key-blocked net on 260 rows under the masks of one (seed, step): Q, every parameter's gradient
    and obss.grad against the oracle (autograd_dropout_helpers.check_dropout_parity, float64 check included)."""
    from autograd_dropout_helpers import check_dropout_parity
    from autograd_helpers import make_inputs, make_module
    cfg = O.NetCfg(**CASES[AUTOGRAD][0])
    params = O.init_params(cfg, seed=3, perturb=True)
    m = make_module(lib, cfg, params, device=device)
    assert_property(AUTOGRAD, cfg, m.net)
    obs, act, bag, w = make_inputs(cfg, AUTOGRAD_BATCH, AUTOGRAD_ROWS, seed=5)
    report = {}
    check_dropout_parity(m, cfg, params, obs, act, bag, w, device=device, report=report)
    return report
