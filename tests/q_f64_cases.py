"""Forward cases at the edges where a row of Q can go wrong, each held row by row to the float64 forward (q_f64_helpers.py); shared by
tests/test_emu_q_f64.py (CPU emulation) and tests/test_gpu_q_f64.py (device).  Every case runs at both weight scales -- the std-0.2
stress weights and the weight matrices times 0.1 (the init scale of helpers.make_td_case(weight_scale=0.1)) -- and asserts the property
it is named for on the net it built, so that a change of the routing cannot quietly turn it into an ordinary case."""
import ctypes

import numpy as np
import torch

from oracle import dtqn_oracle as O

from helpers import net_from_cfg, pack_theta, ptr
from q_f64_helpers import check_forward_f64, check_pooled_f64

SCALES = (1.0, 0.1)
CFG1 = dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50)
ROWBLOCK = dict(obs_dim=3, num_actions=4, inner_embed_size=128, num_heads=4, num_layers=1, history_len=130)
ROWBLOCK_N = (63, 64, 65, 128, 129, 130)

# name -> (network, kind, context lengths n, batch)
CASES = {
    # 16-row record edges of the whole-sequence kernels (64-row tile, one workgroup per sequence), residual and GRU gates
    "record_edges_res": (CFG1, "forward", (1, 2, 15, 16, 17, 31, 32, 33, 49, 50), 3),
    "record_edges_gru": (dict(CFG1, gate="gru"), "forward", (1, 2, 15, 16, 17, 31, 32, 33, 49, 50), 3),
    # dtqn_actor_forward on both sides of its two-workgroup switch (workspace given and n > 32), and with no workspace
    "actor_switch_res": (CFG1, "actor", (31, 32, 33, 34, 35, 36, 50), 2),
    "actor_switch_gru": (dict(CFG1, gate="gru"), "actor", (31, 32, 33, 34, 35, 36, 50), 2),
    # 64-row tile edges of the row-block path, whole-tile attention ...
    "rowblock_edges": (ROWBLOCK, "forward", ROWBLOCK_N, 3),
    # ... and the same net on the key-blocked attention (DTQN_ATTN_KBLOCK=1: blocks of 64 keys), the block edge at the same rows
    "kblock_edges": (ROWBLOCK, "forward", ROWBLOCK_N, 3),
    # width padding: 48 -> 64 columns with six heads of 8 (two all-zero heads), and four heads of 12 -> 16
    "padded_d48_h6": (dict(obs_dim=3, num_actions=3, inner_embed_size=48, num_heads=6, history_len=50), "forward", (1, 50), 3),
    "padded_d48_h4": (dict(obs_dim=3, num_actions=3, inner_embed_size=48, num_heads=4, history_len=50), "forward", (1, 50), 3),
    # discrete observations + action embedding + no positions (test_gpu_forward.VARIANTS[4] cut to a context of 20)
    "discrete_action_nopos": (dict(obs_dim=1, num_actions=5, inner_embed_size=64, num_heads=4, history_len=20, discrete=True, vocab_sizes=22,
                                   action_dim=8, pos="none"), "forward", (1, 2, 20), 3),
    # the bag branch: the smallest bag network of test_emu_forward.test_forward_with_a_bag
    "bag": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, history_len=20, bag_size=5), "forward", (1, 20), 3),
}
BATCH_ORDER = {"record_edges_res": (17, 50), "record_edges_gru": (33,), "rowblock_edges": (129,), "kblock_edges": (65,), "bag": (20,)}
ENV = {"actor_switch_res": {"DTQN_ROW_SPLIT": "1"}, "actor_switch_gru": {"DTQN_ROW_SPLIT": "1"},
       "rowblock_edges": {"DTQN_ATTN_KBLOCK": "0", "DTQN_TL_TRACE": "1"}, "kblock_edges": {"DTQN_ATTN_KBLOCK": "1", "DTQN_TL_TRACE": "1"}}


def scaled_params(cfg: O.NetCfg, seed: int, scale: float):
    """The perturbed parameter set with every weight MATRIX times `scale`, as helpers.make_td_case(weight_scale=scale) builds it."""
    params = O.init_params(cfg, seed=seed, perturb=True)
    if scale != 1.0:
        for k, v in params.items():
            if v.dim() >= 2 and not k.endswith("attn_mask") and k != "position_embedding.position_encoding":
                v.mul_(scale)
    return params


def _stream(device):
    if device == "cpu":
        return None
    from dtqn_amd import engine
    return engine.stream_ptr()


def run_forward(lib, net, theta, obs, act, device, bag=None):
    """Q [B, n, A] of the inference entry point the net is routed to (dtqn_forward, dtqn_forward_tiled, dtqn_forward_bag)."""
    Bn, n = obs.shape[:2]
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a.reshape(Bn, -1) if dt == np.uint8 else a, dtype=dt)).to(device)
    obs_d, act_d = dev(obs, np.float32), dev(act, np.uint8)
    q = torch.full((Bn, n, net.num_actions), float("nan"), device=device)
    need = lib.dtqn_forward_workspace_floats(ctypes.byref(net), Bn)
    ws = torch.zeros(max(1, need), device=device)
    if net.bag_size > 0:
        bo, ba = dev(bag[0], np.float32), dev(bag[1], np.uint8)
        rc = lib.dtqn_forward_bag(ctypes.byref(net), ptr(theta), ptr(obs_d), ptr(act_d), ptr(bo), ptr(ba), Bn, n, ptr(q), ptr(ws), 0, 0, 0, _stream(device))
    elif net.tiled:
        rc = lib.dtqn_forward_tiled(ctypes.byref(net), ptr(theta), ptr(obs_d), ptr(act_d), Bn, n, ptr(q), ptr(ws), _stream(device))
    else:
        rc = lib.dtqn_forward(ctypes.byref(net), ptr(theta), ptr(obs_d), ptr(act_d), Bn, n, ptr(q), _stream(device))
    assert rc == 0, rc
    if device != "cpu":
        torch.cuda.synchronize()
    return q.cpu().numpy()


def run_actor(lib, net, theta, obs, act, device, use_workspace):
    """dtqn_actor_forward on one sequence obs [n, O], act [n] -> (Q of the rows [n, A], Q of the newest row as the host receives it,
    True if the exchange area of the workspace was written: the two workgroups of latency mode handed rows over)."""
    L, Od, A, n = net.ctx_len, net.obs_dim, net.num_actions, obs.shape[0]
    pin = (lambda t: t.pin_memory()) if device != "cpu" else (lambda t: t)
    ctx_h = pin(torch.zeros(L * Od * 4 + L, dtype=torch.uint8))
    c = ctx_h.numpy()
    c[:L * Od * 4].view(np.float32).reshape(L, Od)[:n] = obs
    c[L * Od * 4:][:n] = act
    ctx_d = torch.zeros_like(ctx_h, device=device)
    q_d = torch.full((L, A), float("nan"), device=device)
    q_last = pin(torch.full((A,), float("nan")))
    need = lib.dtqn_forward_workspace_floats(ctypes.byref(net), 1)
    assert need > 0
    ws = torch.zeros(need, device=device) if use_workspace else None
    rc = lib.dtqn_actor_forward(ctypes.byref(net), ptr(theta), ptr(ctx_h), ptr(ctx_d), n, ptr(q_d), ptr(q_last), ptr(ws), 0, 0, 0, _stream(device))
    assert rc == 0, rc
    if device != "cpu":
        torch.cuda.synchronize()
    xch = lib.dtqn_td_xch_floats(ctypes.byref(net), 1)
    exchanged = ws is not None and bool(ws[:xch].any())
    if ws is not None:
        assert not ws[xch:].any()                      # hand-over flags lowered again
    return q_d.cpu().numpy()[:n], q_last.numpy().copy(), exchanged


def assert_property(lib, name, cfg, net):
    """The routing the case is named for."""
    if name.startswith(("record_edges", "actor_switch")):
        assert net.tiled == 0 and net.lp == 64 and net.d_real == 0, (net.tiled, net.lp)
    if name.startswith("actor_switch"):
        assert lib.dtqn_td_row_split(ctypes.byref(net), 1) >= 2            # latency mode exists for this net
    if name in ("rowblock_edges", "kblock_edges"):
        assert net.tiled == 1 and net.lp == 192 and net.head_dim == 32, (net.tiled, net.lp, net.head_dim)
    if name == "padded_d48_h6":
        assert net.tiled == 0 and net.d_real == 48 and net.d_model == 64 and net.head_dim == 8
    if name == "padded_d48_h4":
        assert net.tiled == 0 and net.d_real == 48 and net.d_model == 64 and net.head_dim == 16      # heads of 12 on 16 columns
    if name == "discrete_action_nopos":
        assert net.tiled == 0 and cfg.discrete and cfg.action_dim == 8 and cfg.pos == "none"
    if name == "bag":
        assert net.tiled == 1 and net.bag_size == 5


def run_case(lib, name, scale, device="cpu", assert_=True):
    """-> figures of every check of the case (q_f64_helpers.check_q_f64), the environment of ENV[name] set by the caller."""
    kw, kind, ns, Bn = CASES[name]
    cfg = O.NetCfg(**kw)
    params = scaled_params(cfg, seed=3, scale=scale)
    net = net_from_cfg(lib, cfg)
    assert_property(lib, name, cfg, net)
    theta = torch.from_numpy(pack_theta(net, params)).to(device)
    rng = np.random.default_rng(5)
    draw = lambda b, m: (rng.integers(0, cfg.vocab_sizes, size=(b, m, cfg.obs_dim)) if cfg.discrete
                         else rng.uniform(-1, 1, size=(b, m, cfg.obs_dim)).astype(np.float32))
    pool = []              # one yardstick for the case: D32 over the rows of every context length (and every actor call)
    for n in ns:
        obs, act = draw(Bn, n), rng.integers(0, cfg.num_actions, size=(Bn, n, 1))
        bag = (draw(Bn, cfg.bag_size), rng.integers(0, cfg.num_actions, size=(Bn, cfg.bag_size, 1))) if cfg.bag_size else None
        if kind == "forward":
            q = run_forward(lib, net, theta, obs, act, device, bag)
            check_forward_f64(cfg, params, obs, act, q, bag=bag, what=(name, scale, n), pool=pool)
            if n in BATCH_ORDER.get(name, ()):          # a row's Q must not depend on its neighbours in the batch: bit for bit
                for b in range(Bn):
                    alone = run_forward(lib, net, theta, obs[b:b + 1], act[b:b + 1], device, None if bag is None else (bag[0][b:b + 1], bag[1][b:b + 1]))
                    assert np.array_equal(alone[0], q[b]), (name, scale, n, b, float(np.abs(alone[0] - q[b]).max()))
        else:
            for b in range(Bn):
                for use_ws in ((True, False) if b == 0 else (True,)):
                    q, q_last, exchanged = run_actor(lib, net, theta, obs[b].astype(np.float32), act[b, :, 0], device, use_ws)
                    assert exchanged == (use_ws and n > 32), (name, n, use_ws, exchanged)      # two workgroups exactly beyond 32 rows
                    assert np.array_equal(q_last, q[n - 1])
                    check_forward_f64(cfg, params, obs[b:b + 1], act[b:b + 1], q[None], what=(name, scale, n, b, use_ws), pool=pool)
    figs = check_pooled_f64(pool, assert_=assert_)
    if scale == 0.1:
        # at init-scale weights |Q| < 1 and the asserted bound on |Q - Q64| is of order 1e-6 (the flat rule: an absolute 1e-4); a property
        # of the references alone (margin * D32 * s)
        assert max(f["q_abs_max"] for f in figs) < 1.0 and max(f["abs_bound"] for f in figs) < 1e-5, [(f["q_abs_max"], f["abs_bound"]) for f in figs]
    return figs


def assert_trace(name, err):
    """The attention kernels the row-block cases launched (DTQN_TL_TRACE=1 on stderr)."""
    kb, whole = "tl_attn_kb_kernel" in err, "tl_launch (tl_attn_kernel<" in err
    if name == "rowblock_edges":
        assert whole and not kb, err[-2000:]
    if name == "kblock_edges":
        assert kb and not whole, err[-2000:]
