"""Launch sequences of the row-block path (dtqn_tiled.hip) on the CPU emulation, held against a recording.

forward_records / backward_records decide which kernel instantiations a pass runs from the switches of dtqn_tl_switch.hpp and the shape of
the pass (TlFwdPlan / TlBwdPlan).  Every case here is one TD update (or one inference forward, or one differentiable forward + backward) under
one setting of the switches; DTQN_TL_TRACE=1 prints a line per launch -- kernel, grid, block, dynamic LDS -- and the ordered list of
(kernel base name, grid, block, lds), with dtqn_debug_last_packed_blocks() where a fused-layer launch happened, must equal
tests/golden/tl_launch_trace.json.  That file was recorded (`python tests/test_tl_launch_plan.py --record PATH`) from the commit before the
plans existed, with nothing but the geometry added to its trace line, with the packed-rows case last (there a 32-row layer launch left the
packed-blocks hook at its previous value).  Arithmetic is not compared here: test_emu_td.py and its neighbours hold the same paths against
the oracle.

The start-skew switches (DTQN_SKEW_*) only change a kernel argument of launches of 640 .. 896 workgroups, which no emulated shape reaches:
their cases pin that setting them moves no launch."""
import contextlib
import ctypes
import json
import os
import re
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
GOLDEN_FILE = os.path.join(HERE, "golden", "tl_launch_trace.json")
SWITCH_HEADER = os.path.join(REPO, "dtqn_amd", "csrc", "dtqn_tl_switch.hpp")

# every switch of dtqn_tl_switch.hpp: a switch added there without a case here fails test_every_switch_has_a_case
SWITCHES = [
    "DTQN_TL_TRACE", "DTQN_NO_WIDE", "DTQN_ATTN_KBLOCK", "DTQN_BAG_ATTN_MFMA", "DTQN_LAYER_FUSE", "DTQN_QKV_FUSE", "DTQN_EMBED_QKV",
    "DTQN_PACK_ROWS", "DTQN_HEAD_FUSE", "DTQN_BWD_CHAIN", "DTQN_BWD_CHAIN256", "DTQN_FFN_BWD", "DTQN_FFN_ROWS", "DTQN_ROWS_FFN",
    "DTQN_ROWS_FFNB", "DTQN_ROWS_WIDE", "DTQN_GEMM_ROWS", "DTQN_SKEW_TICKS", "DTQN_SKEW_WIDE", "DTQN_SKEW_LAYER", "DTQN_WPACK",
    "DTQN_EMBED_TABLE",
]

# networks (oracle NetCfg keywords) and the TD case they run in: the configurations of test_emu_td.py
NETS = {
    "d128": (dict(obs_dim=3, num_actions=3, inner_embed_size=128, num_heads=8, num_layers=2, history_len=20), dict(batch=2, T=30, mask=-5)),
    "d128_discrete": (dict(obs_dim=6, num_actions=5, inner_embed_size=128, num_heads=8, num_layers=1, history_len=20, discrete=True, vocab_sizes=9),
                      dict(batch=3, T=30, mask=8)),
    "d128_ctx48": (dict(obs_dim=6, num_actions=5, inner_embed_size=128, num_heads=8, num_layers=2, history_len=48, discrete=True, vocab_sizes=9),
                   dict(batch=4, T=58, mask=8)),
    "d64": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=20), dict(batch=2, T=30, mask=-5)),
    "d64_gru": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=4, num_layers=2, history_len=20, gate="gru"), dict(batch=2, T=30, mask=-5)),
    "d64_identity": (dict(obs_dim=6, num_actions=5, inner_embed_size=64, num_heads=8, num_layers=1, history_len=12, discrete=True, vocab_sizes=9,
                          action_dim=4, identity=True, pos="sin"), dict(batch=3, T=20, mask=8)),
    "d48_padded": (dict(obs_dim=3, num_actions=3, inner_embed_size=48, num_heads=4, num_layers=1, history_len=20), dict(batch=2, T=30, mask=-5)),
    "d256": (dict(obs_dim=3, num_actions=4, inner_embed_size=256, num_heads=8, num_layers=1, history_len=12, action_dim=8), dict(batch=2, T=20, mask=-5)),
    "d64_bag": (dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=20, action_dim=4, bag_size=5),
                dict(batch=2, T=28, mask=-5)),
    "d64_dropout": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=20, dropout=0.1), dict(batch=3, T=30, mask=-5)),
}
R64 = {"DTQN_FFN_ROWS": "64"}          # (the small-launch rule picks 32-row workgroups at every emulated shape; the fused variants exist at 64)

# (id, net, what runs, switch settings).  Order matters to the recorder only: the packed launch comes last.
CASES = [
    ("d128-defaults", "d128", "td", {}),
    ("d128-rows64", "d128", "td", R64),
    ("d128-rows64-layer_fuse0", "d128", "td", {**R64, "DTQN_LAYER_FUSE": "0"}),
    ("d128-rows64-qkv_fuse0", "d128", "td", {**R64, "DTQN_QKV_FUSE": "0"}),
    ("d128-rows64-head_fuse0", "d128", "td", {**R64, "DTQN_HEAD_FUSE": "0"}),
    ("d128-rows64-bwd_chain0", "d128", "td", {**R64, "DTQN_BWD_CHAIN": "0"}),
    ("d128-rows64-ffn_bwd0", "d128", "td", {**R64, "DTQN_FFN_BWD": "0"}),
    ("d128-no_wide", "d128", "td", {"DTQN_NO_WIDE": "1"}),
    ("d128-gemm_rows32", "d128", "td", {"DTQN_GEMM_ROWS": "32"}),
    ("d128-gemm_rows_auto", "d128", "td", {"DTQN_GEMM_ROWS": "auto"}),
    ("d128-rows_wide32", "d128", "td", {"DTQN_ROWS_WIDE": "32"}),
    ("d128-rows_ffn64", "d128", "td", {"DTQN_ROWS_FFN": "64"}),
    ("d128-rows_ffnb64", "d128", "td", {"DTQN_ROWS_FFNB": "64"}),
    ("d128-attn_kblock", "d128", "td", {"DTQN_ATTN_KBLOCK": "1"}),
    ("d128-skew_ticks", "d128", "td", {**R64, "DTQN_SKEW_TICKS": "0"}),
    ("d128-skew_wide_layer", "d128", "td", {**R64, "DTQN_SKEW_WIDE": "0", "DTQN_SKEW_LAYER": "0"}),
    ("d128-inference", "d128", "forward", {}),
    ("d128-inference-untraced", "d128", "forward", {"DTQN_TL_TRACE": None}),
    ("d128-autograd", "d128", "autograd", {}),
    ("discrete-table0-qkv0", "d128_discrete", "td", {"DTQN_EMBED_TABLE": "0", "DTQN_EMBED_QKV": "0"}),
    ("discrete-table0-qkv1", "d128_discrete", "td", {"DTQN_EMBED_TABLE": "0", "DTQN_EMBED_QKV": "1"}),
    ("discrete-table1-qkv0", "d128_discrete", "td", {"DTQN_EMBED_TABLE": "1", "DTQN_EMBED_QKV": "0"}),
    ("discrete-table1-qkv1", "d128_discrete", "td", {"DTQN_EMBED_TABLE": "1", "DTQN_EMBED_QKV": "1"}),
    ("discrete-wpack0", "d128_discrete", "td", {"DTQN_WPACK": "0"}),
    ("d64-residual", "d64", "td", {}),
    ("d64-gru", "d64_gru", "td", {}),
    ("d64-identity", "d64_identity", "td", {}),
    ("d48-padded", "d48_padded", "td", {}),
    ("d256-chain0", "d256", "td", {"DTQN_BWD_CHAIN256": "0"}),
    ("d256-chain1", "d256", "td", {"DTQN_BWD_CHAIN256": "1"}),
    ("bag-mfma0", "d64_bag", "td", {"DTQN_BAG_ATTN_MFMA": "0"}),
    ("bag-mfma1", "d64_bag", "td", {"DTQN_BAG_ATTN_MFMA": "1"}),
    ("dropout", "d64_dropout", "td", {}),
    ("ctx48-pack0", "d128_ctx48", "td", {**R64, "DTQN_PACK_ROWS": "0"}),
    ("ctx48-pack1", "d128_ctx48", "td", {**R64, "DTQN_PACK_ROWS": "1"}),
]

LINE = re.compile(r"^tl_launch \(?(\w+).* grid=(\d+),(\d+),(\d+) block=(\d+) lds=(\d+)$")


@contextlib.contextmanager
def captured_stderr(out: list):
    """File descriptor 2 into a temporary file while the block runs (the trace is written by the library's fprintf)."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            yield
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            tmp.seek(0)
            out.append(tmp.read().decode())


@contextlib.contextmanager
def switches(env: dict):
    """The process environment with exactly these row-block switches (None: unset), DTQN_TL_TRACE=1 and DTQN_FORCE_TILED=1."""
    keep = {k: os.environ.get(k) for k in SWITCHES + ["DTQN_FORCE_TILED"]}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ["DTQN_FORCE_TILED"] = "1"
        for k, v in {"DTQN_TL_TRACE": "1", **env}.items():
            if v is not None:
                os.environ[k] = v
        yield
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run_case(lib, net_name, what, env):
    """-> {"launches": [[kernel base name, [gx, gy, gz], block, lds], ...], "packed_blocks": int | None}"""
    import torch
    from dtqn_amd import _binding as B
    from oracle import dtqn_oracle as O
    from helpers import make_td_case, net_from_cfg, pack_theta, ptr
    kw, run = NETS[net_name]
    cfg = O.NetCfg(**kw)
    err = []
    with switches(env):
        if what == "td":
            net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=33, batch=run["batch"], T=run["T"], n_eps=6, mask=run["mask"])
            assert eng.net.tiled == 1 and (eng.net.d_real > 0) == (net_name == "d48_padded")
            eps, starts = host.sample_indices(run["batch"])
            eng.set_indices(eps, starts)
            if cfg.bag_size > 0:
                rng = np.random.Generator(np.random.PCG64(77))
                eng.set_bag(rng.random((run["batch"], cfg.bag_size, cfg.obs_dim), dtype=np.float32),
                            rng.integers(0, cfg.num_actions, (run["batch"], cfg.bag_size, 1)))
            with captured_stderr(err):
                eng.forward_backward(rep)
        else:
            net = net_from_cfg(lib, cfg)
            assert net.tiled == 1
            Bn, n = 2, cfg.history_len - 3
            theta = pack_theta(net, O.init_params(cfg, seed=3, perturb=True))
            rng = np.random.default_rng(5)
            obs = rng.uniform(-1, 1, (Bn, n, cfg.obs_dim)).astype(np.float32)
            q = np.zeros((Bn, n, cfg.num_actions), np.float32)
            nb = ctypes.byref(net)
            if what == "forward":
                ws = np.zeros(lib.dtqn_forward_workspace_floats(nb, Bn), np.float32)
                with captured_stderr(err):
                    assert lib.dtqn_forward_tiled(nb, ptr(theta), ptr(obs), None, Bn, n, ptr(q), ptr(ws), None) == 0
            else:
                ws = np.zeros(lib.dtqn_grad_workspace_floats(nb, Bn, n), np.float32)
                dq = rng.normal(size=q.shape).astype(np.float32)
                grad, dobs = np.zeros(net.n_trainable, np.float32), np.zeros_like(obs)
                with captured_stderr(err):
                    assert lib.dtqn_forward_train_drop(nb, ptr(theta), ptr(obs), None, None, None, Bn, n, ptr(q), ptr(ws), 7, -1, None) == 0
                    assert lib.dtqn_backward_dq_drop(nb, ptr(theta), ptr(obs), None, None, None, Bn, n, ptr(dq), ptr(ws), ptr(grad), ptr(dobs),
                                                     7, -1, None) == 0
            assert np.isfinite(q).all()
        packed = int(lib.dtqn_debug_last_packed_blocks())
    launches = []
    for line in err[0].splitlines():
        if line.startswith("tl_launch"):
            m = LINE.match(line)
            assert m, line
            launches.append([m.group(1), [int(m.group(2)), int(m.group(3)), int(m.group(4))], int(m.group(5)), int(m.group(6))])
    return {"launches": launches, "packed_blocks": packed if any(k[0] == "tl_layer_kernel" for k in launches) else None}


@pytest.fixture(scope="module")
def emu():
    from dtqn_amd import _binding as B
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.parametrize("name,net,what,env", CASES, ids=[c[0] for c in CASES])
def test_launch_sequence_is_the_recorded_one(emu, golden, name, net, what, env):
    got, want = run_case(emu, net, what, env), golden[name]
    assert [k[0] for k in got["launches"]] == [k[0] for k in want["launches"]]
    assert got["launches"] == want["launches"]
    assert got["packed_blocks"] == want["packed_blocks"]
    assert bool(got["launches"]) == (env.get("DTQN_TL_TRACE", "1") == "1")


def test_recording_covers_the_branches(golden):
    """The recording itself: the cases reach the branches they are named after (a recorder run on the wrong shapes would pin nothing)."""
    names = {c: [k[0] for k in golden[c]["launches"]] for c in golden}
    assert set(names) == {c[0] for c in CASES}
    assert "tl_layer_kernel" in names["d128-rows64"] and "tl_chain_bwd_kernel" in names["d128-rows64"]
    assert "tl_layer_kernel" not in names["d128-rows64-layer_fuse0"] and "tl_ffn_kernel" in names["d128-rows64-layer_fuse0"]
    assert names["d128-rows64-qkv_fuse0"].count("tl_wide_kernel") == 2 * names["d128-rows64"].count("tl_wide_kernel") > 0
    assert "tl_head_bwd_kernel" in names["d128-rows64-head_fuse0"] and "tl_head_bwd_kernel" not in names["d128-rows64"]
    assert "tl_chain_bwd_kernel" not in names["d128-rows64-bwd_chain0"] and "tl_ffn_bwd_kernel" in names["d128-rows64-bwd_chain0"]
    assert "tl_ffn_bwd_kernel" not in names["d128-rows64-ffn_bwd0"] and "tl_chain_bwd_kernel" not in names["d128-rows64-ffn_bwd0"]
    assert "tl_wide_kernel" not in names["d128-no_wide"] and "tl_linear_kernel" in names["d128-no_wide"]
    assert "tl_attn_kb_kernel" in names["d128-attn_kblock"] and "tl_attn_kb_dq_kernel" in names["d128-attn_kblock"]
    assert golden["d128-gemm_rows32"]["launches"] != golden["d128-defaults"]["launches"]
    assert golden["d128-rows64"]["launches"] != golden["d128-defaults"]["launches"]
    assert golden["d128-skew_ticks"] == golden["d128-rows64"] == golden["d128-skew_wide_layer"]
    assert names["d128-inference-untraced"] == [] and "tl_layer_kernel" in names["d128-inference"]
    assert "tl_dq_in_kernel" in names["d128-autograd"]
    for t in ("0", "1"):
        assert ("tl_embed_table_kernel" in names[f"discrete-table{t}-qkv1"]) == (t == "1")
    assert "tl_wide_kernel" in names["discrete-table1-qkv0"] and "tl_wide_kernel" not in names["discrete-table1-qkv1"]
    assert "tl_embed_kernel" in names["discrete-wpack0"]
    assert "tl_gate_bwd_kernel" in names["d64-gru"] and "tl_layernorm_kernel" in names["d64-identity"] and "tl_layernorm_kernel" in names["d48-padded"]
    assert "tl_chain_bwd_kernel" in names["d256-chain1"] and "tl_chain_bwd_kernel" not in names["d256-chain0"]
    assert "tl_bag_attn_kernel" in names["bag-mfma0"] and "tl_bag_attn_mfma_kernel" in names["bag-mfma1"]
    assert "tl_drop_rows_kernel" in names["dropout"]
    nets = NETS["d128_ctx48"]
    lp, batch, ctx = 64, nets[1]["batch"], nets[0]["history_len"]
    assert golden["ctx48-pack0"]["packed_blocks"] == 0 and golden["ctx48-pack1"]["packed_blocks"] == batch * (lp // 64) + 2 * batch * ctx // 64


def test_every_switch_has_a_case():
    """The header's table and this file's list name the same switches, and every one of them is set in a case and unset in another."""
    with open(SWITCH_HEADER) as f:
        in_header = set(re.findall(r'"(DTQN_[A-Z0-9_]+)"', f.read()))
    assert in_header == set(SWITCHES)
    envs = [{"DTQN_TL_TRACE": "1", **c[3]} for c in CASES]
    for s in SWITCHES:
        assert any(e.get(s) is not None for e in envs), f"{s} is set in no case"
        assert any(e.get(s) is None for e in envs), f"{s} is unset in no case"


if __name__ == "__main__":
    # recording mode: run from the tree whose launch sequences are to be pinned, with the tests directory of that tree
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_tl_launch_plan.py --record PATH"
    sys.path[:0] = [REPO, HERE]
    from dtqn_amd import _binding
    from emu import emu_build
    lib_ = _binding.load_library(emu_build.build())
    rec = {}
    for name_, net_, what_, env_ in CASES:
        rec[name_] = run_case(lib_, net_, what_, env_)
        print(name_, len(rec[name_]["launches"]), rec[name_]["packed_blocks"], flush=True)
    with open(sys.argv[2], "w") as f_:
        json.dump(rec, f_, indent=0, sort_keys=True)
        f_.write("\n")
