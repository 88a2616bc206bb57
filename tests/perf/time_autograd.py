"""Wall-clock of one policy forward + backward through torch autograd (DTQN(..., autograd=True): dtqn_forward_train + dtqn_backward_dq,
loss = (Q * w).sum()) against one fused TD update (three forwards, loss, backward, weight gradients, clip + Adam: dtqn_td_update) at
BASELINE config 1 / 3 / 4 / 5 shapes and batches.  Prints one line per config and writes the numbers as JSON to the path given as the
first argument (default bench_out/time_autograd.json)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from autograd_helpers import make_inputs, make_module  # noqa: E402
from dtqn_amd import engine  # noqa: E402
from helpers import make_td_case  # noqa: E402
from oracle import dtqn_oracle as O  # noqa: E402

lib = engine.get_lib()
engine.require_gpu()
torch.cuda.set_device(0)
SHAPES = {
    "cfg1": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50), 32),
    "cfg3": (dict(obs_dim=10, num_actions=10, inner_embed_size=128, num_heads=8, num_layers=2, history_len=50, discrete=True, vocab_sizes=9), 512),
    "cfg4": (dict(obs_dim=6, num_actions=6, inner_embed_size=128, num_heads=8, num_layers=2, history_len=128, discrete=True, vocab_sizes=12), 128),
    "cfg5": (dict(obs_dim=1, num_actions=5, inner_embed_size=256, num_heads=8, num_layers=2, history_len=256, discrete=True, vocab_sizes=22), 32),
}
WARM, ITERS = 3, 20


def timed(fn):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS


res = {}
for tag, (kw, Bn) in SHAPES.items():
    cfg = O.NetCfg(**kw)
    L = cfg.history_len
    params = O.init_params(cfg, seed=1)
    m = make_module(None, cfg, params, device="cuda")
    obs, act, _, w = make_inputs(cfg, Bn, L, seed=2)
    o, a, wt = torch.as_tensor(obs, device="cuda"), torch.as_tensor(act, device="cuda"), torch.as_tensor(w, device="cuda")

    def step():
        m.zero_grad(set_to_none=True)
        (m(o, a) * wt).sum().backward()

    def fwd_nograd():
        with torch.no_grad():
            m(o, a)

    ag = timed(step)
    nf = timed(fwd_nograd)
    del m
    net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=1, batch=Bn, T=L + 40, n_eps=64, mask=(kw["vocab_sizes"] - 1) if cfg.discrete else -5,
                                               device="cuda", test_lib=False)
    eps, starts = host.sample_indices(Bn)
    eng.set_indices(eps, starts)
    n_, r_, t_, s_ = ctypes.byref(eng.net), ctypes.byref(rep.view), ctypes.byref(eng.td), eng._stream()
    td = timed(lambda: lib.dtqn_td_update(n_, r_, t_, s_))
    res[tag] = dict(batch=Bn, autograd_fwd_bwd_us=round(ag, 1), nograd_forward_us=round(nf, 1), fused_td_update_us=round(td, 1),
                    ratio=round(ag / td, 3))
    print(f"{tag} B={Bn}: autograd forward+backward {ag:.1f} us | no-grad forward {nf:.1f} us | fused TD update {td:.1f} us | "
          f"ratio {ag / td:.2f}", flush=True)
    del eng, rep
    torch.cuda.empty_cache()
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join("bench_out", "time_autograd.json")
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
