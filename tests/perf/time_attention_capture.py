"""Wall-clock of attention capture (DTQN(..., capture_attention=True)): the capturing no-grad forward (dtqn_forward_train into the
module's record workspace + dtqn_attn_weights) against the plain no-grad forward, and tl_alpha_kernel alone (dtqn_attn_weights on the
kept records) per layer, at BASELINE config 1 and config 5 shapes (L = 256 and 512), batch 32.  Prints one line per shape and writes the
numbers as JSON to the path given as the first argument (default bench_out/time_attention_capture.json)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from autograd_helpers import make_inputs, make_module  # noqa: E402
from dtqn_amd import engine  # noqa: E402
from oracle import dtqn_oracle as O  # noqa: E402

lib = engine.get_lib()
engine.require_gpu()
torch.cuda.set_device(0)
CFG5 = dict(obs_dim=1, num_actions=5, inner_embed_size=256, num_heads=8, num_layers=2, history_len=256, discrete=True, vocab_sizes=22)
SHAPES = {
    "cfg1": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50), 32),
    "cfg5_L256": (CFG5, 32),
    "cfg5_L512": (dict(CFG5, history_len=512), 32),
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
    m = make_module(None, cfg, O.init_params(cfg, seed=1), device="cuda", autograd=False).eval()
    obs, act, _, _ = make_inputs(cfg, Bn, L, seed=2)
    o, a = torch.as_tensor(obs, device="cuda"), torch.as_tensor(act, device="cuda")

    def fwd():
        with torch.no_grad():
            m(o, a)

    m.set_capture_attention(False)
    plain = timed(fwd)
    m.set_capture_attention(True)
    cap = timed(fwd)
    # the alpha kernel alone, on the records the last capturing forward kept
    net, ws = m._grad_net(), m._capture_ws
    alpha = torch.empty((cfg.num_layers, Bn, L, L), dtype=torch.float32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (ctypes.byref(net), ctypes.c_void_p(ws.data_ptr()), Bn, L, ctypes.c_void_p(alpha.data_ptr()), None, stream)
    assert lib.dtqn_attn_weights(*args) == 0
    kern = timed(lambda: lib.dtqn_attn_weights(*args)) / cfg.num_layers
    res[tag] = dict(batch=Bn, L=L, plain_forward_us=round(plain, 1), capturing_forward_us=round(cap, 1), ratio=round(cap / plain, 3),
                    alpha_kernel_us_per_layer=round(kern, 1), alpha_mb_per_layer=round(Bn * L * L * 4 / 1e6, 2))
    print(f"{tag} B={Bn} L={L}: plain forward {plain:.1f} us | capturing forward {cap:.1f} us (x{cap / plain:.2f}) | "
          f"tl_alpha_kernel {kern:.1f} us per layer", flush=True)
    del m, alpha
    torch.cuda.empty_cache()
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join("bench_out", "time_attention_capture.json")
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
