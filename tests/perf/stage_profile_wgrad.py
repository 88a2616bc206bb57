"""Per-stage wall-clock breakdown of workgroups 0 / 1 of dtqn_wgrad_direct_kernel (debug aid; the companion of stage_profile.py, same
profile buffer: the kernel's marks sit in slots 16 .. 21 of each workgroup's forward half, which the forward kernel leaves alone).
Needs a library built with the stage clocks: DTQN_BUILD_PROF=1 python -m dtqn_amd.build (the product build has none).
usage: stage_profile_wgrad.py [batch] [context]"""
import ctypes, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from oracle import dtqn_oracle as O
from helpers import make_td_case
from dtqn_amd import engine
lib = engine.get_lib(); engine.require_gpu()
Bn = int(sys.argv[1]) if len(sys.argv) > 1 else 32
L = int(sys.argv[2]) if len(sys.argv) > 2 else 50
cfg = O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=L)
net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=1, batch=Bn, T=200, n_eps=300, mask=-5, device="cuda", test_lib=False)
eps, starts = host.sample_indices(Bn); eng.set_indices(eps, starts)
prof = torch.zeros(128, dtype=torch.int64, device="cuda")
lib.dtqn_debug_set_profile_buffer(ctypes.c_void_p(prof.data_ptr()))
for _ in range(5): eng.forward_backward(rep)
torch.cuda.synchronize()
N, FIRST, MARKS = 40, 16, 6
acc = np.zeros((2, MARKS)); seen = 0
for _ in range(N):
    prof.zero_(); eng.forward_backward(rep); torch.cuda.synchronize()
    p = prof.cpu().numpy().astype(np.float64)
    segs = [p[base + FIRST:base + FIRST + MARKS] for base in (0, 32)]
    if any((s <= 0).any() for s in segs):
        continue
    seen += 1
    for w, s in enumerate(segs):
        acc[w] += (s - s[0]) / 100.0                          # 100 MHz -> us since kernel entry
lib.dtqn_debug_set_profile_buffer(None)
if seen == 0:
    raise SystemExit("no marks: the library was built without the stage clocks")
acc /= seen
labels = ["kernel entry", "tile and job known", "all loads issued", "last MFMA done", "slabs reduced, grad stored", "norm partial stored"]
print(f"== dtqn_wgrad_direct_kernel (B={Bn}, L={L}, lp={net.lp}; workgroups 0 | 1; mean of {seen}; us since entry, and since the mark before)")
for i, lab in enumerate(labels):
    d = acc[:, i] - (acc[:, i - 1] if i else 0.0)
    print(f"  {lab:28s} {acc[0, i]:7.2f} ({d[0]:+6.2f})   {acc[1, i]:7.2f} ({d[1]:+6.2f})")
