"""Per-stage wall-clock breakdown of the first and the last workgroup of dtqn_clip_adam_kernel (debug aid; the companion of
stage_profile_wgrad.py, same profile buffer: the kernel's marks sit in slots 22 .. 28 of each workgroup's forward half, which the
forward and the weight-gradient kernels leave alone).  The first workgroup is an Adam block, the last one carries the statistics and
the host ring and sets the kernel's length.  Every sample is the last of `chain` updates issued back to back, so the kernel starts
behind the weight gradients with cold caches as it does in training (chain 1: behind a drained stream).
Needs a library built with the stage clocks: DTQN_BUILD_PROF=1 python -m dtqn_amd.build (the product build has none).
usage: stage_profile_adam.py [batch] [context] [chain]"""
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
CHAIN = int(sys.argv[3]) if len(sys.argv) > 3 else 4
cfg = O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=L)
net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=1, batch=Bn, T=200, n_eps=300, mask=-5, device="cuda", test_lib=False)
eps, starts = host.sample_indices(Bn); eng.set_indices(eps, starts)
prof = torch.zeros(128, dtype=torch.int64, device="cuda")
lib.dtqn_debug_set_profile_buffer(ctypes.c_void_p(prof.data_ptr()))
for _ in range(5):
    eng.forward_backward(rep); eng.clip_adam()
torch.cuda.synchronize()
N, FIRST, MARKS = 40, 22, 7
labels = ["kernel entry", "all loads issued", "why / k known", "norm known", "Adam stores issued", "statistics reduced", "ring written"]
have = [[0, 1, 2, 3, 4], [0, 1, 2, 3, 5, 6]]                    # the marks each of the two workgroups carries
acc = np.zeros((2, MARKS)); skew = 0.0; seen = 0
for _ in range(N):
    prof.zero_()
    for _ in range(CHAIN):
        eng.forward_backward(rep); eng.clip_adam()
    torch.cuda.synchronize()
    p = prof.cpu().numpy().astype(np.float64)
    segs = [p[base + FIRST:base + FIRST + MARKS] for base in (0, 32)]
    if any((s[h] <= 0).any() for s, h in zip(segs, have)):
        continue
    seen += 1
    skew += (segs[1][0] - segs[0][0]) / 100.0
    for w, s in enumerate(segs):
        acc[w] += (s - s[0]) / 100.0                          # 100 MHz -> us since the workgroup's entry
lib.dtqn_debug_set_profile_buffer(None)
if seen == 0:
    raise SystemExit("no marks: the library was built without the stage clocks")
acc /= seen
print(f"== dtqn_clip_adam_kernel (B={Bn}, L={L}, n={net.n_trainable}, {eng.n_norm_blocks + 1} workgroups, chain {CHAIN}; first | last workgroup; "
      f"mean of {seen}; us since the workgroup's entry, and since its mark before; marks in the order the last workgroup passes them)")
print(f"  (the last workgroup enters {skew / seen:+.2f} us after the first)")
order = sorted(range(MARKS), key=lambda i: (acc[1, i] if i in have[1] else acc[0, i], i))
prev = [0.0, 0.0]
for i in order:
    cells = []
    for w in (0, 1):
        if i in have[w]:
            cells.append(f"{acc[w, i]:7.2f} ({acc[w, i] - prev[w]:+6.2f})"); prev[w] = acc[w, i]
        else:
            cells.append(f"{'-':>7s} {'':8s}")
    print(f"  {labels[i]:22s} {cells[0]}   {cells[1]}")
