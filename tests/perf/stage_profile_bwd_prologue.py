"""Deferred stage marks of the backward launch's prologue (loss, Q head, top of the first layer) in the launch the benchmark runs:
dtqn_td_backward_ahead behind a pipelined forward (debug aid; the sibling of stage_profile.py, which profiles the staged launch).

    python tests/perf/stage_profile_bwd_prologue.py [batch] [updates]

Needs a library built with the stage clocks, the second profiled workgroup being the LOWEST slice of sequence 0 (workgroup 0 is its
uppermost slice; at batch >= 8 the slices of a sequence are blocks 0, 8, 16, 24: slice_block_map):
    python tools/build_variant.py <tag> -DDTQN_ENABLE_PROF -DDTQN_PROF_WG1=24,  DTQN_HIP_LIB=tools/variants/libdtqn_hip_<tag>.so
The prologue's marks are read into scalar registers and stored at the end of the kernel (dtqn_backward.hip), so no mark puts a store
or a wait between the prologue's loads and their use.  Times are the MEDIAN over the updates, in us since the kernel's first mark."""
import ctypes, sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from oracle import dtqn_oracle as O
from helpers import make_td_case
from dtqn_amd import engine
lib = engine.get_lib(); engine.require_gpu()
Bn = int(sys.argv[1]) if len(sys.argv) > 1 else 32
N = int(sys.argv[2]) if len(sys.argv) > 2 else 200
cfg = O.NetCfg(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50)
net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=1, batch=Bn, T=200, n_eps=300, mask=-5, device="cuda", test_lib=False)
assert eng.row_split == 4 and eng.enable_pipeline(lambda: 0) and eng._pipe["ride"], "not the pipelined four-slice update"
n_valid, exclude = min(host.pos[0], host.max_size), host.pos[0] % host.max_size
prof = torch.zeros(128, dtype=torch.int64, device="cuda")
lib.dtqn_debug_set_profile_buffer(ctypes.c_void_p(prof.data_ptr()))


def update():
    eng.sample_in_forward(n_valid, exclude, 1234)
    eng.update(rep)


for _ in range(20):
    update()
torch.cuda.synchronize()
# (slot, name): the prologue in program order
# (25: written by the parent's prologue only, behind its zero-fill barrier; 16 .. 19 stay empty for stage_profile.py)
MARKS = [(24, "prefetches issued"), (20, "loss loads issued"), (25, "loss wave enters"), (26, "loss wave done"), (27, "barrier"),
         (1, "LOSS DONE (dq record stores issued)"), (21, "head: elementwise pass done (head.2 operands used)"), (2, "HEAD DONE"),
         (22, "L_top: dh fragment prefetch issued"), (23, "L_top: LN statistics -> LDS, next layer's in flight"),
         (28, "L_top: before s2 -> LDS"), (29, "s2 in LDS"), (30, "barrier"), (31, "LN2 backward body"), (3, "LN2 BWD DONE (top layer)")]
STAGES = ["FFNb", "LN1b", "dO", "attnb", "dqkvWin"]
rows = {0: [], 1: []}
for _ in range(N):
    prof.zero_(); update(); torch.cuda.synchronize()
    p = prof.cpu().numpy().astype(np.float64)
    for half in (0, 1):
        q = p[64 + 32 * half:96 + 32 * half]
        if q[0] > 0:
            rows[half].append(np.where(q > 0, (q - q[0]) / 100.0, np.nan))      # 100 MHz -> us
assert rows[0] and rows[1], "no marks: is this a -DDTQN_ENABLE_PROF build?"
import warnings
with warnings.catch_warnings():
    warnings.simplefilter("ignore", RuntimeWarning)           # (a slot no mark writes is NaN throughout)
    med = [np.nanmedian(np.array(rows[h]), axis=0) for h in (0, 1)]
print(f"== backward prologue, dtqn_td_backward_ahead behind the pipelined forward (B={Bn}, median of {N} updates, pass ahead used {eng._pipe['used']} times)")
print("   us since the kernel's first mark; workgroup 0 (uppermost slice of sequence 0) | workgroup DTQN_PROF_WG1 (its lowest slice)")
for slot, name in MARKS:
    print(f"  {name:52s} {med[0][slot]:8.2f}   {med[1][slot]:8.2f}")
print("   the steady stages behind it (us each; immediate-store marks as in stage_profile.py)")
for l, base in ((1, 3), (0, 8)):
    for i, s in enumerate(STAGES if l == 1 else ["LN2b"] + STAGES):
        a, b = base + i, base + i + 1
        print(f"  L{l}:{s:10s} {med[0][b] - med[0][a]:8.2f}   {med[1][b] - med[1][a]:8.2f}")
last = 15
print(f"  {'last mark (embedding stage starts)':52s} {med[0][last]:8.2f}   {med[1][last]:8.2f}")
lib.dtqn_debug_set_profile_buffer(None)
