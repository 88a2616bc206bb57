"""TD-updates/s of agent.train() at BASELINE config 5 shapes (d_model 256, 8 heads of 32, 2 layers, batch 32) at long contexts: L = 256 on
the whole-tile attention kernels, L = 256 with DTQN_ATTN_KBLOCK=1 (the key-blocked kernels forced), L = 384 and L = 512 (key-blocked by
necessity).  Rates over a window of at least `--window` seconds after warm-up; one JSON line per case.
    python tests/perf/time_long_context.py [--window 1.5] [--cases 256,256kb,384,512]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

import bench

argv = sys.argv[1:]
window = float(argv[argv.index("--window") + 1]) if "--window" in argv else 1.5
cases = (argv[argv.index("--cases") + 1] if "--cases" in argv else "256,256kb,384,512").split(",")
device = torch.device("cuda:0")
for case in cases:
    L = int(case.rstrip("kb"))
    os.environ["DTQN_ATTN_KBLOCK"] = "1" if case.endswith("kb") else "0"     # read per launch by the engine
    c = dict(bench.CONFIGS[5], L=L, T=max(bench.CONFIGS[5]["T"], L))
    agent = bench.make_agent(c, c["B"], device, 0, "device")
    for _ in range(10):
        agent.train()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(10):
            agent.train()
        n += 10
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= window:
            break
    agent._drain_stats(block=True)
    print(json.dumps({"case": case, "L": L, "D": c["D"], "H": c["H"], "B": c["B"], "kblock_forced": case.endswith("kb"),
                      "updates": n, "seconds": round(dt, 3), "updates_per_s": round(n / dt, 2)}), flush=True)
    del agent
    torch.cuda.empty_cache()
os.environ.pop("DTQN_ATTN_KBLOCK", None)
