"""TD-updates/s of agent.train() on bag networks, resident bag attention kernels (DTQN_BAG_ATTN_MFMA=0) against the matrix-core ones (=1),
in one process on one build, after the warm-up protocol of tests/perf/time_agent_cfg.py (10 updates, synchronise, wall clock over `steps`).

  python tests/perf/time_bag.py                      # A/B: d_model 128, 8 heads, context 128, batch 32, bags 8 / 32 / 128
  python tests/perf/time_bag.py --large              # context 256 / bag 160 and context 512 / bag 80: no resident kernel to compare with
  python tests/perf/time_bag.py --ctx 128 --bag 32 --knob 1 --steps 30     # one case
  python tests/perf/time_bag.py --kernel-stats OUT   # per-kernel times: for each (bag, knob) of the A/B one fresh child under
        timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d OUT/bag<N>_knob<K> -o run -- \
            python tests/perf/time_bag.py --ctx 128 --bag <N> --knob <K> --steps 30
    and from its *kernel_stats.csv the rows of the bag attention kernels (calls, average and total ns); stops at the first child that fails.

Each result is one JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench


def make_agent(ctx, bag, batch, device, d_model=128, heads=8, seed=1):
    from dtqn_amd.agents.dtqn import DtqnAgent
    from dtqn_amd.networks.dtqn import DTQN
    import dtqn_amd.utils.random as rnd
    c = dict(kind="box", O=3, A=4, T=ctx + 72, L=ctx)
    torch.manual_seed(seed)
    rnd.RNG.rng = np.random.Generator(np.random.PCG64(seed))
    factory = lambda: DTQN(c["O"], c["A"], 8, 0, d_model, heads, 2, ctx, bag_size=bag).to(device)
    agent = DtqnAgent(factory, buffer_size=256 * c["T"], device=device, env_obs_length=c["O"], max_env_steps=c["T"], obs_mask=-5,
                      num_actions=c["A"], is_discrete_env=False, batch_size=batch, context_len=ctx, history=ctx,
                      target_update_frequency=10_000, bag_size=bag, sampler="device", sample_seed=seed)
    bench.fill_synthetic_replay(agent, seed=seed, c=c)
    return agent


def run(ctx, bag, batch, knob, steps, device, d_model=128, heads=8):
    if knob is None:
        os.environ.pop("DTQN_BAG_ATTN_MFMA", None)
    else:
        os.environ["DTQN_BAG_ATTN_MFMA"] = knob          # read per launch
    agent = make_agent(ctx, bag, batch, device, d_model, heads)
    for _ in range(10): agent.train()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps): agent.train()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    st = agent.engine.read_stats()
    print(json.dumps(dict(d_model=d_model, heads=heads, ctx=ctx, bag=bag, batch=batch, knob=knob, steps=steps, updates_per_s=round(1 / dt, 1),
                          us_per_update=round(dt * 1e6, 1), nonfinite=st["nonfinite"])), flush=True)
    del agent
    torch.cuda.empty_cache()


def kernel_stats(out_dir, batch):
    """One rocprofv3 --kernel-trace --stats child per (bag, knob); nothing of the GPU is touched in this process."""
    import csv, glob, subprocess
    for bag in (8, 32, 128):
        for knob in ("0", "1"):
            d = os.path.join(out_dir, f"bag{bag}_knob{knob}")
            cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
                   sys.executable, os.path.abspath(__file__), "--ctx", "128", "--bag", str(bag), "--batch", str(batch), "--knob", knob,
                   "--steps", "30"]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
                sys.exit(r.returncode)
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            rows = []
            with open(files[0]) as f:
                all_rows = list(csv.DictReader(f))
            total = sum(float(x["TotalDurationNs"]) for x in all_rows)
            for x in all_rows:
                if "bag_attn" in x["Name"]:
                    name = x["Name"].split("(")[0].replace("void dtqn::", "")
                    rows.append(dict(kernel=name, calls=int(x["Calls"]), avg_us=round(float(x["AverageNs"]) / 1e3, 2),
                                     total_us=round(float(x["TotalDurationNs"]) / 1e3, 1)))
            print(json.dumps(dict(ctx=128, bag=bag, batch=batch, knob=knob, all_kernels_total_us=round(total / 1e3, 1), bag_attention=rows)), flush=True)
            for t in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
                os.remove(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-stats", metavar="OUT")
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--ctx", type=int)
    ap.add_argument("--bag", type=int)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--knob", choices=["0", "1"])
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.batch)
    device = torch.device("cuda:0")
    if a.ctx is not None:
        run(a.ctx, a.bag, a.batch, a.knob, a.steps, device)
    elif a.large:
        run(256, 160, a.batch, None, a.steps, device)
        run(512, 80, a.batch, None, a.steps, device)
    else:
        for bag in (8, 32, 128):
            for knob in ("0", "1"):
                run(128, bag, a.batch, knob, a.steps, device)


if __name__ == "__main__":
    main()
