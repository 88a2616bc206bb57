"""TD-updates/s of agent.train() on wide discrete observations (the panel embedding-gradient kernel, tl_embed_bwd_panel_kernel) next to a
continuous network of equal obs_dim as the yardstick for what the embedding gradient costs, after the warm-up protocol of
tests/perf/time_agent_cfg.py (10 updates, synchronise, wall clock over `steps`).

  python tests/perf/time_wide_discrete.py                    # 49 tokens x vocabulary 20, x vocabulary 6000, and 49 floats: d_model 128, context 128, batch 32
  python tests/perf/time_wide_discrete.py --vocab 6000 --steps 30        # one case (--vocab 0: the continuous network)
  python tests/perf/time_wide_discrete.py --kernel-stats OUT # per-kernel times: for each case one fresh child under
        timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d OUT/vocab<V> -o run -- \
            python tests/perf/time_wide_discrete.py --vocab <V> --steps 30
    and from its *kernel_stats.csv the rows of the embedding kernels (calls, average and total ns); stops at the first child that fails.

Each result is one JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import bench

TOKENS, CTX, D_MODEL, HEADS = 49, 128, 128, 8
VOCABS = (20, 6000, 0)


def make_agent(vocab, batch, device, seed=1):
    from dtqn_amd.agents.dtqn import DtqnAgent
    from dtqn_amd.networks.dtqn import DTQN
    import dtqn_amd.utils.random as rnd
    disc = vocab > 0
    c = dict(kind="multidiscrete" if disc else "box", O=TOKENS, A=4, T=CTX + 72, L=CTX, nvec=max(1, vocab - 1))
    torch.manual_seed(seed)
    rnd.RNG.rng = np.random.Generator(np.random.PCG64(seed))
    factory = lambda: DTQN(TOKENS, c["A"], 8, 0, D_MODEL, HEADS, 2, CTX, discrete=disc, vocab_sizes=vocab if disc else None).to(device)
    agent = DtqnAgent(factory, buffer_size=256 * c["T"], device=device, env_obs_length=TOKENS, max_env_steps=c["T"],
                      obs_mask=vocab - 1 if disc else -5, num_actions=c["A"], is_discrete_env=disc, batch_size=batch, context_len=CTX,
                      history=CTX, target_update_frequency=10_000, sampler="device", sample_seed=seed)
    bench.fill_synthetic_replay(agent, seed=seed, c=c)
    return agent


def run(vocab, batch, steps, device):
    agent = make_agent(vocab, batch, device)
    for _ in range(10): agent.train()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps): agent.train()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    st = agent.engine.read_stats()
    print(json.dumps(dict(d_model=D_MODEL, heads=HEADS, ctx=CTX, tokens=TOKENS, vocab=vocab, batch=batch, steps=steps,
                          updates_per_s=round(1 / dt, 1), us_per_update=round(dt * 1e6, 1), nonfinite=st["nonfinite"])), flush=True)
    del agent
    torch.cuda.empty_cache()


def kernel_stats(out_dir, batch):
    """One rocprofv3 --kernel-trace --stats child per case; nothing of the GPU is touched in this process."""
    import csv, glob, subprocess
    for vocab in VOCABS:
        d = os.path.join(out_dir, f"vocab{vocab}")
        cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--",
               sys.executable, os.path.abspath(__file__), "--vocab", str(vocab), "--batch", str(batch), "--steps", "30"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            sys.exit(r.returncode)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        with open(files[0]) as f:
            all_rows = list(csv.DictReader(f))
        total = sum(float(x["TotalDurationNs"]) for x in all_rows)
        rows = []
        for x in all_rows:
            if "tl_embed" in x["Name"]:
                name = x["Name"].split("(")[0].replace("void dtqn::", "")
                rows.append(dict(kernel=name, calls=int(x["Calls"]), avg_us=round(float(x["AverageNs"]) / 1e3, 2),
                                 total_us=round(float(x["TotalDurationNs"]) / 1e3, 1),
                                 share=round(float(x["TotalDurationNs"]) / total, 4)))
        print(json.dumps(dict(ctx=CTX, tokens=TOKENS, vocab=vocab, batch=batch, all_kernels_total_us=round(total / 1e3, 1), embedding=rows)), flush=True)
        for t in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            os.remove(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-stats", metavar="OUT")
    ap.add_argument("--vocab", type=int)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.batch)
    device = torch.device("cuda:0")
    for vocab in (VOCABS if a.vocab is None else (a.vocab,)):
        run(vocab, a.batch, a.steps, device)


if __name__ == "__main__":
    main()
