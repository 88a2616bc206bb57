"""Device-resident rollout of a bag network (`run.py --bag-size K --device-envs N`, DeviceBagVectorActor) against the host vector actor
with the same bag (`--num-envs N`, VectorActor: one module forward per environment to act, and one over K + 1 candidate bags with a
blocking read per environment once context and bag are full) on the config-1 network (d_model 64, 8 heads, 2 layers, context 50,
batch 32) with `--bag-size 5` and DiscreteCarFlag-v0:

  actor    env-steps/s of the actor alone at N = 8 and 32 (epsilon 0.1: every vector step runs the forward), no updates queued;
  coupled  TD-updates/s through run.train -- the loop run.py runs -- at 1 env step : 1 update: N updates queued behind every vector step.

Protocol: a host clock around work that ends in a device synchronise; one untimed warm-up window that reaches the choosing phase (more
than L + K vector steps), then windows of at least `--seconds` (default 1.0); device and host alternate `--repeats` times (default 3)
inside this one command.  One JSON line per window, then one summary line per (mode, N, path) with the median and the spread
(min .. max) over the repeats; the device lines carry the share of vector steps that launched the candidate forward.

  python tests/perf/time_device_bag.py
  python tests/perf/time_device_bag.py --mode actor --envs 32 --repeats 3"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

ENV_ID, BAG = "DiscreteCarFlag-v0", 5


def make_agent(device, seed):
    from dtqn_amd import envs
    from dtqn_amd.utils import agent_utils
    from dtqn_amd.utils.random import set_global_seed
    env = envs.make(ENV_ID)
    set_global_seed(seed, env)
    agent = agent_utils.get_agent("DTQN", [env], 8, 0, 64, 100_000, device, 3e-4, 32, 50, -1, 50, 10_000, 0.99, 8, 2, 0.0, False, "res",
                                  "learned", BAG, sampler="device", sample_seed=seed)
    return agent, env


def make_path(path, n, device, prepopulate):
    """-> (agent, vector actor, the environments run.train wants)."""
    import run as runpy
    from dtqn_amd import envs
    agent, env = make_agent(device, 1)
    if path == "device":
        from dtqn_amd.agents.device_bag import DeviceBagVectorActor
        vec = DeviceBagVectorActor(agent, ENV_ID, n, 1001)
        if prepopulate:
            vec.prepopulate(prepopulate)
    else:
        from dtqn_amd.agents.vector import VectorActor
        if prepopulate:
            runpy.prepopulate(agent, prepopulate, [env])
        copies = [envs.make(ENV_ID) for _ in range(n)]
        for k, e in enumerate(copies):
            e.seed(1001 + k)
        vec = VectorActor(agent, copies)
    vec.reset_all()
    return agent, vec, [env]


def choice_share(vec, since=(0, 0)):
    """Share of the vector steps since `since` that launched the candidate forward (device path), and the new mark."""
    if not hasattr(vec, "choice_steps"):
        return None, since
    steps, chosen = vec.vector_steps - since[0], vec.choice_steps - since[1]
    return (round(chosen / steps, 4) if steps else None), (vec.vector_steps, vec.choice_steps)


def actor_window(vec, seconds, chunk=16, min_steps=0):
    """Vector steps until `seconds` have passed (and at least min_steps), then a synchronise -> env-steps/s."""
    torch.cuda.synchronize()
    t0, steps = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds or steps < min_steps * vec.n:
        for _ in range(chunk):
            vec.step_all(0.1)
        steps += chunk * vec.n
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


class _NoLog:
    def log(self, *a, **k):
        pass


def coupled_window(agent, vec, envs_, updates):
    """`updates` iterations of run.train (no evaluation episodes, no checkpoint), then a synchronise -> TD-updates/s."""
    import run as runpy
    from dtqn_amd.utils import epsilon_anneal
    eps = epsilon_anneal.LinearAnneal(0.1, 0.1, 1)
    torch.cuda.synchronize()
    t0, s0 = time.perf_counter(), agent.num_train_steps
    runpy.train(agent, envs_, envs_, [ENV_ID], s0 + updates, eps, 10 ** 9, 0, "", False, _NoLog(), None, None, None, None, vector=vec)
    if hasattr(vec, "sync"):
        vec.sync()
    torch.cuda.synchronize()
    return (agent.num_train_steps - s0) / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", nargs="+", default=["actor", "coupled"], choices=["actor", "coupled"])
    ap.add_argument("--envs", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--updates", type=int, default=4096, help="updates per coupled window of the host path (the device path runs four times as many: windows of a second and more)")
    a = ap.parse_args()
    device = torch.device("cuda:0")
    summary = []
    for mode in a.mode:
        for n in a.envs:
            paths = {p: make_path(p, n, device, 5000 if mode == "coupled" else 0) for p in ("device", "host")}
            rates, shares, marks = {p: [] for p in paths}, {p: [] for p in paths}, {p: (0, 0) for p in paths}
            for p in paths:                                      # warm-up: into the choosing phase (context 50 + bag 5 vector steps)
                if mode == "actor":
                    actor_window(paths[p][1], 0.3, min_steps=64)
                else:
                    coupled_window(*paths[p], 64 * n)
                _, marks[p] = choice_share(paths[p][1])
            for r in range(a.repeats):
                for p in ("device", "host"):
                    rate = actor_window(paths[p][1], a.seconds) if mode == "actor" else coupled_window(*paths[p], a.updates * (4 if p == "device" else 1))
                    share, marks[p] = choice_share(paths[p][1], marks[p])
                    rates[p].append(rate)
                    shares[p].append(share)
                    print(json.dumps(dict(mode=mode, envs=n, path=p, repeat=r, rate=round(rate, 1), candidate_forward_share=share)), flush=True)
            for p in ("device", "host"):
                summary.append(dict(mode=mode, envs=n, path=p, unit="env-steps/s" if mode == "actor" else "updates/s",
                                    median=round(float(np.median(rates[p])), 1), min=round(min(rates[p]), 1), max=round(max(rates[p]), 1),
                                    candidate_forward_share=shares[p]))
            del paths
            torch.cuda.empty_cache()
    for s in summary:
        print(json.dumps(dict(summary=s)), flush=True)


if __name__ == "__main__":
    main()
