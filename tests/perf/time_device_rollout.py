"""Device-resident rollout (`run.py --device-envs N`, DeviceVectorActor) against the host vector actor (`--num-envs N`, VectorActor) on the
config-1 network (d_model 64, 8 heads, 2 layers, context 50, batch 32) with DiscreteCarFlag-v0:

  actor    env-steps/s of the actor alone at N = 8 and 32 (epsilon 0.1: every vector step runs the forward), no updates queued;
  coupled  TD-updates/s through run.train -- the loop run.py runs -- at 1 env step : 1 update with N = 32: N updates queued behind
           every vector step.  A commit in front of an update costs the target pass launched ahead; `ahead_used` in the result counts
           the passes that were used (the device path bumps the replay version only with the launches it authorises to commit).

Protocol: a host clock around work that ends in a device synchronise; one untimed warm-up window, then windows of at least `--seconds`
(default 1.0); device and host alternate `--repeats` times (default 3) inside this one command.  One JSON line per window, then one
summary line per (mode, N, path) with the median and the spread (min .. max) over the repeats.

  python tests/perf/time_device_rollout.py
  python tests/perf/time_device_rollout.py --mode actor --envs 32 --repeats 3"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

ENV_ID = "DiscreteCarFlag-v0"


def make_agent(device, seed):
    from dtqn_amd import envs
    from dtqn_amd.utils import agent_utils
    from dtqn_amd.utils.random import set_global_seed
    env = envs.make(ENV_ID)
    set_global_seed(seed, env)
    agent = agent_utils.get_agent("DTQN", [env], 8, 0, 64, 100_000, device, 3e-4, 32, 50, -1, 50, 10_000, 0.99, 8, 2, 0.0, False, "res",
                                  "learned", 0, sampler="device", sample_seed=seed)
    return agent, env


def make_path(path, n, device, prepopulate):
    """-> (agent, vector actor, the environments run.train wants)."""
    import run as runpy
    from dtqn_amd import envs
    agent, env = make_agent(device, 1)
    if path == "device":
        from dtqn_amd.agents.device_rollout import DeviceVectorActor
        vec = DeviceVectorActor(agent, ENV_ID, n, 1001)
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


def actor_window(vec, seconds, chunk=64):
    """Vector steps until `seconds` have passed, then a synchronise -> env-steps/s."""
    torch.cuda.synchronize()
    t0, steps = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
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
    pipe = getattr(agent.engine, "_pipe", None)
    used0 = pipe.get("used", 0) if pipe else 0
    torch.cuda.synchronize()
    t0, s0 = time.perf_counter(), agent.num_train_steps
    runpy.train(agent, envs_, envs_, [ENV_ID], s0 + updates, eps, 10 ** 9, 0, "", False, _NoLog(), None, None, None, None, vector=vec)
    if hasattr(vec, "sync"):
        vec.sync()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return (agent.num_train_steps - s0) / dt, (pipe.get("used", 0) - used0) if pipe else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", nargs="+", default=["actor", "coupled"], choices=["actor", "coupled"])
    ap.add_argument("--envs", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--coupled-envs", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--updates", type=int, default=16384, help="updates per coupled window (at least a second at 11 k updates/s)")
    a = ap.parse_args()
    device = torch.device("cuda:0")
    summary = []
    if "actor" in a.mode:
        for n in a.envs:
            paths = {p: make_path(p, n, device, 0) for p in ("device", "host")}
            rates = {p: [] for p in paths}
            for p in paths:
                actor_window(paths[p][1], 0.3)                   # warm-up
            for r in range(a.repeats):
                for p in ("device", "host"):
                    rate = actor_window(paths[p][1], a.seconds)
                    rates[p].append(rate)
                    print(json.dumps(dict(mode="actor", envs=n, path=p, repeat=r, env_steps_per_s=round(rate, 1))), flush=True)
            for p in ("device", "host"):
                summary.append(dict(mode="actor", envs=n, path=p, unit="env-steps/s", median=round(float(np.median(rates[p])), 1),
                                    min=round(min(rates[p]), 1), max=round(max(rates[p]), 1)))
            del paths
            torch.cuda.empty_cache()
    if "coupled" in a.mode:
        n = a.coupled_envs
        paths = {p: make_path(p, n, device, 5000) for p in ("device", "host")}
        rates, ahead = {p: [] for p in paths}, {p: [] for p in paths}
        for p in paths:
            coupled_window(*paths[p], 2048)                       # warm-up
        for r in range(a.repeats):
            for p in ("device", "host"):
                rate, used = coupled_window(*paths[p], a.updates)
                rates[p].append(rate)
                ahead[p].append(used)
                print(json.dumps(dict(mode="coupled", envs=n, path=p, repeat=r, updates_per_s=round(rate, 1), updates=a.updates, ahead_used=used)),
                      flush=True)
        for p in ("device", "host"):
            summary.append(dict(mode="coupled", envs=n, path=p, unit="updates/s", median=round(float(np.median(rates[p])), 1),
                                min=round(min(rates[p]), 1), max=round(max(rates[p]), 1), ahead_used=ahead[p]))
    for s in summary:
        print(json.dumps(dict(summary=s)), flush=True)


if __name__ == "__main__":
    main()
