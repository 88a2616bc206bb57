"""Device-resident rollout of a tabular POMDP (`run.py --envs POMDP-corridor-episodic-v0 --device-envs N`) against the host vector actor
(`--num-envs N`) and against CarFlag on the same build, with the protocol and the window functions of time_device_rollout.py (config-1
network: d_model 64, 8 heads, 2 layers, context 50, batch 32):

  actor    env-steps/s of the actor alone at N = 8 and 32 (epsilon 0.1), device and host alternating, for the corridor;
  coupled  TD-updates/s through run.train at 1 env step : 1 update with N = 32: the corridor on the device path, the corridor on the
           host path and CarFlag on the device path, alternating;
  step     microseconds per step-kernel launch at N = 32 with epsilon = 1 (no forward is launched: the stream holds step kernels
           only), corridor and CarFlag alternating, device events around 2048 launches.

One JSON line per window, then one summary line per figure with the median and the spread (min .. max) over the repeats.

  python tests/perf/time_pomdp_rollout.py"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

import time_device_rollout as T

POMDP, CARFLAG = "POMDP-corridor-episodic-v0", "DiscreteCarFlag-v0"


def make_path(env_id, path, n, device, prepopulate):
    T.ENV_ID = env_id                                    # time_device_rollout.make_path builds its agent and environments from this id
    return T.make_path(path, n, device, prepopulate)


def coupled_window(env_id, agent, vec, envs_, updates):
    T.ENV_ID = env_id
    return T.coupled_window(agent, vec, envs_, updates)


def step_window(vec, launches=2048):
    """`launches` vector steps with epsilon = 1 (step kernel only) between two device events -> microseconds per launch."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = vec.agent._main_stream
    torch.cuda.synchronize()
    start.record(stream)
    for _ in range(launches):
        vec.step_all(1.0, store=False)
    end.record(stream)
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1000.0 / launches


def summarise(summary, rates, **tags):
    for key, vals in rates.items():
        summary.append(dict(tags, path=key, median=round(float(np.median(vals)), 2), min=round(min(vals), 2), max=round(max(vals), 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", nargs="+", default=["actor", "coupled", "step"], choices=["actor", "coupled", "step"])
    ap.add_argument("--envs", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--updates", type=int, default=16384)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    summary = []
    if "actor" in a.mode:
        for n in a.envs:
            paths = {p: make_path(POMDP, p, n, device, 0) for p in ("device", "host")}
            rates = {p: [] for p in paths}
            for p in paths:
                T.actor_window(paths[p][1], 0.3)                  # warm-up
            for r in range(a.repeats):
                for p in ("device", "host"):
                    rate = T.actor_window(paths[p][1], a.seconds)
                    rates[p].append(rate)
                    print(json.dumps(dict(mode="actor", env=POMDP, envs=n, path=p, repeat=r, env_steps_per_s=round(rate, 1))), flush=True)
            summarise(summary, rates, mode="actor", env=POMDP, envs=n, unit="env-steps/s")
            del paths
            torch.cuda.empty_cache()
    if "coupled" in a.mode:
        cases = {f"{POMDP} device": (POMDP, "device"), f"{POMDP} host": (POMDP, "host"), f"{CARFLAG} device": (CARFLAG, "device")}
        paths = {k: make_path(e, p, 32, device, 5000) for k, (e, p) in cases.items()}
        rates = {k: [] for k in paths}
        for k in paths:
            coupled_window(cases[k][0], *paths[k], 2048)          # warm-up
        for r in range(a.repeats):
            for k in paths:
                rate, used = coupled_window(cases[k][0], *paths[k], a.updates)
                rates[k].append(rate)
                print(json.dumps(dict(mode="coupled", case=k, envs=32, repeat=r, updates_per_s=round(rate, 1), ahead_used=used)), flush=True)
        summarise(summary, rates, mode="coupled", envs=32, unit="updates/s")
        del paths
        torch.cuda.empty_cache()
    if "step" in a.mode:
        paths = {e: make_path(e, "device", 32, device, 0) for e in (POMDP, CARFLAG)}
        rates = {e: [] for e in paths}
        for e in paths:
            step_window(paths[e][1], 256)                         # warm-up
        for r in range(a.repeats):
            for e in paths:
                us = step_window(paths[e][1])
                rates[e].append(us)
                print(json.dumps(dict(mode="step", env=e, envs=32, repeat=r, us_per_step_kernel=round(us, 2))), flush=True)
        summarise(summary, rates, mode="step", envs=32, unit="us per step-kernel launch")
    for s in summary:
        print(json.dumps(dict(summary=s)), flush=True)


if __name__ == "__main__":
    main()
