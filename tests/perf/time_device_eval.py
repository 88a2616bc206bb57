"""Device-resident greedy evaluation (`run.py --device-eval-envs N`, DeviceEvaluator) against the two host paths -- run.evaluate
(`--eval-envs 1`) and VectorEvaluator (`--eval-envs N`) -- at
  cfg1   config 1 shapes (d_model 64, 8 heads, 2 layers, context 50) on DiscreteCarFlag-v0,
  cfg3   config 3 shapes (d_model 128, 8 heads, 2 layers, context 50) on Memory-5-v0,
`--episodes` episodes per evaluation (default 10, run.py's --eval-episodes), N = `--envs` (default 10) for the two vector paths.

  eval     one evaluation per path on ONE agent whose parameters stand still.  The three paths play different episodes (the host paths
           draw from the environments' generators, the device path from its counter-based keys), so env-steps/s is the comparable figure.
  coupled  TD-updates/s through run.train -- evaluations included -- with `--device-envs 32 --eval-frequency 5000`, once evaluating
           through run.evaluate (the default) and once through DeviceEvaluator (`--device-eval-envs N`).

Protocol: all paths in this one command; one untimed evaluation (window) each, then the paths alternate `--repeats` times (default 3);
every timed evaluation (window) sits between two device synchronisations.  One JSON line per measurement, then one summary line per
path: median (min .. max) in ms and env-steps/s, or updates/s.

  python tests/perf/time_device_eval.py
  python tests/perf/time_device_eval.py --mode eval --config cfg1 --repeats 3"""
import argparse, json, os, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import numpy as np
import torch

from time_eval import Seeded, make

ENV_IDS = {"cfg1": "DiscreteCarFlag-v0", "cfg3": "Memory-5-v0"}


def eval_paths(config, n, episodes, device):
    """-> {path: callable -> (result triple, env steps of that evaluation)} on one agent."""
    import run as runpy
    from dtqn_amd.agents.device_eval import DeviceEvaluator
    from dtqn_amd.agents.vector import VectorEvaluator
    agent, make_env = make(config, device)
    single = Seeded(make_env(), 1000, 0, 1)
    copies = [Seeded(make_env(), 5000, i, n) for i in range(n)]
    vec = VectorEvaluator(agent, copies)
    dev = DeviceEvaluator(agent, ENV_IDS[config], n, 1701, max_episodes=max(1, episodes))

    def host_one():
        s0 = single.steps
        return runpy.evaluate(agent, single, episodes), single.steps - s0

    def host_vec():
        s0 = sum(c.steps for c in copies)
        return vec.evaluate(episodes), sum(c.steps for c in copies) - s0

    def device_vec():
        out = dev.evaluate(episodes)
        return out, int(dev.results().lengths.sum())

    return agent, {"run.evaluate": host_one, "VectorEvaluator": host_vec, "DeviceEvaluator": device_vec}


def eval_mode(config, a, device, summary):
    agent, paths = eval_paths(config, a.envs, a.episodes, device)
    for one in paths.values():
        one()                                                     # untimed
    ms, rate, last = {p: [] for p in paths}, {p: [] for p in paths}, {}
    for r in range(a.repeats):
        for p, one in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            result, steps = one()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ms[p].append(dt * 1e3)
            rate[p].append(steps / dt)
            last[p] = result
            print(json.dumps(dict(mode="eval", config=config, path=p, envs=1 if p == "run.evaluate" else a.envs, repeat=r, episodes=a.episodes,
                                  env_steps=steps, ms=round(dt * 1e3, 2), env_steps_per_s=round(steps / dt, 1),
                                  result=[round(float(v), 4) for v in result])), flush=True)
    for p in paths:
        summary.append(dict(mode="eval", config=config, path=p, envs=1 if p == "run.evaluate" else a.envs, episodes=a.episodes,
                            tiled=int(agent.engine.actor_net.tiled), ms_median=round(float(np.median(ms[p])), 2), ms_min=round(min(ms[p]), 2),
                            ms_max=round(max(ms[p]), 2), env_steps_per_s_median=round(float(np.median(rate[p])), 1),
                            env_steps_per_s_min=round(min(rate[p]), 1), env_steps_per_s_max=round(max(rate[p]), 1)))
    del agent, paths
    torch.cuda.empty_cache()


class _NoLog:
    def log(self, *a, **k):
        pass


def coupled_window(agent, vec, env, evaluators, updates, a):
    """`updates` iterations of run.train with an evaluation every a.eval_frequency steps, then a synchronise -> TD-updates/s."""
    import run as runpy
    from dtqn_amd.utils import epsilon_anneal
    eps = epsilon_anneal.LinearAnneal(0.1, 0.1, 1)
    torch.cuda.synchronize()
    t0, s0 = time.perf_counter(), agent.num_train_steps
    runpy.train(agent, [env], [env], [ENV_IDS["cfg1"]], s0 + updates, eps, a.eval_frequency, a.episodes, "", False, _NoLog(), None, None, None,
                None, vector=vec, evaluators=evaluators)
    vec.sync()
    torch.cuda.synchronize()
    return (agent.num_train_steps - s0) / (time.perf_counter() - t0)


def coupled_mode(a, device, summary):
    from time_device_rollout import make_path
    from dtqn_amd.agents.device_eval import DeviceEvaluator
    setups = {}
    for p in ("run.evaluate", "DeviceEvaluator"):
        agent, vec, envs_ = make_path("device", a.coupled_envs, device, 5000)
        evaluators = [DeviceEvaluator(agent, ENV_IDS["cfg1"], a.envs, 1701, max_episodes=max(1, a.episodes))] if p == "DeviceEvaluator" else None
        setups[p] = (agent, vec, envs_[0], evaluators)
    rates = {p: [] for p in setups}
    for p in setups:
        coupled_window(*setups[p], a.eval_frequency, a)           # warm-up: one evaluation
    for r in range(a.repeats):
        for p in setups:
            rate = coupled_window(*setups[p], a.updates, a)
            rates[p].append(rate)
            print(json.dumps(dict(mode="coupled", device_envs=a.coupled_envs, eval_path=p, eval_envs=a.envs if p == "DeviceEvaluator" else 1,
                                  repeat=r, updates=a.updates, eval_frequency=a.eval_frequency, updates_per_s=round(rate, 1))), flush=True)
    for p in setups:
        summary.append(dict(mode="coupled", device_envs=a.coupled_envs, eval_path=p, eval_frequency=a.eval_frequency, unit="updates/s",
                            median=round(float(np.median(rates[p])), 1), min=round(min(rates[p]), 1), max=round(max(rates[p]), 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", nargs="+", default=["eval", "coupled"], choices=["eval", "coupled"])
    ap.add_argument("--config", nargs="+", default=["cfg1", "cfg3"], choices=["cfg1", "cfg3"])
    ap.add_argument("--envs", type=int, default=10)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--coupled-envs", type=int, default=32)
    ap.add_argument("--eval-frequency", type=int, default=5000)
    ap.add_argument("--updates", type=int, default=20000, help="updates per coupled window (four evaluations at the default frequency)")
    a = ap.parse_args()
    device = torch.device("cuda:0")
    summary = []
    if "eval" in a.mode:
        for config in a.config:
            eval_mode(config, a, device, summary)
    if "coupled" in a.mode:
        coupled_mode(a, device, summary)
    for s in summary:
        print(json.dumps(dict(summary=s)), flush=True)


if __name__ == "__main__":
    main()
