"""Device-resident greedy evaluation of a bag network (`run.py --bag-size K --device-bag-eval-envs N`, DeviceBagEvaluator) against the
two host paths, and the candidate forward on a shared trunk against the candidate forward over N (K + 1) full sequences, on the config-1
network (d_model 64, 8 heads, 2 layers, context 50) with `--bag-size 5` and DiscreteCarFlag-v0:

  eval       env-steps/s of an evaluation of 10 episodes: DeviceBagEvaluator with N = 10 | VectorEvaluator with N = 10 (`--eval-envs 10`) |
             run.evaluate (one environment), the same agent behind all three;
  candidates us per call of dtqn_forward_bag_candidates (N trunks, N (K + 1) tails) | dtqn_forward_bag on the N (K + 1) tiled sequences
             (N (K + 1) trunks and tails: the launches of the rollout's tiled_forward_bag_resident candidate forward, whose embedding reads
             the N contexts through an index table instead) on the same device arrays, at N = 8, 10, 32.

Protocol: a host clock around work that ends in a device synchronise; one untimed warm-up per path, then windows of at least `--seconds`
(default 1.0); the paths alternate `--repeats` times (default 3) inside this one command.  One JSON line per window, then one summary line
per (mode, N, path) with the median and the spread (min .. max) over the repeats.

  python tests/perf/time_device_bag_eval.py
  python tests/perf/time_device_bag_eval.py --mode candidates --envs 10 --repeats 3"""
import argparse, ctypes, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

ENV_ID, BAG, EPISODES = "DiscreteCarFlag-v0", 5, 10


def make_agent(device, seed):
    from dtqn_amd import envs
    from dtqn_amd.utils import agent_utils
    from dtqn_amd.utils.random import set_global_seed
    env = envs.make(ENV_ID)
    set_global_seed(seed, env)
    agent = agent_utils.get_agent("DTQN", [env], 8, 0, 64, 100_000, device, 3e-4, 32, 50, -1, 50, 10_000, 0.99, 8, 2, 0.0, False, "res",
                                  "learned", BAG, sampler="device", sample_seed=seed)
    return agent, env


def eval_paths(agent, env, n):
    """path -> a call that plays EPISODES greedy episodes and returns the environment steps it took."""
    import run as runpy
    from dtqn_amd import envs
    from dtqn_amd.agents.device_bag_eval import DeviceBagEvaluator
    from dtqn_amd.agents.vector import VectorEvaluator
    dev_ev = DeviceBagEvaluator(agent, ENV_ID, n, 1701, max_episodes=EPISODES)
    copies = [envs.make(ENV_ID) for _ in range(n)]
    for k, e in enumerate(copies):
        e.seed(1501 + k)
    vec_ev = VectorEvaluator(agent, copies)
    steps = lambda triple: int(round(triple[2] * EPISODES))
    return {"device": lambda: steps(dev_ev.evaluate(EPISODES)), "host-vector": lambda: steps(vec_ev.evaluate(EPISODES)),
            "host-single": lambda: steps(runpy.evaluate(agent, env, EPISODES))}, dev_ev


def eval_window(play, seconds):
    """Evaluations until `seconds` have passed, then a synchronise -> env-steps/s."""
    torch.cuda.synchronize()
    t0, steps = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        steps += play()
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0)


def candidate_paths(agent, n):
    """path -> one enqueued candidate forward of n contexts x (BAG + 1) candidate bags on device arrays both paths share."""
    net, lib = agent.policy_network, agent.engine.lib
    ref, L, A, O, C = agent.engine._actor_net_ref, agent.context_len, agent.num_actions, int(agent.env_obs_length), BAG + 1
    dev, S = agent.device, n * C
    g = torch.Generator().manual_seed(3)
    obs = (torch.rand(n, L, O, generator=g) * 2 - 1).to(dev)
    act = torch.randint(0, A, (n, L), generator=g, dtype=torch.uint8).to(dev)
    cand_obs = (torch.rand(n, C, BAG, O, generator=g) * 2 - 1).to(dev)
    cand_act = torch.randint(0, A, (n, C, BAG), generator=g, dtype=torch.uint8).to(dev)
    obs_t, act_t = obs.repeat_interleave(C, dim=0).contiguous(), act.repeat_interleave(C, dim=0).contiguous()
    q = {p: torch.zeros(S * L * A, device=dev) for p in ("shared-trunk", "full-sequences")}
    ws = {"shared-trunk": torch.zeros(lib.dtqn_bag_candidates_workspace_floats(ref, n, C), device=dev),
          "full-sequences": torch.zeros(lib.dtqn_forward_workspace_floats(ref, S), device=dev)}
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    theta, stream = p(net.flat), agent.engine._stream()
    has_a = agent.engine.actor_net.action_dim > 0

    def shared():
        rc = lib.dtqn_forward_bag_candidates(ref, theta, p(obs), p(act) if has_a else None, p(cand_obs), p(cand_act) if has_a else None, n, C, L,
                                             p(q["shared-trunk"]), p(ws["shared-trunk"]), stream)
        assert rc == 0, rc

    def full():
        rc = lib.dtqn_forward_bag(ref, theta, p(obs_t), p(act_t) if has_a else None, p(cand_obs), p(cand_act) if has_a else None, S, L,
                                  p(q["full-sequences"]), p(ws["full-sequences"]), 0, 0, 0, stream)
        assert rc == 0, rc
    keep = (obs, act, cand_obs, cand_act, obs_t, act_t)
    return {"shared-trunk": shared, "full-sequences": full}, q, keep


def call_window(call, seconds, chunk=64):
    """Calls until `seconds` have passed, then a synchronise -> us per call."""
    torch.cuda.synchronize()
    t0, calls = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        for _ in range(chunk):
            call()
        calls += chunk
        torch.cuda.synchronize()                                 # (once per chunk: the queue never runs far ahead of the clock)
    return (time.perf_counter() - t0) / calls * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", nargs="+", default=["eval", "candidates"], choices=["eval", "candidates"])
    ap.add_argument("--eval-envs", type=int, default=10)
    ap.add_argument("--envs", type=int, nargs="+", default=[8, 10, 32], help="contexts of the candidate forward")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    agent, env = make_agent(device, 1)
    summary = []

    def run(mode, n, paths, window, unit, extra=None):
        rates = {p: [] for p in paths}
        for p in paths:                                          # warm-up: every shape the timed windows use
            window(paths[p], 0.2)
        for r in range(a.repeats):
            for p in paths:
                rate = window(paths[p], a.seconds)
                rates[p].append(rate)
                print(json.dumps(dict(mode=mode, envs=n, path=p, repeat=r, rate=round(rate, 1), unit=unit)), flush=True)
        for p in paths:
            summary.append(dict(mode=mode, envs=n, path=p, unit=unit, median=round(float(np.median(rates[p])), 1),
                                min=round(min(rates[p]), 1), max=round(max(rates[p]), 1), **(extra or {})))

    if "eval" in a.mode:
        paths, dev_ev = eval_paths(agent, env, a.eval_envs)
        run("eval", a.eval_envs, paths, eval_window, "env-steps/s")
        summary[-3]["candidate_forward_share"] = round(dev_ev.choice_steps / max(1, dev_ev.vector_steps), 4)
        summary[-3]["bag_counters"] = dev_ev.bag_counters()
    if "candidates" in a.mode:
        for n in a.envs:
            paths, q, keep = candidate_paths(agent, n)
            for p in paths:
                paths[p]()
            torch.cuda.synchronize()
            diff = float((q["shared-trunk"] - q["full-sequences"]).abs().max())
            run("candidates", n, paths, call_window, "us/call", dict(max_abs_difference=diff, bit_equal=bool(torch.equal(q["shared-trunk"], q["full-sequences"]))))
            del paths, q, keep
    for s in summary:
        print(json.dumps(dict(summary=s)), flush=True)


if __name__ == "__main__":
    main()
