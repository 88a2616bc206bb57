"""Wall time of ONE greedy evaluation of `--episodes` episodes (default 10, run.py's --eval-episodes) through the single-environment actor
(N = 1: run.evaluate, the path `run.py --eval-envs 1` takes) and through VectorEvaluator with N environments (`--eval-envs N`), at
  cfg1   config 1 shapes (d_model 64, 8 heads, 2 layers, context 50) on DiscreteCarFlag-v0,
  cfg3   config 3 shapes (d_model 128, 8 heads, 2 layers, context 50) on Memory-5-v0,
  image  frames of 3 x 144 x 144, d_model 64, context 50, a synthetic environment with episodes of 60 steps.
The parameters are those of a fresh agent and stand still.  Every episode is seeded by its number, so every N plays the same episodes
(up to near-ties of Q).  Protocol per (configuration, N): one untimed evaluation, then `--runs` timed ones (default 5), each between two
device synchronisations; the line reports the median, the minimum and the maximum in ms, and env-steps per second at the median.

  python tests/perf/time_eval.py                        # every configuration at N = 1, 5, 10
  python tests/perf/time_eval.py --config cfg1 --envs 10 --runs 3

Each result is one JSON line."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch


class Seeded:
    """Re-seeds the project's environment with (base + episode number) at every reset; first / stride: the episodes this copy plays."""

    def __init__(self, env, base, first, stride):
        self.env, self.base, self.first, self.stride, self.next = env, base, first, stride, first
        self.observation_space, self.action_space = env.observation_space, env.action_space
        self.steps = 0

    def rewind(self):
        self.next, self.steps = self.first, 0

    def reset(self):
        inner = self.env
        while hasattr(inner, "env"):
            inner = inner.env
        if hasattr(inner, "np_random"):
            inner.np_random = None
        self.env.seed(self.base + self.next)
        self.next += self.stride
        return self.env.reset()

    def step(self, action):
        self.steps += 1
        return self.env.step(action)


class PoolEnv:
    def __init__(self, shape, ep_len=60, actions=8):
        from dtqn_amd.envs import spaces
        self.observation_space = spaces.Box(low=0, high=255, shape=shape, dtype=np.uint8)
        self.action_space = spaces.Discrete(actions)
        self._max_episode_steps = ep_len
        self.pool = np.random.default_rng(5).integers(0, 256, size=(16,) + tuple(shape), dtype=np.uint8)
        self.seed(0)

    def seed(self, seed=None):
        self.rng = np.random.default_rng(seed)
        return [seed]

    def reset(self):
        self.t = 0
        return self.pool[int(self.rng.integers(16))]

    def step(self, action):
        self.t += 1
        return self.pool[int(self.rng.integers(16))], 0.0, self.t >= self._max_episode_steps, {}


def make(config, device):
    """-> (agent, factory of one environment)."""
    from dtqn_amd import envs
    from dtqn_amd.utils import agent_utils
    from dtqn_amd.utils.random import set_global_seed
    if config == "image":
        from dtqn_amd.agents.dtqn import DtqnAgent
        from dtqn_amd.networks.dtqn import DTQN
        shape, ctx = (3, 144, 144), 50
        set_global_seed(1)
        factory = lambda: DTQN(shape, 8, 8, 0, 64, 8, 2, ctx).to(device)
        agent = DtqnAgent(factory, buffer_size=4 * 60, device=device, env_obs_length=shape, max_env_steps=60, obs_mask=0, num_actions=8,
                          is_discrete_env=False, batch_size=2, context_len=ctx, history=ctx, target_update_frequency=10_000,
                          sampler="device", sample_seed=1)
        return agent, lambda: PoolEnv(shape)
    env_id, d_model = {"cfg1": ("DiscreteCarFlag-v0", 64), "cfg3": ("Memory-5-v0", 128)}[config]
    env = envs.make(env_id)
    set_global_seed(1, env)
    agent = agent_utils.get_agent("DTQN", [env], 8, 0, d_model, 4000, device, 3e-4, 32, 50, -1, 50, 10_000, 0.99, 8, 2, 0.0, False, "res",
                                  "learned", 0, sampler="device", sample_seed=1)
    return agent, lambda: envs.make(env_id)


def run(config, n_envs, a, device):
    import run as runpy
    from dtqn_amd.agents.vector import VectorEvaluator
    agent, make_env = make(config, device)
    copies = [Seeded(make_env(), 1000, i, n_envs) for i in range(n_envs)]
    if n_envs == 1:
        one = lambda: runpy.evaluate(agent, copies[0], a.episodes)
    else:
        ev = VectorEvaluator(agent, copies)
        one = lambda: ev.evaluate(a.episodes)
    times, result = [], None
    for k in range(a.runs + 1):
        for c in copies:
            c.rewind()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = one()
        torch.cuda.synchronize()
        if k > 0:
            times.append((time.perf_counter() - t0) * 1e3)
    steps = sum(c.steps for c in copies)
    med = float(np.median(times))
    print(json.dumps(dict(config=config, envs=n_envs, path="run.evaluate" if n_envs == 1 else "VectorEvaluator", episodes=a.episodes,
                          tiled=int(agent.engine.actor_net.tiled), runs=a.runs, env_steps=steps, ms_median=round(med, 2),
                          ms_min=round(min(times), 2), ms_max=round(max(times), 2), env_steps_per_s=round(steps / med * 1e3, 1),
                          result=[round(float(v), 4) for v in result])), flush=True)
    del agent
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", nargs="+", default=["cfg1", "cfg3", "image"], choices=["cfg1", "cfg3", "image"])
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 5, 10])
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    for config in a.config:
        for n in a.envs:
            run(config, n, a, device)


if __name__ == "__main__":
    main()
