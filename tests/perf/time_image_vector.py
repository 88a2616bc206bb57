"""Actor-only env-steps/s of an image agent: the single-environment path (DtqnAgent._image_action: the whole context uploaded and encoded
on every step) against the vectorised rollout (VectorActor: N frames uploaded per vector step, only the frames without a current
embedding encoded), each with the parameters frozen (no update) and with one agent.train() per (vector) step.  One process, one
build.  Protocol per case: `--warmup` (vector) steps, synchronise, wall clock over `--steps` (vector) steps, synchronise; one run each.
Both paths are in train mode (the networks have no dropout) and write their episodes to the device replay, so with the defaults
(60 + 60 steps, episodes of 120) every environment's one episode end -- 120 frames into the replay -- falls inside the timed window of
either path.  The vectorised cases also report where the host spent the step: staging + library call (`launch`), waiting for Q
(`wait`), replaying finished episodes (`commit`).

  python tests/perf/time_image_vector.py                                   # (3, 144, 144), context 50, d_model 64: N = 1, 8, 32
  python tests/perf/time_image_vector.py --envs 8 --mode frozen --steps 50     # one case (e.g. under rocprofv3 --kernel-trace --stats -- ...)

Each result is one JSON line.  The environments are synthetic (frames out of a pool of random images, episodes of 120 steps), so the
figures are actor rates, not learning curves.  The warm-up should be at least the context length, so that every window is full."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch


class PoolEnv:
    def __init__(self, shape, seed, ep_len=120, actions=8):
        from dtqn_amd.envs import spaces
        self.observation_space = spaces.Box(low=0, high=255, shape=shape, dtype=np.uint8)
        self.action_space = spaces.Discrete(actions)
        self._max_episode_steps = ep_len
        self.rng = np.random.default_rng(seed)
        self.pool = self.rng.integers(0, 256, size=(16,) + tuple(shape), dtype=np.uint8)

    def reset(self):
        self.t = 0
        return self.pool[int(self.rng.integers(16))]

    def step(self, action):
        self.t += 1
        return self.pool[int(self.rng.integers(16))], 0.0, self.t >= self._max_episode_steps, {}


def make_agent(shape, ctx, d_model, heads, layers, batch, device, seed=1):
    from dtqn_amd.agents.dtqn import DtqnAgent
    from dtqn_amd.networks.dtqn import DTQN
    from dtqn_amd.utils.random import set_global_seed
    set_global_seed(seed)
    T = 120
    factory = lambda: DTQN(tuple(shape), 8, 8, 0, d_model, heads, layers, ctx).to(device)
    agent = DtqnAgent(factory, buffer_size=48 * T, device=device, env_obs_length=tuple(shape), max_env_steps=T, obs_mask=0, num_actions=8,
                      is_discrete_env=False, batch_size=batch, context_len=ctx, history=ctx, target_update_frequency=10_000,
                      sampler="device", sample_seed=seed)
    env, rb = PoolEnv(shape, 99), agent.replay_buffer
    for _ in range(batch + 8):                  # finished episodes, so that train() can sample
        rb.store_obs(env.reset())
        for t in range(ctx + 10):
            rb.store(env.step(0)[0], 0, 0.0, t == ctx + 9, t + 1)
        rb.flush()
    return agent


def run(a, n_envs, mode, device):
    import run as runpy
    from dtqn_amd.agents.vector import VectorActor
    from dtqn_amd.utils.epsilon_anneal import Constant
    agent = make_agent(a.shape, a.ctx, a.d_model, a.heads, a.layers, a.batch, device)
    frozen = mode == "frozen"
    host = {}
    if n_envs == 1:
        env, eps = PoolEnv(a.shape, 7), Constant(0.0)
        agent.context_reset(env.reset())

        def one():
            if runpy.step(agent, env, eps):
                agent.replay_buffer.flush()
                agent.context_reset(env.reset())
            if not frozen:
                agent.train()
    else:
        vec = VectorActor(agent, [PoolEnv(a.shape, 7 + k) for k in range(n_envs)])
        vec.reset_all()
        one = lambda: vec.step_all(0.0, updates=0 if frozen else 1)

        def clocked(obj, name, key):
            inner = getattr(obj, name)
            host[key] = 0.0

            def f(*args, **kw):
                t = time.perf_counter()
                try:
                    return inner(*args, **kw)
                finally:
                    host[key] += time.perf_counter() - t
            setattr(obj, name, f)
    for _ in range(a.warmup):
        one()
    torch.cuda.synchronize()
    if n_envs > 1:
        for obj, name, key in ((vec._be, "launch", "launch_q"), (vec._be, "wait", "wait_q"), (vec, "_commit_episode", "commit_episode")):
            clocked(obj, name, key)
    t0 = time.perf_counter()
    for _ in range(a.steps):
        one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    assert agent.num_train_steps == (0 if frozen else a.warmup + a.steps), "the updates of this case did not run"
    print(json.dumps(dict(shape=list(a.shape), ctx=a.ctx, d_model=a.d_model, layers=a.layers, batch=a.batch, envs=n_envs, mode=mode,
                          path="_image_action" if n_envs == 1 else "VectorActor", warmup=a.warmup, steps=a.steps,
                          ms_per_step=round(dt * 1e3, 3), env_steps_per_s=round(n_envs / dt, 1),
                          host_ms_per_step={k.strip("_"): round(v / a.steps * 1e3, 3) for k, v in host.items()})), flush=True)
    del agent
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[3, 144, 144])
    ap.add_argument("--ctx", type=int, default=50)
    ap.add_argument("--d-model", type=int, default=64)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--envs", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--mode", choices=["frozen", "updates"], nargs="+", default=["frozen", "updates"])
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--steps", type=int, default=60)
    a = ap.parse_args()
    a.shape = tuple(a.shape)
    device = torch.device("cuda:0")
    for n in a.envs:
        for mode in a.mode:
            run(a, n, mode, device)


if __name__ == "__main__":
    main()
