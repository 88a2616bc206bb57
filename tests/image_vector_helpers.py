"""Shared by test_image_vector.py (HIP emulation on the CPU) and test_gpu_image_vector.py (MI355X): a seeded synthetic pixel environment
with a fixed episode length, an image agent at the shape the issue names (d_model 64, 8 heads, 1 layer, context 6, 4 actions), and the
checks of the vectorised image rollout (dtqn_amd/agents/vector.py, dtqn_img_actor_forward_batch)."""
import numpy as np
import torch

from oracle import dtqn_oracle as O

from q_f64_helpers import check_forward_f64, check_pooled_f64

L, D, H, NL, A = 6, 64, 8, 1, 4
REUSE_ENV = "DTQN_IMG_ACTOR_REUSE"


class PixelEnv:
    """Frames of seeded uniform noise, episodes of exactly `ep_len` steps, a reward that depends on the action."""

    def __init__(self, shape, ep_len, seed):
        from dtqn_amd.envs import spaces
        self.shape, self._max_episode_steps = tuple(shape), int(ep_len)
        self.observation_space = spaces.Box(low=0, high=255, shape=self.shape, dtype=np.uint8)
        self.action_space = spaces.Discrete(A)
        self.rng = np.random.default_rng(seed)
        self.taken = []

    def _obs(self):
        return self.rng.integers(0, 256, size=self.shape, dtype=np.uint8)

    def reset(self):
        self.t = 0
        return self._obs()

    def step(self, action):
        self.t += 1
        self.taken.append(int(action))
        return self._obs(), float(action == self.t % A), self.t >= self._max_episode_steps, {}

    def seed(self, seed=None):
        self.rng = np.random.default_rng(seed)
        return [seed]


def make_envs(shape, lengths=(2, 5, 11), seed=100):
    return [PixelEnv(shape, n, seed + k) for k, n in enumerate(lengths)]


def make_agent(lib, device, shape, dropout=0.0, batch=2, seed=3, max_steps=11):
    """lib: the emulation library (agent on the CPU), or None for the product engine on `device`."""
    from dtqn_amd.agents.dtqn import DtqnAgent
    from dtqn_amd.networks.dtqn import DTQN
    from dtqn_amd.utils.random import set_global_seed
    set_global_seed(seed)

    def factory():
        m = DTQN(tuple(shape), A, 8, 0, D, H, NL, L, dropout=dropout, **({"_test_lib": lib} if lib is not None else {}))
        m._allow_cpu = lib is not None
        return m.to(device)
    return DtqnAgent(factory, buffer_size=24 * max_steps, device=torch.device(device), env_obs_length=tuple(shape), max_env_steps=max_steps,
                     obs_mask=0, num_actions=A, is_discrete_env=False, batch_size=batch, context_len=L, history=L,
                     target_update_frequency=1000, sampler="device", sample_seed=seed)


def oracle_cfg(shape, dropout=0.0):
    return O.NetCfg(obs_dim=int(np.prod(shape)), num_actions=A, inner_embed_size=D, num_heads=H, num_layers=NL, history_len=L,
                    dropout=dropout, image=tuple(shape))


def prefixes(vec):
    """The frames of every environment's current window, oldest first: [n_i, C, H, W] uint8 (from the episodes the actor collects)."""
    out = []
    for ep in vec.episodes:
        frames = [ep[0]] + [e[0] for e in ep[1:]]
        out.append(np.stack(frames[-vec.L:]))
    return out


def module_rows(agent, pre, drop=None):
    """Row len_i - 1 of DTQN.forward on every prefix alone, zero-padded to the longest one."""
    n_max = max(len(p) for p in pre)
    rows = []
    for p in pre:
        obs = np.zeros((1, n_max) + p.shape[1:], dtype=np.uint8)
        obs[0, :len(p)] = p
        q = agent.policy_network(torch.as_tensor(obs), None, _train_dropout=drop)
        rows.append(q[0, len(p) - 1].cpu().numpy())
    return np.stack(rows)


def oracle_rows(agent, shape, pre):
    params = {k: v.detach().cpu().clone() for k, v in agent.policy_network.state_dict().items()}
    cfg = oracle_cfg(shape)
    with torch.no_grad():
        return np.stack([O.forward(params, cfg, torch.as_tensor(p[None])).numpy()[0, -1] for p in pre])


def check_step(agent, vec, shape, q, where, oracle=True):
    """q [N, A] of one vector step against the module forward (bit for bit) and the oracle (the project's Q bound)."""
    pre = prefixes(vec)
    qm = module_rows(agent, pre)
    print(where, "max |q - module| =", float(np.abs(q - qm).max()))
    assert np.array_equal(q, qm), (where, q, qm)
    if oracle:
        ref = oracle_rows(agent, shape, pre)
        err, bound = float(np.abs(q - ref).max()), 1e-4 * max(1.0, float(np.abs(ref).max()))
        print(where, "max |q - oracle| =", err, "bound", bound)
        assert err <= bound, (where, err, bound)
        params = {k: v.detach().cpu().clone() for k, v in agent.policy_network.state_dict().items()}
        pool = []                 # ... and the reported row of every environment against float64, one yardstick for the step
        for i, p in enumerate(pre):
            check_forward_f64(oracle_cfg(shape), params, p[None], None, q[i:i + 1], what=(where, "env", i), pool=pool)
        check_pooled_f64(pool)
    return pre


def frozen_run(agent, vec, shape, steps=20, eps=0.3, oracle=True, check=True):
    """`steps` vector steps with the parameters standing still -> (Q of every step, encoded tokens of every step, new frames of every step)."""
    lib = agent.engine.lib
    vec.reset_all()
    qs, tokens, fresh = [], [], []
    for step in range(steps):
        before = vec._pushed.copy()
        q = vec.q_values().copy()
        tokens.append(int(lib.dtqn_debug_last_img_actor_tokens()))
        fresh.append(int((before != vec._pushed).sum()))
        if check:
            pre = check_step(agent, vec, shape, q, ("frozen", step), oracle=oracle)
            assert [len(p) for p in pre] == [min(L, c.timestep + 1) for c in vec.contexts]
        qs.append(q)
        vec.max_t = max(getattr(vec, "max_t", 0), max(c.timestep for c in vec.contexts))      # (the longest context a launch saw)
        vec.step_all(eps)
    return np.stack(qs), tokens, fresh


def prefill(agent, shape, episodes=6, ep_len=9, seed=50):
    """Finished random episodes in the replay, so that train() can sample."""
    rng = np.random.default_rng(seed)
    rb = agent.replay_buffer
    for _ in range(episodes):
        rb.store_obs(rng.integers(0, 256, size=shape, dtype=np.uint8))
        for t in range(ep_len):
            rb.store(rng.integers(0, 256, size=shape, dtype=np.uint8), int(rng.integers(A)), float(rng.integers(2)), t == ep_len - 1, t + 1)
        rb.flush()
    assert rb.can_sample(agent.batch_size)


def training_run(agent, vec, shape, steps=20, reload_at=None):
    """An agent.train() between vector steps (and optionally a host-side load_state_dict): Q must follow the current parameters."""
    prefill(agent, shape)
    vec.reset_all()
    moved = 0
    for step in range(steps):
        q = vec.q_values().copy()
        check_step(agent, vec, shape, q, ("train", step), oracle=False)
        vec.step_all(0.3)
        before = agent.policy_network.flat.clone()
        if step == reload_at:          # a host-side write alone: no optimizer launch tells the actor about it
            sd = {k: (v + 0.01 if k.endswith("obs_embedding.observation_embedding.0.bias") else v.clone())
                  for k, v in agent.policy_network.state_dict().items()}
            agent.policy_network.load_state_dict(sd)
        else:
            agent.train()
        moved += int(not torch.equal(before, agent.policy_network.flat))
    assert moved == steps and agent.num_train_steps == steps - (reload_at is not None)
