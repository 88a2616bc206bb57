"""Environment construction and introspection (reference: utils/env_processing.py).

Space types are recognised by class NAME so that both dtqn_amd.envs.spaces and (when installed)
gym.spaces objects work."""
from typing import Union

import numpy as np

from .. import envs as _envs

DISCRETE_KINDS = ("Discrete", "MultiDiscrete", "MultiBinary")


def _kind(space) -> str:
    return type(space).__name__


def make_env(id_or_path: str, max_episode_steps=None):
    """Registered id, POMDP id or `.pomdp` path -> env.  (The reference falls back to a gridverse YAML factory here,
    utils/env_processing.py:36-54; that simulator is not available, see dtqn_amd.envs.)  max_episode_steps: the step cap of a
    tabular POMDP (a `.pomdp` path needs one); the registered ids keep their own."""
    return _envs.make(id_or_path, max_episode_steps=max_episode_steps)


def is_discrete_env(env) -> bool:
    return _kind(env.observation_space) in DISCRETE_KINDS


def is_image_env(env) -> bool:
    space = env.observation_space
    return (_kind(space) == "Box" and len(getattr(space, "shape", ())) == 3
            and np.all(np.asarray(space.low) == 0) and np.all(np.asarray(space.high) == 255))


def _probe_reset(env):
    """The reference decides the observation type by looking at a SAMPLE observation: `get_env_obs_type` calls `env.reset()`
    (utils/env_processing.py:63-66), and both get_env_obs_length and get_env_obs_mask go through it.  Those resets advance the
    env's own random stream before the first rollout step (get_agent runs them on envs[0], agent_utils.py:87-88), so a seeded
    run only visits the reference's episodes if they happen here too (pinned by tests/golden G12)."""
    return env.reset()


def get_env_obs_length(env) -> int:
    space = env.observation_space
    _probe_reset(env)
    if is_image_env(env):
        return tuple(int(v) for v in np.shape(env.reset()))      # utils/env_processing.py:86-87: the observation's (C, H, W) shape
    kind = _kind(space)
    if kind == "Discrete":
        return 1
    if kind in ("MultiDiscrete", "Box"):
        if len(space.shape) != 1:
            raise NotImplementedError("We do not yet support 2D observation spaces")
        return int(space.shape[0])
    if kind == "MultiBinary":
        return int(space.n)
    raise NotImplementedError(f"We do not yet support {space}")


def get_env_obs_mask(env) -> Union[int, float]:
    """Padding value for unseen observations: one past the largest token for discrete spaces,
    -5 for continuous ones (below CarFlag's minimum of -1.1; utils/env_processing.py:100-120)."""
    space = env.observation_space
    _probe_reset(env)
    if is_image_env(env):
        return 0                                                 # utils/env_processing.py:106-108
    kind = _kind(space)
    if kind == "Discrete":
        return int(space.n)
    if kind == "MultiDiscrete":
        return int(max(space.nvec)) + 1
    if kind == "Box":
        return -5
    raise NotImplementedError(f"We do not yet support {space}")


def get_env_max_steps(env):
    for attr in ("_max_episode_steps", "max_episode_steps"):
        try:
            return getattr(env, attr)
        except AttributeError:
            continue
    return None
