"""Host-side rollout environments and their registry (reference ids: envs/__init__.py:31-48).

Only the envs that are self-contained in the reference are restated (CarFlag, Memory).  The
gridverse / gym-pomdps / MiniHack families need third-party simulators that are not vendored by the
reference and are absent here; `make` falls through to `gym.make` for them when gym is installed.

Tabular POMDPs are this project's own (pomdp_file.py, pomdp.py): `make` takes a path ending in `.pomdp`, or the ids
`POMDP-<name>-episodic-v0` / `POMDP-<name>-v0`, which resolve `<name>.pomdp` in the directories of the DTQN_POMDP_PATH environment
variable first and in the bundled pomdp_models/ then.
"""
import dataclasses
import os
import re

import numpy as np

from .car_flag import CarFlag
from .memory_cards import Memory
from .pomdp import TabularPOMDP
from .pomdp_file import PomdpModel, load_pomdp
from .time_limit import TimeLimit

REGISTRY = {
    "DiscreteCarFlag-v0": lambda: TimeLimit(CarFlag(discrete=True), max_episode_steps=200),
    "Memory-5-v0": lambda: TimeLimit(Memory(num_pairs=5), max_episode_steps=50),
}

POMDP_MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pomdp_models")
POMDP_CAPS = {"tiger": 50, "corridor": 100}        # step caps of the bundled models
_POMDP_ID = re.compile(r"^POMDP-(.+?)(-episodic)?-v0$")


def is_pomdp(id_or_path: str) -> bool:
    return str(id_or_path).endswith(".pomdp") or _POMDP_ID.match(str(id_or_path)) is not None


def _find_model(name: str) -> str:
    dirs = [d for d in os.environ.get("DTQN_POMDP_PATH", "").split(os.pathsep) if d] + [POMDP_MODELS]
    for d in dirs:
        path = os.path.join(d, name + ".pomdp")
        if os.path.isfile(path):
            return path
    raise KeyError(f"no {name}.pomdp in {dirs} (DTQN_POMDP_PATH names directories of your own models; "
                   f"bundled: {sorted(POMDP_CAPS)})")


def make_pomdp(id_or_path: str, max_episode_steps=None):
    """A `.pomdp` path or a POMDP id -> TimeLimit(TabularPOMDP).  The cap: `max_episode_steps`, else the bundled model's own; a path
    or a model of the user's has none, and is refused without one."""
    m = _POMDP_ID.match(id_or_path)
    if id_or_path.endswith(".pomdp"):
        path, episodic, cap = id_or_path, True, None
        if not os.path.isfile(path):
            raise KeyError(f"no such file: {path!r}")
    else:
        name, episodic = m.group(1), m.group(2) is not None
        path = _find_model(name)
        cap = POMDP_CAPS.get(name) if os.path.dirname(path) == POMDP_MODELS else None
    if max_episode_steps is not None and int(max_episode_steps) > 0:
        cap = int(max_episode_steps)
    if cap is None:
        raise ValueError(f"{id_or_path!r} has no step cap of its own: give one with --max-episode-steps (make(..., max_episode_steps=N))")
    model = load_pomdp(path)
    if episodic and not model.episodic:
        raise ValueError(f"{id_or_path!r}: {path} has no `reset` pair, so no episode of it ends (use the id without -episodic)")
    if not episodic and model.episodic:              # the continuing form: a reset pair restarts the state, the episode goes on
        model = dataclasses.replace(model, D=np.zeros_like(model.D), episodic=False)
    return TimeLimit(TabularPOMDP(model), max_episode_steps=cap)


def make(env_id: str, max_episode_steps=None):
    """max_episode_steps: the step cap of a tabular POMDP (required for a `.pomdp` path); the registered ids keep their own."""
    if env_id in REGISTRY:
        return REGISTRY[env_id]()
    if is_pomdp(env_id):
        return make_pomdp(env_id, max_episode_steps)
    try:
        import gym
    except ImportError as exc:
        raise KeyError(
            f"Unknown environment {env_id!r}: dtqn_amd ships {sorted(REGISTRY)} and tabular POMDPs (a .pomdp path, POMDP-<name>-episodic-v0, "
            f"POMDP-<name>-v0; bundled: {sorted(POMDP_CAPS)}); gridverse / gym-pomdps / MiniHack "
            "domains need their third-party packages plus gym, which are not installed") from exc
    return gym.make(env_id)
