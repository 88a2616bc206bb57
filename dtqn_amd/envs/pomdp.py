"""Tabular POMDP environment over a PomdpModel (envs/pomdp_file.py): `Discrete(Z)` observations -- the token index --
and `Discrete(A)` actions.

The semantics are this project's own (DESIGN.md "Tabular POMDP environments"), modelled on what gym-pomdps is understood to do, with
no claim of bit-equality with that package:
  * reset: s0 is drawn from `start`, the first observation from O[first_obs_action][s0].  A POMDP has no observation before an
    action; this is the stated convention, and immaterial for models whose O ignores the action;
  * step(a): s' is drawn from T[a][s], z from O[a][s'], reward = R[a][s][s'][z], done = D[a][s] (the `reset` pairs of the file),
    info["is_success"] = done and reward > 0.
Every draw is "the first k with u < cdf[k]" on the CDFs the parser derived; `reset_with` / `step_with` take the uniforms, so the
device-resident environments (csrc/dtqn_devenv.hpp) can be replayed draw for draw.
"""
import numpy as np
from numpy.random import Generator

from . import spaces
from .pomdp_file import PomdpModel, draw


class TabularPOMDP:
    def __init__(self, model: PomdpModel, first_obs_action: int = 0):
        S, A, Z = model.sizes
        if not 0 <= int(first_obs_action) < A:
            raise ValueError(f"first_obs_action {first_obs_action} is not one of the {A} actions")
        self.model, self.first_obs_action = model, int(first_obs_action)
        self.observation_space = spaces.Discrete(Z)
        self.action_space = spaces.Discrete(A)
        self.state = -1
        self.np_random = None

    def seed(self, seed=None):
        if self.np_random is None:
            self.np_random = Generator(np.random.PCG64(np.random.SeedSequence(seed)))
        return [seed]

    def reset_with(self, u_state: float, u_obs: float) -> int:
        m = self.model
        self.state = draw(m.start_cdf, u_state)
        return draw(m.O_cdf[self.first_obs_action, self.state], u_obs)

    def step_with(self, action: int, u_state: float, u_obs: float):
        m, s, a = self.model, self.state, int(action)
        if s < 0:
            raise ValueError("Trying to take step in invalid state. Did you reset?")
        if not 0 <= a < self.action_space.n:
            raise ValueError(f"action {action} is not one of the {self.action_space.n} actions")
        s2 = draw(m.T_cdf[a, s], u_state)
        z = draw(m.O_cdf[a, s2], u_obs)
        reward = float(m.R[a, s, s2, z])
        done = bool(m.D[a, s])
        self.state = s2
        return z, reward, done, {"is_success": done and reward > 0}

    def reset(self):
        return self.reset_with(self.np_random.random(), self.np_random.random())

    def step(self, action: int):
        return self.step_with(action, self.np_random.random(), self.np_random.random())
