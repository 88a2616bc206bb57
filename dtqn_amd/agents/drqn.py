"""DRQN agent with the reference's surface (dtqn/agents/drqn.py:13-210 and the parts of dtqn/agents/dqn.py:24-327 it inherits).

The network runs on the gfx950 LSTM kernels (dtqn_amd.networks.DRQN); the update around it is written in torch on that module:
three packed forwards, the double-DQN target, the MSE over the last `history` columns, clip_grad_norm_ and torch.optim.Adam.  The
fused TD update, the vectorised and device-resident rollouts and data parallelism do not cover this agent.
"""
from __future__ import annotations

import random
from typing import Callable, Optional, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from ..buffers.replay_buffer import ReplayBuffer
from ..utils.context import Context
from ..utils.logging_utils import RunningAverage
from ..utils.random import RNG
from .dtqn import TrainMode

_STATS = ("td_errors", "grad_norms", "qvalue_max", "qvalue_mean", "qvalue_min", "target_max", "target_mean", "target_min")


class DrqnAgent:
    def __init__(self, network_factory: Callable[[], torch.nn.Module], buffer_size: int, device: torch.device,
                 env_obs_length: int, max_env_steps: int, obs_mask: Union[int, float], num_actions: int,
                 is_discrete_env: bool, learning_rate: float = 0.0003, batch_size: int = 32, context_len: int = 50,
                 gamma: float = 0.99, grad_norm_clip: float = 1.0, target_update_frequency: int = 10_000,
                 embed_size: int = 64, history: int = 50, ref_quirks: bool = False, **kwargs):
        if isinstance(env_obs_length, (tuple, list)):
            raise NotImplementedError("DrqnAgent: image observations are not covered")
        self.context_len, self.env_obs_length = context_len, env_obs_length
        self.device = torch.device(device)
        self.policy_network = network_factory()
        self.target_network = network_factory()
        self.target_update()
        self.target_network.eval()
        self.is_discrete_env = is_discrete_env
        self.obs_context_type = np.int_ if is_discrete_env else np.float32
        self.obs_tensor_type = torch.long if is_discrete_env else torch.float32
        self.optimizer = torch.optim.Adam(self.policy_network.parameters(), lr=learning_rate)
        self.replay_buffer = ReplayBuffer(buffer_size, env_obs_length=env_obs_length, obs_mask=obs_mask, max_episode_steps=max_env_steps,
                                          context_len=context_len, device=self.device, lib=self.policy_network._lib)
        self.batch_size, self.gamma = batch_size, gamma
        self.grad_norm_clip, self.target_update_frequency = grad_norm_clip, target_update_frequency
        self.history = history
        self.num_train_steps = 0
        for name in _STATS:
            setattr(self, name, RunningAverage(100))
        self.num_actions, self.obs_mask = num_actions, obs_mask
        self.train_mode = TrainMode.TRAIN
        self.zeros_hidden = torch.zeros(1, 1, embed_size, dtype=torch.float32, device=self.device, requires_grad=False)
        hidden_states = (self.zeros_hidden, self.zeros_hidden)
        mk = lambda: Context(context_len, obs_mask, num_actions, env_obs_length, init_hidden=hidden_states, discrete=is_discrete_env,
                             ref_quirks=ref_quirks)
        self.train_context, self.eval_context = mk(), mk()

    @property
    def context(self) -> Context:
        return self.train_context if self.train_mode == TrainMode.TRAIN else self.eval_context

    def eval_on(self) -> None:
        self.train_mode = TrainMode.EVAL
        self.policy_network.eval()

    def eval_off(self) -> None:
        self.train_mode = TrainMode.TRAIN
        self.policy_network.train()

    def context_reset(self, obs: np.ndarray) -> None:
        self.context.reset(obs)
        if self.train_mode == TrainMode.TRAIN:
            self.replay_buffer.store_obs(obs)

    def observe(self, obs, action, reward, done) -> None:
        self.context.add_transition(obs, action, reward, done)
        if self.train_mode == TrainMode.TRAIN:
            self.replay_buffer.store(obs, action, reward, done, self.context.timestep)

    @torch.no_grad()
    def get_action(self, epsilon: float = 0.0) -> int:
        """drqn.py:84-112: the network always steps on the newest observation with the carried state; epsilon is drawn after that."""
        row = min(self.context.timestep, self.context_len - 1)
        obs = torch.as_tensor(self.context.obs[row], dtype=self.obs_tensor_type, device=self.device).unsqueeze(0).unsqueeze(0)
        act = torch.as_tensor(self.context.action[row], dtype=torch.long, device=self.device).unsqueeze(0).unsqueeze(0)
        q_values, self.context.hidden = self.policy_network(obs, act, hidden_states=self.context.hidden)
        if RNG.rng.random() < epsilon:
            return RNG.rng.integers(self.num_actions)
        return torch.argmax(q_values).item()

    def _td_loss(self, obss, actions, rewards, next_obss, next_actions, dones, episode_lengths):
        """drqn.py:129-184 on one sampled batch: (loss, q, targets), q and targets cut to the last `history` columns."""
        dev = self.device
        obss = torch.as_tensor(obss, dtype=self.obs_tensor_type, device=dev)
        next_obss = torch.as_tensor(next_obss, dtype=self.obs_tensor_type, device=dev)
        actions = torch.as_tensor(actions, dtype=torch.long, device=dev)
        next_actions = torch.as_tensor(next_actions, dtype=torch.long, device=dev)
        rewards = torch.as_tensor(rewards, dtype=torch.float32, device=dev)
        dones = torch.as_tensor(dones, dtype=torch.long, device=dev)
        # the replay's int32 lengths (the reference's uint8 storage wraps at 256; not reproduced)
        episode_lengths = torch.as_tensor(np.asarray(episode_lengths), dtype=torch.long, device=torch.device("cpu")).reshape(-1)
        q_values, _ = self.policy_network(obss, actions, episode_lengths=episode_lengths)
        q_values = q_values.gather(2, actions).squeeze(-1)
        with torch.no_grad():
            argmax = torch.argmax(self.policy_network(next_obss, next_actions, episode_lengths=episode_lengths)[0], dim=2).unsqueeze(-1)
            next_obs_q_values = self.target_network(next_obss, next_actions, episode_lengths=episode_lengths)[0].gather(2, argmax).squeeze(-1)
            targets = rewards.squeeze(-1) + (1 - dones.squeeze(-1)) * (next_obs_q_values * self.gamma)
        q_values = q_values[:, -self.history:]
        targets = targets[:, -self.history:]
        return F.mse_loss(q_values, targets), q_values, targets

    def train_on_batch(self, batch) -> None:
        """One update on a batch shaped like ReplayBuffer.sample()'s return value."""
        loss, q_values, targets = self._td_loss(*batch)
        self.qvalue_max.add(q_values.max().item())
        self.qvalue_mean.add(q_values.mean().item())
        self.qvalue_min.add(q_values.min().item())
        self.target_max.add(targets.max().item())
        self.target_mean.add(targets.mean().item())
        self.target_min.add(targets.min().item())
        self.td_errors.add(loss.item())
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(self.policy_network.parameters(), self.grad_norm_clip, error_if_nonfinite=True)
        self.grad_norms.add(norm.item())
        self.optimizer.step()
        self.num_train_steps += 1
        if self.num_train_steps % self.target_update_frequency == 0:
            self.target_update()

    def train(self) -> None:
        if not self.replay_buffer.can_sample(self.batch_size):
            return
        self.eval_off()
        self.train_on_batch(self.replay_buffer.sample(self.batch_size))

    def target_update(self) -> None:
        """Hard update: the policy network's parameters are copied into the target network."""
        self.target_network.load_state_dict(self.policy_network.state_dict())

    # ---- checkpoints (dqn.py:212-327), plain arrays instead of pickled objects -------------------
    def save_mini_checkpoint(self, checkpoint_dir: str, wandb_id: Optional[str]) -> None:
        torch.save({"step": self.num_train_steps, "wandb_id": wandb_id}, checkpoint_dir + "_mini_checkpoint.pt")

    @staticmethod
    def load_mini_checkpoint(checkpoint_dir: str) -> dict:
        return torch.load(checkpoint_dir + "_mini_checkpoint.pt")

    def _optimizer_arrays(self) -> dict:
        """Adam's state keyed by parameter name: step, exp_avg, exp_avg_sq as plain arrays."""
        out = {}
        for name, p in self.policy_network.named_parameters():
            st = self.optimizer.state.get(p)
            if st:
                out[name] = {"step": float(st["step"]), "exp_avg": st["exp_avg"].detach().cpu().numpy(),
                             "exp_avg_sq": st["exp_avg_sq"].detach().cpu().numpy()}
        return out

    def _load_optimizer_arrays(self, arrays: dict) -> None:
        self.optimizer.state.clear()
        for name, p in self.policy_network.named_parameters():
            if name in arrays:
                a = arrays[name]
                self.optimizer.state[p] = {"step": torch.tensor(float(a["step"])),
                                           "exp_avg": torch.as_tensor(a["exp_avg"]).to(p.device).clone(),
                                           "exp_avg_sq": torch.as_tensor(a["exp_avg_sq"]).to(p.device).clone()}

    def save_checkpoint(self, checkpoint_dir: str, wandb_id, episode_successes: RunningAverage, episode_rewards: RunningAverage,
                        episode_lengths: RunningAverage, eps) -> None:
        self.save_mini_checkpoint(checkpoint_dir=checkpoint_dir, wandb_id=wandb_id)
        ra = lambda r: {"size": r.size, "q": list(r.q), "sum": r.sum}
        sd = lambda m: {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        torch.save({
            "step": self.num_train_steps, "wandb_id": wandb_id, "replay_buffer_pos": [self.replay_buffer.pos[0], 0],
            "policy_net_state_dict": sd(self.policy_network), "target_net_state_dict": sd(self.target_network),
            "optimizer_state_dict": self._optimizer_arrays(), "epsilon": eps.val,
            "episode_successes": ra(episode_successes), "episode_rewards": ra(episode_rewards), "episode_lengths": ra(episode_lengths),
            **{k: ra(getattr(self, k)) for k in _STATS},
            "random_rng_state": random.getstate(), "rng_bit_generator_state": RNG.rng.bit_generator.state,
            "numpy_rng_state": np.random.get_state(), "torch_rng_state": torch.get_rng_state(),
        }, checkpoint_dir + "_checkpoint.pt")
        np.savez(checkpoint_dir + "buffer.npz", **self.replay_buffer.export_arrays())

    def load_checkpoint(self, checkpoint_dir: str) -> Tuple[str, RunningAverage, RunningAverage, RunningAverage, float]:
        ck = torch.load(checkpoint_dir + "_checkpoint.pt", weights_only=False)
        self.num_train_steps = ck["step"]
        self.replay_buffer.pos = list(ck["replay_buffer_pos"])
        self.replay_buffer.import_arrays(dict(np.load(checkpoint_dir + "buffer.npz")))
        as_sd = lambda d: {k: torch.as_tensor(v) for k, v in d.items()}
        self.policy_network.load_state_dict(as_sd(ck["policy_net_state_dict"]))
        self.target_network.load_state_dict(as_sd(ck["target_net_state_dict"]))
        self._load_optimizer_arrays(ck["optimizer_state_dict"])

        def restore(dst: RunningAverage, src: dict) -> RunningAverage:
            dst.size, dst.sum = src["size"], src["sum"]
            dst.q.clear(); dst.q.extend(src["q"])
            return dst
        for k in _STATS:
            restore(getattr(self, k), ck[k])
        random.setstate(ck["random_rng_state"])
        RNG.rng.bit_generator.state = ck["rng_bit_generator_state"]
        np.random.set_state(ck["numpy_rng_state"])
        torch.set_rng_state(ck["torch_rng_state"])
        out = [restore(RunningAverage(10), ck[k]) for k in ("episode_successes", "episode_rewards", "episode_lengths")]
        return ck["wandb_id"], out[0], out[1], out[2], ck["epsilon"]
