"""Shared by test_emu_devenv_bits.py, test_gpu_devenv_bits.py and tests/golden/make_devenv_parent_bits.py: one recorded scenario of the
device-resident rollout and evaluation per environment kind, compared byte for byte with what the commit BEFORE the shared
environment layer (csrc/dtqn_devenv.hpp, agents/device_env.py) produced (tests/golden/devenv_parent_bits.npz).

Shapes, those of device_rollout_helpers.py and pomdp_env_helpers.py: N = 3 environments, E = 5 replay slots, context 8, caps 12 (CarFlag,
POMDP) and 6 (Memory, 2 pairs), the whole-sequence network.  The scenario: reset_all, 40 x step_all(epsilon), sync(); then
DeviceEvaluator.evaluate(7, key=3) on the same agent.  epsilon = 0.3 runs the forward (recorded on the emulation only: Q bits differ
between back-ends); epsilon = 1 launches no forward, so its rollout bytes are integer arithmetic, table look-ups and f64, recorded at
the parent on the emulation AND on the MI355X: they agree except in one array, which the fixture holds once per back-end."""
import os

import numpy as np

import device_eval_helpers as E
import device_rollout_helpers as R
import pomdp_env_helpers as P

KINDS = ("car", "mem", "pomdp")
EPSILONS = {"eps03": 0.3, "eps1": 1.0}
STEPS, EPISODES, KEY = 40, 7, 3
ROLLOUT_KEYS = ("rollout_state", "rollout_status", "replay_obs", "replay_actions", "replay_rewards", "replay_dones", "replay_ep_len")
EVAL_KEYS = ("eval_state", "eval_status", "eval_triple")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "devenv_parent_bits.npz")


def run_scenario(lib, device, kind, epsilon, with_eval=True):
    """-> {name: array} of the scenario for one kind; lib: the emulation library (agent on the CPU) or None."""
    if kind == "pomdp":
        agent = P.make_agent(lib, device)
        actor = P.make_actor(agent)
    else:
        agent = R.make_agent(lib, device, kind)
        actor = R.make_actor(agent, kind)
    actor.reset_all()
    for _ in range(STEPS):
        actor.step_all(epsilon)
    actor.sync()
    out = {"rollout_state": actor.get_state().raw.copy(), "rollout_status": actor._status_np.copy()}
    out.update({"replay_" + k: v for k, v in R.replay_arrays(agent.replay_buffer).items()})
    if with_eval:
        ev = P.make_evaluator(agent) if kind == "pomdp" else E.make_evaluator(agent, kind)
        triple = ev.evaluate(EPISODES, key=KEY)
        out.update(eval_state=ev.get_state().raw.copy(), eval_status=ev._status_np.copy(), eval_triple=np.asarray(triple, dtype=np.float64))
    return out


def check_against_fixture(lib, device, eps_name, names):
    """Every array in `names` of the scenario `eps_name`, for the three kinds, byte-equal to the recorded one: the parent's on this
    back-end ("gpu/<key>" where the MI355X recording differed from the emulation's; make_devenv_parent_bits.py names the one array)."""
    z = np.load(FIXTURE)
    for kind in KINDS:
        got = run_scenario(lib, device, kind, EPSILONS[eps_name], with_eval=any(n in EVAL_KEYS for n in names))
        for name in names:
            key = f"{kind}/{eps_name}/{name}"
            want = z["gpu/" + key] if device != "cpu" and "gpu/" + key in z.files else z[key]
            assert got[name].dtype == want.dtype and got[name].shape == want.shape, (kind, eps_name, name, got[name].dtype, got[name].shape)
            assert got[name].tobytes() == want.tobytes(), (kind, eps_name, name)


def nan_argmax_case(lib, device, k=1):
    """ffn.2.bias[k] = NaN makes Q[:, k] NaN in every row: one greedy step on CarFlag takes action k in every environment (a NaN
    counts as the maximum, as torch.argmax has it)."""
    import torch
    agent = R.make_agent(lib, device, "car")
    sd = {n: v.clone() for n, v in agent.policy_network.state_dict().items()}
    sd["ffn.2.bias"][k] = float("nan")
    agent.policy_network.load_state_dict(sd)
    agent.target_update()
    actor = R.make_actor(agent, "car")
    actor.reset_all()
    actor.step_all(0.0)
    actor.sync()
    st = actor.get_state()
    q = actor.q_rows()
    assert np.isnan(q[:, k]).all() and np.isfinite(np.delete(q, k, axis=1)).all(), q
    assert (st.last[:, 0] == k).all() and (st.last[:, 1] == 0).all(), st.last
    assert torch.equal(torch.argmax(torch.from_numpy(q), dim=1), torch.full((R.N,), k))
