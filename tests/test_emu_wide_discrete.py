"""Discrete observations of any admitted width and vocabulary on the CPU emulation: the panel embedding-gradient kernel
(tl_embed_bwd_panel_kernel) against the oracle, which kernel runs where, the bounds dtqn_net_init refuses at construction, and an agent on
a 20-token observation."""
import pytest
import torch

from dtqn_amd import _binding as B

import wide_discrete_cases as W


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_td_update_vs_oracle_on_the_panel_kernel(emu, case, monkeypatch, capfd):
    monkeypatch.setenv("DTQN_TL_TRACE", "1")
    W.run_case(emu, case, False, capfd)


@pytest.mark.parametrize("fill", ["same", "two"])
def test_worst_case_collisions_match_the_oracle_and_repeat_bit_for_bit(emu, fill):
    W.run_collisions(emu, fill, gpu=False)


def test_todays_observations_keep_the_resident_kernel(emu, monkeypatch, capfd):
    monkeypatch.setenv("DTQN_TL_TRACE", "1")
    names = W.run_traced(emu, W.TODAY, 2, False, capfd)
    assert W.RESIDENT in names and W.PANEL not in names, sorted(names)


def test_bounds_are_refused_at_construction(emu):
    W.check_construction(emu)


def test_agent_trains_and_acts_on_a_20_token_observation(emu, monkeypatch):
    from dtqn_amd.networks.dtqn import DTQN
    from dtqn_amd.utils import agent_utils

    def on_emulation(*a, **k):
        m = DTQN(*a, _test_lib=emu, **k)
        m._allow_cpu = True
        return m
    monkeypatch.setitem(agent_utils.MODEL_MAP, "DTQN", on_emulation)
    env = W.memory_env(4)
    agent = agent_utils.get_agent("DTQN", [env], 8, 0, 128, 2000, torch.device("cpu"), 3e-4, 4, 70, 70, 70, 1000, 0.99, 8, 1, sampler="device")   # (max_env_steps 70: a replay row holds a whole context)
    W.run_agent(agent, env)
