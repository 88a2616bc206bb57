"""-m gpu: discrete observations of any admitted width and vocabulary on the MI355X -- the cases of test_emu_wide_discrete.py on the
gfx950 build: the panel embedding-gradient kernel against the oracle, which kernel runs where, the construction bounds, and an agent."""
import pytest
import torch

import wide_discrete_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_td_update_vs_oracle_on_the_panel_kernel(lib, case, monkeypatch, capfd):
    monkeypatch.setenv("DTQN_TL_TRACE", "1")
    W.run_case(lib, case, True, capfd)


@pytest.mark.parametrize("fill", ["same", "two"])
def test_worst_case_collisions_match_the_oracle_and_repeat_bit_for_bit(lib, fill):
    W.run_collisions(lib, fill, gpu=True)


def test_todays_observations_keep_the_resident_kernel(lib, monkeypatch, capfd):
    monkeypatch.setenv("DTQN_TL_TRACE", "1")
    names = W.run_traced(lib, W.TODAY, 2, True, capfd)
    assert W.RESIDENT in names and W.PANEL not in names, sorted(names)


def test_bounds_are_refused_at_construction(lib):
    W.check_construction(lib)


def test_agent_trains_and_acts_on_a_20_token_observation(lib):
    from dtqn_amd.utils.agent_utils import get_agent
    env = W.memory_env(4)
    agent = get_agent("DTQN", [env], 8, 0, 128, 2000, torch.device("cuda"), 3e-4, 4, 70, 70, 70, 1000, 0.99, 8, 1, sampler="device")   # (max_env_steps 70: a replay row holds a whole context)
    W.run_agent(agent, env)
