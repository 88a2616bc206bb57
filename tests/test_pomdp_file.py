"""The `.pomdp` parser (dtqn_amd/envs/pomdp_file.py), the host environment over its model and the registry entries: every accepted form
of T, O, R and `start`, overrides, wildcards, `values: cost`, the `reset` extension, every error with its line number, the size
limits, the CDF rule, the two bundled models.  CPU only."""
import os

import numpy as np
import pytest

from dtqn_amd import envs
from dtqn_amd.envs.pomdp_file import MAX_ACTIONS, MAX_OBSERVATIONS, cdf_rows, load_pomdp

PREAMBLE = "discount: 0.9\nvalues: reward\nstates: a b c\nactions: go stay\nobservations: x y\n"

# one model three ways: matrices, rows, single entries (with wildcards and indices)
MATRIX = PREAMBLE + """start: 0.25 0.75 0.0
T: go
0.0 1.0 0.0
0.0 0.5 0.5
1.0 0.0 0.0
T: stay
identity
O: go
0.9 0.1
0.5 0.5
0.0 1.0
O: stay
uniform
R: go : a
0.0 0.0
1.0 2.0
0.0 0.0
R: go : b
0.0 0.0
0.0 0.0
-1.0 -1.0
"""
ROWS = PREAMBLE + """start:
0.25 0.75 0.0
T: go : a
0.0 1.0 0.0
T: go : b 0.0 0.5 0.5
T: go : c
1.0 0.0 0.0
T: stay : a
1 0 0
T: stay : b
0 1 0
T: stay : c
0 0 1
O: go : a
0.9 0.1
O: go : b
uniform
O: go : c 0.0 1.0
O: stay : * uniform
R: go : a : b
1.0 2.0
R: go : b : c -1.0 -1.0
"""
SINGLE = """# the same model, entry by entry
discount: 0.9
values: reward
states: 3          # a count: the names are 0 1 2
actions: go stay
observations: 2
start: 0.25 0.75 0.0
T: 0 : 0 : 1 1.0     # action by index
T: go : 1 : 1 0.5
T: go : 1 : 2 0.5
T: go : 2 : 0 1.0
T: stay : 0 : 0 1.0
T: stay : 1 : 1 1.0
T: stay : 2 : 2 1.0
O: go : 0 : 0 0.9
O: go : 0 : 1 0.1
O: * : * : * 0.5     # everything uniform ...
O: go : 0 : 0 0.9    # ... and the exceptions again: later entries win
O: go : 0 : 1 0.1
O: go : 2 : 0 0.0
O: go : 2 : 1 1.0
R: go : 0 : 1 : 0 1.0
R: go : 0 : 1 : 1 2.0
R: go : 1 : 2 : * -1.0
"""


def _same(a, b):
    for key in ("start", "T", "O", "R", "D", "start_cdf", "T_cdf", "O_cdf"):
        assert np.array_equal(getattr(a, key), getattr(b, key)), key


def test_the_three_forms_parse_to_the_same_dense_arrays():
    m = load_pomdp(MATRIX)
    assert m.sizes == (3, 2, 2) and m.discount == 0.9 and not m.episodic and not m.D.any()
    assert m.state_names == ["a", "b", "c"] and m.action_names == ["go", "stay"] and m.observation_names == ["x", "y"]
    assert all(t.dtype == np.float64 for t in (m.start, m.T, m.O, m.R)) and m.D.dtype == bool
    assert m.T.shape == (2, 3, 3) and m.O.shape == (2, 3, 2) and m.R.shape == (2, 3, 3, 2) and m.D.shape == (2, 3)
    assert np.array_equal(m.start, [0.25, 0.75, 0.0])
    assert np.array_equal(m.T[0], [[0, 1, 0], [0, 0.5, 0.5], [1, 0, 0]]) and np.array_equal(m.T[1], np.eye(3))
    assert np.array_equal(m.O[0], [[0.9, 0.1], [0.5, 0.5], [0, 1]]) and np.array_equal(m.O[1], np.full((3, 2), 0.5))
    expect = np.zeros((2, 3, 3, 2))
    expect[0, 0, 1], expect[0, 1, 2] = (1.0, 2.0), (-1.0, -1.0)
    assert np.array_equal(m.R, expect)
    _same(m, load_pomdp(ROWS))
    single = load_pomdp(SINGLE)
    assert single.state_names == ["0", "1", "2"] and single.observation_names == ["0", "1"]
    _same(m, single)


def test_a_path_loads_like_its_text(tmp_path):
    path = tmp_path / "m.pomdp"
    path.write_text(MATRIX)
    _same(load_pomdp(MATRIX), load_pomdp(str(path)))


@pytest.mark.parametrize("start,expect", [
    ("start: uniform", [1 / 3, 1 / 3, 1 / 3]), ("", [1 / 3, 1 / 3, 1 / 3]), ("start: b", [0, 1, 0]), ("start: 2", [0, 0, 1]),
    ("start include: a c", [0.5, 0, 0.5]), ("start exclude: a", [0, 0.5, 0.5]), ("start: 0.5 0.5 0.0", [0.5, 0.5, 0])])
def test_start_forms(start, expect):
    m = load_pomdp(PREAMBLE + start + "\nT: * identity\nO: * uniform\n")
    assert np.array_equal(m.start, expect)


def test_overrides_and_wildcards():
    m = load_pomdp(PREAMBLE + """T: * uniform
T: go identity
T: go : b : * 0.0          # a wildcard in the last position: the whole row ...
T: go : b : c 1.0          # ... then one entry of it
T: * : c
0.5 0.5 0.0
O: * : * : x 1.0
O: stay : * : x 0.25
O: stay : * : y 0.75
R: * : * : * : * -1
R: * : a : * : y 3
R: stay : * : b
7 8
""")
    third = np.full(3, 1 / 3)
    assert np.array_equal(m.T[0], [[1, 0, 0], [0, 0, 1], [0.5, 0.5, 0]]) and np.array_equal(m.T[1], [third, third, [0.5, 0.5, 0]])
    assert np.array_equal(m.O[0], [[1, 0]] * 3) and np.array_equal(m.O[1], [[0.25, 0.75]] * 3)
    expect = np.full((2, 3, 3, 2), -1.0)
    expect[:, 0, :, 1] = 3
    expect[1, :, 1] = (7, 8)
    assert np.array_equal(m.R, expect)


def test_values_cost_negates_the_rewards():
    body = "T: * identity\nO: * uniform\nR: go : a : * : * 2\nR: stay : b : b : x -3\n"
    reward, cost = load_pomdp(PREAMBLE + body), load_pomdp(PREAMBLE.replace("values: reward", "values: cost") + body)
    assert reward.R.any() and np.array_equal(cost.R, -reward.R)


def test_reset_pairs_end_the_episode_and_restart_from_the_start_distribution():
    m = load_pomdp(PREAMBLE + "start: 0.25 0.75 0.0\nT: * identity\nT: go : c reset\nT: stay : * reset\nT: stay : a\n0 1 0\nO: * uniform\n")
    assert m.episodic and np.array_equal(m.D, [[False, False, True], [False, True, True]])      # the later row took (a, stay) back
    assert np.array_equal(m.T[0, 2], m.start) and np.array_equal(m.T[1, 1], m.start) and np.array_equal(m.T[1, 2], m.start)
    assert np.array_equal(m.T[1, 0], [0, 1, 0]) and np.array_equal(m.T[0, :2], np.eye(3)[:2])
    env = envs.TabularPOMDP(m)
    env.state = 2
    z, r, done, info = env.step_with(0, 0.5, 0.5)
    assert done and env.state == 1 and z == 1 and r == 0.0 and info == {"is_success": False}


@pytest.mark.parametrize("body,line,what", [
    ("T: * identity\nO: * uniform\nT: go : nowhere : a 1.0\n", 8, "unknown state"),
    ("T: * identity\nO: * uniform\nT: fly identity\n", 8, "unknown action"),
    ("T: * identity\nO: * uniform\nO: go : a : w 1.0\n", 8, "unknown observation"),
    ("T: * identity\nO: * uniform\nR: go : a : 3 : x 1.0\n", 8, "out of range"),
    ("T: * identity\nO: * uniform\nO: 2 uniform\n", 8, "out of range"),
    ("T: * identity\nO: * uniform\n\nT: go : a\n0.5 0.75 -0.25\n", 10, "negative"),
    ("start: 0.5 -0.5 1.0\nT: * identity\nO: * uniform\n", 6, "negative"),
    ("T: * identity\n# a comment line\nT: go : b\n0.5 0.25 0.25001\nO: * uniform\n", 9, "T row"),
    ("T: * identity\nO: * uniform\nO: stay : c : x 0.4\n", 8, "O row"),
    ("start: 0.5 0.25 0.2\nT: * identity\nO: * uniform\n", 6, "start row"),
    ("T: * identity\nO: * uniform\nstart include: a z\n", 8, "unknown state"),
])
def test_errors_carry_their_line_number(body, line, what):
    with pytest.raises(ValueError, match=rf"line {line}\b.*{what}"):
        load_pomdp(PREAMBLE + body)


def test_a_row_sum_within_the_tolerance_is_accepted():
    load_pomdp(PREAMBLE + "T: * identity\nT: go : a\n0.5 0.25 0.2500005\nO: * uniform\n")


def test_size_limits_are_named():
    head = "discount: 1\nvalues: reward\n"
    with pytest.raises(ValueError, match=f"limit of {MAX_ACTIONS}"):
        load_pomdp(head + "states: 2\nactions: 256\nobservations: 2\n")
    with pytest.raises(ValueError, match=f"limit of {MAX_OBSERVATIONS}"):
        load_pomdp(head + "states: 2\nactions: 2\nobservations: 65536\n")
    with pytest.raises(ValueError, match="256 MiB"):                  # 8 * 4 * 300 * 300 * 100 bytes of R alone
        load_pomdp(head + "states: 300\nactions: 4\nobservations: 100\n")
    load_pomdp(head + "states: 2\nactions: 255\nobservations: 2\nT: * identity\nO: * uniform\n")


def test_cdf_properties():
    rng = np.random.default_rng(5)
    p = rng.random((40, 9))
    p[rng.random(p.shape) < 0.4] = 0.0                                # zeros inside, in front and behind
    p[:, 4] += 0.1                                                    # (no all-zero row)
    p[0] = [0, 0, 0, 1, 0, 0, 0, 0, 0]
    p[1, 6:] = 0
    p /= p.sum(axis=1, keepdims=True)
    cdf = cdf_rows(p)
    assert cdf.dtype == np.float64 and (np.diff(cdf, axis=1) >= 0).all() and (cdf[:, -1] == 1.0).all() and (cdf >= 0).all()
    last = p.shape[1] - 1 - np.argmax((p > 0)[:, ::-1], axis=1)
    for row, k in zip(cdf, last):
        assert (row[k:] == 1.0).all() and (row[:k] < 1.0).all()
    u = np.concatenate([[0.0, np.nextafter(1.0, 0.0)], rng.random(9_998)])
    assert len(u) == 10_000 and u.max() < 1.0
    for row_p, row in zip(p, cdf):
        k = np.searchsorted(row, u, side="right")
        assert k.max() < len(row) and (row_p[k] > 0).all()
        assert k[0] == np.argmax(row_p > 0) and k[1] == np.nonzero(row_p)[0][-1]     # u = 0: the first positive entry; u -> 1: the last


@pytest.mark.parametrize("name,sizes,cap", [("tiger", (2, 3, 2), 50), ("corridor", (20, 2, 5), 100)])
def test_bundled_models_load_and_every_row_sums_to_one(name, sizes, cap):
    m = load_pomdp(os.path.join(envs.POMDP_MODELS, name + ".pomdp"))
    assert m.sizes == sizes and m.episodic
    for table in (m.start, m.T, m.O):
        assert np.allclose(table.sum(axis=-1), 1.0, rtol=0, atol=1e-12) and (table >= 0).all()
    env = envs.make(f"POMDP-{name}-episodic-v0")
    assert env._max_episode_steps == cap and env.observation_space.n == sizes[2] and env.action_space.n == sizes[1]
    assert isinstance(env.env, envs.TabularPOMDP) and env.env.model.D.any()
    assert envs.make(f"POMDP-{name}-episodic-v0", max_episode_steps=7)._max_episode_steps == 7
    cont = envs.make(f"POMDP-{name}-v0")
    assert not cont.env.model.D.any() and np.array_equal(cont.env.model.T, m.T)


def test_tiger_and_corridor_are_what_they_say():
    t = load_pomdp(os.path.join(envs.POMDP_MODELS, "tiger.pomdp"))
    assert t.D[0].sum() == 0 and t.D[1:].all() and np.array_equal(t.T[0], np.eye(2)) and np.array_equal(t.O[0], [[0.85, 0.15], [0.15, 0.85]])
    assert (t.R[1, 0] == -100).all() and (t.R[1, 1] == 10).all() and (t.R[2, 0] == 10).all() and (t.R[0] == -1).all()
    c = load_pomdp(os.path.join(envs.POMDP_MODELS, "corridor.pomdp"))
    s = {n: k for k, n in enumerate(c.state_names)}
    assert c.D.sum() == 4 and c.D[0, s["L0"]] and c.D[0, s["R0"]] and c.D[1, s["L9"]] and c.D[1, s["R9"]]
    assert (c.R[0, s["L0"]] == 1).all() and (c.R[0, s["R0"]] == -1).all() and (c.R[1, s["R9"]] == 1).all() and (c.R[1, s["L9"]] == -1).all()
    moves = c.T.copy()                                               # the world only changes through a reset
    moves[c.D] = 0
    assert moves[:, :10, 10:].sum() == 0 and moves[:, 10:, :10].sum() == 0
    # partially observable: away from the ends and the signpost both worlds look alike, and the signpost tells them apart
    z = {n: k for k, n in enumerate(c.observation_names)}
    for cell in (1, 2, 3, 4, 5, 7, 8):
        assert np.array_equal(c.O[:, s[f"L{cell}"]], c.O[:, s[f"R{cell}"]]) and (c.O[:, s[f"L{cell}"], z["corridor"]] == 1).all()
    assert c.O[0, s["L6"], z["sign-left"]] == 0.9 and c.O[0, s["R6"], z["sign-right"]] == 0.9 and c.O[0, s["L6"], z["sign-right"]] == 0


def test_registry_resolves_ids_through_the_path_variable_first(tmp_path, monkeypatch):
    (tmp_path / "mine.pomdp").write_text(MATRIX.replace("T: stay\nidentity", "T: stay\nidentity\nT: stay : c reset"))
    (tmp_path / "tiger.pomdp").write_text(MATRIX)
    with pytest.raises(KeyError, match="mine.pomdp"):
        envs.make("POMDP-mine-episodic-v0", max_episode_steps=9)
    monkeypatch.setenv("DTQN_POMDP_PATH", os.pathsep.join([str(tmp_path / "nowhere"), str(tmp_path)]))
    env = envs.make("POMDP-mine-episodic-v0", max_episode_steps=9)
    assert env._max_episode_steps == 9 and env.observation_space.n == 2 and env.action_space.n == 2
    with pytest.raises(ValueError, match="max-episode-steps"):        # a model of the user's has no registry cap
        envs.make("POMDP-mine-episodic-v0")
    with pytest.raises(ValueError, match="reset"):                    # this tiger.pomdp shadows the bundled one, and has no reset pair
        envs.make("POMDP-tiger-episodic-v0", max_episode_steps=9)
    assert envs.make("POMDP-tiger-v0", max_episode_steps=9).action_space.n == 2
    with pytest.raises(ValueError, match="max-episode-steps"):
        envs.make(str(tmp_path / "mine.pomdp"))
    assert envs.make(str(tmp_path / "mine.pomdp"), max_episode_steps=4)._max_episode_steps == 4


def test_host_environment_draws_follow_the_cdf_rule_and_the_time_limit():
    from dtqn_amd.utils import env_processing
    env = envs.make("POMDP-tiger-episodic-v0")
    env.seed(3)
    assert env_processing.get_env_obs_length(env) == 1 and env_processing.get_env_obs_mask(env) == 2 and env_processing.is_discrete_env(env)
    inner = env.env
    assert inner.reset_with(0.49999, 0.84) == 0 and inner.state == 0 and inner.reset_with(0.5, 0.14) == 0 and inner.state == 1
    assert inner.reset_with(0.5, 0.15) == 1                           # u < cdf[k]: 0.15 is not below the first entry of (0.15, 1.0)
    obs = env.reset()
    assert obs in (0, 1) and inner.state in (0, 1)
    for t in range(50):
        obs, r, done, info = env.step(0)
        assert r == -1.0 and obs in (0, 1) and info["is_success"] is False
    assert done and info["TimeLimit.truncated"] is True
    env.reset()
    s = inner.state
    obs, r, done, info = env.step(2 if s == 0 else 1)                 # the free door
    assert done and r == 10.0 and info["is_success"] is True and "TimeLimit.truncated" not in info
    with pytest.raises(ValueError):
        inner.step_with(3, 0.1, 0.1)
