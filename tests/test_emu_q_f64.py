"""The forward edge cases of tests/q_f64_cases.py on the CPU emulation: every row of Q within margin * D32 of the oracle's float64
forward (q_f64_helpers.py), at stress and at init-scale weights.  The device runs the same cases in test_gpu_q_f64.py."""
import numpy as np
import pytest

from dtqn_amd import _binding as B

from q_f64_cases import CASES, ENV, SCALES, assert_trace, run_case
from q_f64_helpers import check_q_f64


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_edges_against_float64(emu, name, scale, monkeypatch, capfd):
    for k, v in ENV.get(name, {}).items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    run_case(emu, name, scale)
    assert_trace(name, capfd.readouterr().err)


def test_the_check_itself():
    """check_q_f64 on made-up rows: a quiet row next to a loud one is held at the floor of its own sequence, not at the loud sequence's
    scale; an error of 1e-3 of a row fails; a float32 reference is refused."""
    rng = np.random.default_rng(0)
    q64 = rng.standard_normal((2, 6, 4))
    q64[1] *= 1e3                                   # a loud sequence
    q64[0, 2] *= 1e-3                               # a quiet row: held at the floor 2^-4 of sequence 0
    q32 = q64.astype(np.float32)
    fig = check_q_f64(q32, q64, q32)
    assert fig["over_d32"] <= 1.0 and fig["d32"] <= 2.0 ** -23
    bad = q32.copy()
    bad[0, 1, 0] *= 1.0 + 1e-3
    with pytest.raises(AssertionError, match="beyond margin"):
        check_q_f64(bad, q64, q32)
    bad = q32.copy()
    bad[0, 2, 0] += 1e-3 * np.abs(q64[0]).max() * 2.0 ** -4          # 1e-3 of the floor of sequence 0, far below the loud sequence's scale
    with pytest.raises(AssertionError, match="beyond margin"):
        check_q_f64(bad, q64, q32)
    with pytest.raises(AssertionError, match="not float64"):
        check_q_f64(q32, q32, q32)
    bad = q32.copy()
    bad[1, 0, 0] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        check_q_f64(bad, q64, q32)
    rows = np.ones((2, 6), dtype=bool)
    rows[1, 0] = False
    check_q_f64(bad, q64, q32, rows=rows)           # a row that is not compared may hold anything
