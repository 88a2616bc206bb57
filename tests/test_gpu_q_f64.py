"""-m gpu: the forward edge cases of tests/q_f64_cases.py on the device (the same inputs as on the emulation: test_emu_q_f64.py), every
row of Q within margin * D32 of the oracle's float64 forward.  The worst figures of every case go to the parity report."""
import pytest

from helpers import parity_report
from q_f64_cases import CASES, ENV, SCALES, assert_trace, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_edges_against_float64(lib, name, scale, monkeypatch, capfd):
    for k, v in ENV.get(name, {}).items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    figs = run_case(lib, name, scale, device="cuda")
    assert_trace(name, capfd.readouterr().err)
    worst = max(figs, key=lambda f: f["over_bound"])
    parity_report(f"gpu_q64_{name}_scale{scale}", {"q64_over_bound": worst["over_bound"], "q64_over_d32": worst["over_d32"], "q64_d32": worst["d32"],
                                                   "q64_row": worst["row"], "q64_n": worst["n"], "q64_checks": len(figs),
                                                   "q64_abs_bound": max(f["abs_bound"] for f in figs), "q_abs_max": max(f["q_abs_max"] for f in figs)})
