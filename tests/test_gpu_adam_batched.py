"""-m gpu: the batched-load optimizer kernel on the device (cases: tests/adam_batched_cases.py; CPU-emulation twins:
tests/test_emu_adam_batched.py)."""
import pytest

import adam_batched_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("name", sorted(C.ORACLE_CASES))
def test_update_matches_the_oracle(lib, name):
    C.run_oracle_case(lib, "cuda", name)


def test_nan_in_grad_skips_the_update_and_the_next_call_reports_3(lib):
    C.run_nan_grad_case(lib, "cuda")


def test_exchange_status_word_zero_applies_and_one_refuses(lib):
    C.run_xstatus_case(lib, "cuda")


def test_ring_slots_carry_the_statistics_of_their_call(lib):
    C.run_ring_case(lib, "cuda")
