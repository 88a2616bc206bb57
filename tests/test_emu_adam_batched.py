"""The batched-load optimizer kernel on the CPU kernel emulation (cases: tests/adam_batched_cases.py; -m gpu twins:
tests/test_gpu_adam_batched.py)."""
import pytest

from dtqn_amd import _binding as B

import adam_batched_cases as C


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.mark.parametrize("name", sorted(C.ORACLE_CASES))
def test_update_matches_the_oracle(emu, name):
    C.run_oracle_case(emu, "cpu", name)


def test_nan_in_grad_skips_the_update_and_the_next_call_reports_3(emu):
    C.run_nan_grad_case(emu, "cpu")


def test_exchange_status_word_zero_applies_and_one_refuses(emu):
    C.run_xstatus_case(emu, "cpu")


def test_ring_slots_carry_the_statistics_of_their_call(emu):
    C.run_ring_case(emu, "cpu")
