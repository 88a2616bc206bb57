"""Greedy evaluation with idle environments on the test-only HIP emulation: the entry points dtqn_actor_greedy_batch and
dtqn_img_actor_greedy_batch, VectorEvaluator, and `run.py --eval-envs N` (greedy_eval_helpers.py; the MI355X runs the same checks in
test_gpu_greedy_eval.py)."""
import numpy as np
import pytest

from dtqn_amd import _binding as B

import greedy_eval_helpers as G
import image_vector_helpers as IV


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.mark.parametrize("kw", [G.WHOLE, G.ROWBLOCK], ids=["whole-sequence", "row-block"])
def test_greedy_entry_equals_the_batch_entry_on_the_live_subset(emu, kw):
    G.check_entry_parity(emu, kw)


def test_greedy_entry_argument_checks(emu):
    G.check_argument_errors(emu)


@pytest.mark.parametrize("kw", [G.WHOLE, G.ROWBLOCK], ids=["whole-sequence", "row-block"])
def test_ties_go_to_the_first_maximum(emu, kw):
    G.check_ties(emu, kw)


def test_image_evaluation_encodes_every_frame_once_and_leaves_idle_rows_alone(emu):
    G.check_image_evaluation(emu, "cpu")


@pytest.mark.parametrize("env_id,shape,base,limits", G.EVALUATOR_CASES, ids=["carflag-whole-sequence", "memory-row-block"])
def test_evaluator_against_the_sequential_loop(emu, env_id, shape, base, limits):
    G.check_evaluator_against_the_sequential_loop(emu, "cpu", env_id, shape, base, limits=limits)


def test_bag_evaluator_batched_equals_one_at_a_time(emu):
    G.check_bag_evaluator(emu, "cpu")


def test_eval_envs_1_takes_the_single_environment_function(emu, monkeypatch, tmp_path):
    G.check_run_py_plumbing(emu, "cpu", monkeypatch, tmp_path)
