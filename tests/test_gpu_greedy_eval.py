"""-m gpu: greedy evaluation with idle environments on the MI355X -- dtqn_actor_greedy_batch, dtqn_img_actor_greedy_batch, VectorEvaluator
and `run.py --eval-envs N` (greedy_eval_helpers.py; the same checks run on the HIP emulation in test_greedy_eval.py)."""
import pytest

import greedy_eval_helpers as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.fixture
def stream():
    from dtqn_amd import engine
    return engine.stream_ptr()


@pytest.mark.parametrize("kw", [G.WHOLE, G.ROWBLOCK], ids=["whole-sequence", "row-block"])
def test_greedy_entry_equals_the_batch_entry_on_the_live_subset(lib, stream, kw):
    G.check_entry_parity(lib, kw, device="cuda", stream=stream)


def test_greedy_entry_argument_checks(lib, stream):
    G.check_argument_errors(lib, device="cuda", stream=stream)


@pytest.mark.parametrize("kw", [G.WHOLE, G.ROWBLOCK], ids=["whole-sequence", "row-block"])
def test_ties_go_to_the_first_maximum(lib, stream, kw):
    G.check_ties(lib, kw, device="cuda", stream=stream)


def test_image_evaluation_encodes_every_frame_once_and_leaves_idle_rows_alone(lib):
    G.check_image_evaluation(None, "cuda")


@pytest.mark.parametrize("env_id,shape,base,limits", G.EVALUATOR_CASES, ids=["carflag-whole-sequence", "memory-row-block"])
def test_evaluator_against_the_sequential_loop(lib, env_id, shape, base, limits):
    G.check_evaluator_against_the_sequential_loop(None, "cuda", env_id, shape, base, limits=limits)


def test_bag_evaluator_batched_equals_one_at_a_time(lib):
    G.check_bag_evaluator(None, "cuda")


def test_eval_envs_1_takes_the_single_environment_function(lib, monkeypatch, tmp_path):
    G.check_run_py_plumbing(None, "cuda", monkeypatch, tmp_path)
