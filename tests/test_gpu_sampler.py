"""-m gpu: the device sampler on the device, every draw equal to oracle/sampler_oracle.py -- the cases of test_emu_sampler.py
(sampler_helpers.py, inputs in sampler_cases.py) through the hipcc-built engine."""
import pytest

import sampler_cases as C
import sampler_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("batch", C.BATCHES)
def test_window_draw_grid(lib, batch):
    assert H.run_window_grid(lib, DEV, batch) == len(C.EXCLUDES) * len(C.SEEDS) * (len(C.STEPS) + len(H.edge_steps()))


def test_window_draw_small_rings(lib):
    H.run_window_small_rings(lib, DEV)


def test_window_draw_edge_keys(lib):
    H.run_window_edge_keys(lib, DEV)


def test_window_draw_step_counter(lib):
    H.run_window_step_counter(lib, DEV)


def test_window_draw_refusals(lib):
    H.run_window_refusals(lib, DEV)


@pytest.mark.parametrize("bag", C.BAGS)
@pytest.mark.parametrize("kind", ["float", "discrete"])
def test_bags(lib, kind, bag):
    H.run_bags(lib, DEV, kind, bag)


def test_bags_collision_keys(lib):
    H.run_bags_collision_keys(lib, DEV)


def test_bags_of_max_size(lib):
    H.run_bags_max(lib, DEV)


def test_bags_refusals(lib):
    H.run_bags_refusals(lib, DEV)


@pytest.mark.parametrize("kind", ["float", "discrete"])
def test_bags_from_host_rows(lib, kind):
    H.run_bags_host_rows(lib, DEV, kind)


@pytest.mark.parametrize("split", ["0", "1", "4", "tiled"])
def test_draw_inside_the_update(lib, split, monkeypatch):
    if split == "tiled":
        monkeypatch.setenv("DTQN_FORCE_TILED", "1")
    else:
        monkeypatch.setenv("DTQN_ROW_SPLIT", split)
    H.run_update_draw(lib, DEV, split)


def test_draw_of_the_pipelined_update_and_of_the_pass_ahead(lib):
    H.run_pipelined_draw(lib, DEV)


def test_bags_of_a_training_agent(lib):
    H.run_bag_agent_draw(None, DEV)
