"""The device sampler on the CPU emulation, every draw equal to oracle/sampler_oracle.py (sampler_helpers.py, inputs in
sampler_cases.py).  The device runs the same cases in test_gpu_sampler.py; the oracle's distribution is tested in
test_sampler_reference.py."""
import pytest

from dtqn_amd import _binding as B

import sampler_cases as C
import sampler_helpers as H


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.mark.parametrize("batch", C.BATCHES)
def test_window_draw_grid(emu, batch):
    assert H.run_window_grid(emu, "cpu", batch) == len(C.EXCLUDES) * len(C.SEEDS) * (len(C.STEPS) + len(H.edge_steps()))


def test_window_draw_small_rings(emu):
    H.run_window_small_rings(emu, "cpu")


def test_window_draw_edge_keys(emu):
    H.run_window_edge_keys(emu, "cpu")


def test_window_draw_step_counter(emu):
    H.run_window_step_counter(emu, "cpu")


def test_window_draw_refusals(emu):
    H.run_window_refusals(emu, "cpu")


@pytest.mark.parametrize("bag", C.BAGS)
@pytest.mark.parametrize("kind", ["float", "discrete"])
def test_bags(emu, kind, bag):
    H.run_bags(emu, "cpu", kind, bag)


def test_bags_collision_keys(emu):
    H.run_bags_collision_keys(emu, "cpu")


def test_bags_of_max_size(emu):
    H.run_bags_max(emu, "cpu")


def test_bags_refusals(emu):
    H.run_bags_refusals(emu, "cpu")


@pytest.mark.parametrize("kind", ["float", "discrete"])
def test_bags_from_host_rows(emu, kind):
    H.run_bags_host_rows(emu, "cpu", kind)


@pytest.mark.parametrize("split", ["0", "1", "4", "tiled"])
def test_draw_inside_the_update(emu, split, monkeypatch):
    if split == "tiled":
        monkeypatch.setenv("DTQN_FORCE_TILED", "1")
    else:
        monkeypatch.setenv("DTQN_ROW_SPLIT", split)
    H.run_update_draw(emu, "cpu", split)


def test_draw_of_the_pipelined_update_and_of_the_pass_ahead(emu):
    H.run_pipelined_draw(emu, "cpu")


def test_bags_of_a_training_agent(emu):
    H.run_bag_agent_draw(emu, "cpu")
