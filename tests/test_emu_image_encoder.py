"""The image encoder's kernels, stand-alone, on the test-only HIP emulation against torch in float64: every layer's feature map, every
embedding row, every per-tap tile of the weight gradients (image_encoder_helpers.py, docs/image_encoder_tests.md).  The same cases run
on the MI355X in test_gpu_image_encoder.py."""
import pytest

from dtqn_amd import _binding as B

from image_encoder_helpers import CASES, CaseRun

@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.fixture(scope="module")
def runs(emu):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = CaseRun(emu, name, "cpu")
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_feature_maps_and_embeddings_on_the_emulation(runs, name):
    runs(name).forward()


@pytest.mark.parametrize("name", list(CASES))
def test_weight_gradients_per_tap_tile_on_the_emulation(runs, name):
    runs(name).gradients()


@pytest.mark.parametrize("name", list(CASES))
def test_backward_exact_properties_on_the_emulation(runs, name):
    runs(name).exact()
