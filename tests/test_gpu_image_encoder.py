"""-m gpu: the image encoder's kernels, stand-alone, on the MI355X against torch in float64 -- the cases, groups and exact properties of
test_emu_image_encoder.py (image_encoder_helpers.py, docs/image_encoder_tests.md)."""
import pytest

from image_encoder_helpers import CASES, CaseRun

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.fixture(scope="module")
def runs(lib):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = CaseRun(lib, name, "cuda")
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(CASES))
def test_feature_maps_and_embeddings_on_the_gpu(runs, name):
    runs(name).forward()


@pytest.mark.parametrize("name", list(CASES))
def test_weight_gradients_per_tap_tile_on_the_gpu(runs, name):
    runs(name).gradients()


@pytest.mark.parametrize("name", list(CASES))
def test_backward_exact_properties_on_the_gpu(runs, name):
    runs(name).exact()
