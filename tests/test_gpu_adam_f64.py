"""-m gpu: clip + Adam and the launches in front of it against a float64 reference, on the device (cases:
tests/adam_f64_cases.py, reference and bounds: tests/adam_f64_helpers.py; CPU-emulation twins: tests/test_emu_adam_f64.py, which also
hold the host-only checks of the bounds themselves)."""
import pytest

import adam_f64_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("k", C.STEP_KS)
def test_step_index(lib, k):
    C.run_step_index(lib, DEV, k)


@pytest.mark.parametrize("k", (1, 2, 1024))
@pytest.mark.parametrize("netname", ("d128", "sin48"))
def test_step_index_wide_and_padded_nets(lib, netname, k):
    C.run_step_index_other_nets(lib, DEV, netname, k)


@pytest.mark.parametrize("regime", sorted(C.REGIMES))
@pytest.mark.parametrize("clip", C.CLIPS)
def test_clip(lib, clip, regime):
    C.run_clip(lib, DEV, "d64", clip, regime)


@pytest.mark.parametrize("regime", ("below", "just_above", "above_1e15"))
def test_clip_with_more_than_256_norm_partials(lib, regime):
    C.run_clip(lib, DEV, "d128", 1.0, regime)


def test_zero_gradient(lib):
    C.run_zero_gradient(lib, DEV)


@pytest.mark.parametrize("clipped", (False, True))
@pytest.mark.parametrize("gs", (1.0, 0.5, 0.125))
def test_grad_scale(lib, gs, clipped):
    C.run_grad_scale(lib, DEV, gs, clipped)


@pytest.mark.parametrize("lr,betas,eps", C.HYPERS)
def test_hyperparameters(lib, lr, betas, eps):
    C.run_hyper(lib, DEV, lr, betas, eps)


@pytest.mark.parametrize("k", (1, 2))
def test_eps_dominated_tiny_gradients(lib, k):
    C.run_tiny(lib, DEV, k)


def test_target_copy(lib):
    C.run_target_copy(lib, DEV)


def test_target_sync_copies_every_float(lib):
    C.run_target_sync(lib, DEV)


def test_prescribed_gradient_trajectory(lib):
    C.run_trajectory(lib, DEV, steps=64)


def test_reduce_kernel(lib):
    C.run_reduce(lib, DEV)


@pytest.mark.parametrize("netname", ("d64", "d128"))
def test_gradnorm_kernel(lib, netname):
    C.run_gradnorm(lib, DEV, netname)


@pytest.mark.parametrize("world", (1, 3, 8))
def test_xreduce_kernel_in_one_process(lib, world):
    C.run_xreduce(lib, DEV, world)
