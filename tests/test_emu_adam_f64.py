"""Clip + Adam and the launches in front of it against a float64 reference, on the CPU kernel emulation (cases:
tests/adam_f64_cases.py, reference and bounds: tests/adam_f64_helpers.py; -m gpu twins: tests/test_gpu_adam_f64.py)."""
import numpy as np
import pytest
import torch

from dtqn_amd import _binding as B

import adam_f64_cases as C
import adam_f64_helpers as H

DEV = "cpu"


@pytest.fixture(scope="module")
def lib():
    from emu import emu_build
    return B.load_library(emu_build.build())


def test_bounds_hold_for_an_independent_f32_restatement_on_the_host():
    """Before anything is asked of a kernel: plain-numpy f32 Adam stays inside every bound against R32h, for the inputs of every case."""
    worst = C.run_host_restatement()
    C._report("host_restatement", {k: max(v.values()) for k, v in worst.items()})


def test_reference_halves_are_clip_grad_norm():
    """get_total_norm + clip_grads_with_norm_, as the reference calls them, is clip_grad_norm_."""
    g = torch.from_numpy(H.synth_inputs(4096, 1)["g"].astype(np.float64)) * 3.0
    p = torch.nn.Parameter(torch.zeros(4096, dtype=torch.float64))
    p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_([p], 1.0, error_if_nonfinite=True)
    assert float(total) == H.ref_norm(g.numpy(), 1.0)
    assert torch.equal(p.grad, g * H.clip_factor(float(total), 1.0))


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
