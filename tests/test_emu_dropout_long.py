"""Dropout at contexts beyond 256 rows on the CPU emulation: the cases of tests/dropout_long_cases.py (one TD update each under the
oracle's keep masks, with the float64 gradient, Q and statistics checks), and the differentiable forward at 260 rows.  The device runs
the same cases in test_gpu_dropout_long.py."""
import pytest

from dtqn_amd import _binding as B

from dropout_long_cases import CASES, ENV, assert_trace, run_autograd_case, run_case, show


@pytest.fixture(scope="module")
def emu():
    from emu import emu_build
    return B.load_library(emu_build.build())


@pytest.mark.parametrize("name", sorted(CASES))
def test_td_update_with_dropout_beyond_256_rows(emu, name, monkeypatch, capfd):
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    worst = run_case(emu, name)
    assert_trace(name, capfd.readouterr().err)
    show(name, worst)


def test_differentiable_forward_with_dropout_at_260_rows(emu):
    run_autograd_case(emu)


def test_a_batch_beyond_the_keys_sequence_field_is_refused(emu):
    """The mask key holds the sequence in 20 bits below the pass: the launch layer refuses a mask-drawing launch of more sequences per
    pass than that (DTQN_MAX_DROP_BATCH, the oracle's DROP_MAX_BATCH), in front of every launch.  Every other argument of the calls
    below is one the entry point accepts, so the refusal is the bound's."""
    import ctypes
    import numpy as np
    from oracle import dtqn_oracle as O
    from helpers import net_from_cfg, ptr
    assert B._LIMITS["DTQN_MAX_DROP_BATCH"] == O.DROP_MAX_BATCH == 1 << 20
    cfg = O.NetCfg(**CASES["whole_tile_h16"][0])
    net = net_from_cfg(emu, cfg)
    x = np.zeros(16, np.float32)
    nb, big = ctypes.byref(net), O.DROP_MAX_BATCH + 1
    ERR_ARG = B.DEFINES["DTQN_ERR_ARG"]
    assert emu.dtqn_forward_train_drop(nb, ptr(x), ptr(x), None, None, None, big, 1, ptr(x), ptr(x), 1, 0, None) == ERR_ARG
    assert emu.dtqn_backward_dq_drop(nb, ptr(x), ptr(x), None, None, None, big, 1, ptr(x), ptr(x), ptr(x), None, 1, 0, None) == ERR_ARG
    # the TD entry points: every check in front of the bound passes (a replay of the net's width, a valid history), nothing is launched
    from dtqn_amd.learner import TdEngine
    eng = TdEngine(net, 2, _test_lib=emu)
    eng.td.batch = big
    rp = B.DtqnReplay()
    rp.obs_dim, rp.max_steps = cfg.obs_dim, cfg.history_len + 8
    assert emu.dtqn_td_forward(nb, ctypes.byref(rp), ctypes.byref(eng.td), None) == ERR_ARG
    assert emu.dtqn_td_backward(nb, ctypes.byref(rp), ctypes.byref(eng.td), None) == ERR_ARG
