"""Bag attention on the matrix core (tl_bag_attn_mfma_*) on the device: the networks whose resident bag backward does not fit LDS against
the oracle, a pipelined DtqnAgent.train() run on one of them, the forced kernels against the resident ones under dropout, and
dtqn_forward_bag on a partial context.  Bounds as in tests/test_emu_bag_mfma.py."""
import numpy as np
import pytest
import torch

from oracle import dtqn_oracle as O

from q_f64_helpers import check_forward_f64
from bag_mfma_helpers import LDS_BYTES, OVERFLOW, agent_train_run, bag_weights, launched, one_update, resident_bwd_lds, small_cfg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("name,kw,seed", OVERFLOW, ids=[c[0] for c in OVERFLOW])
def test_td_update_beyond_the_resident_tile_vs_oracle(lib, name, kw, seed, monkeypatch, capfd):
    cfg = O.NetCfg(**kw)
    assert resident_bwd_lds(cfg) > LDS_BYTES
    _, _, err = one_update(lib, cfg, None, monkeypatch, capfd, seed=seed, batch=4, device="cuda", test_lib=False)
    assert launched(err) == {"mfma": True, "resident": False, "mixed": False}


@pytest.mark.parametrize("ctx,bag", [(20, 5), (100, 37)])
def test_forced_matrix_core_kernels_match_the_resident_ones_under_dropout(lib, ctx, bag, monkeypatch, capfd):
    cfg = small_cfg(ctx, bag, 0.1)
    q0, g0, err0 = one_update(lib, cfg, "0", monkeypatch, capfd, seed=29, batch=4, device="cuda", test_lib=False)
    q1, g1, err1 = one_update(lib, cfg, "1", monkeypatch, capfd, seed=29, batch=4, device="cuda", test_lib=False)
    assert launched(err0) == {"mfma": False, "resident": True, "mixed": False}
    assert launched(err1) == {"mfma": True, "resident": False, "mixed": False}
    dq, dg = float(torch.abs(q1 - q0).max()), float(torch.abs(g1 - g0).max())
    print("old vs new", ctx, bag, "dQ", dq, "|Q|max", float(torch.abs(q0).max()), "dg", dg, "|g|max", float(torch.abs(g0).max()))
    assert dq <= 1e-4 * max(1.0, float(torch.abs(q0).max()))
    assert dg <= 2e-4 * float(torch.abs(g0).max())
    monkeypatch.setenv("DTQN_BAG_ATTN_MFMA", "0")
    _, wa = bag_weights(lib, cfg, seed=7, batch=2, n=ctx, device="cuda")
    monkeypatch.setenv("DTQN_BAG_ATTN_MFMA", "1")
    _, wb = bag_weights(lib, cfg, seed=7, batch=2, n=ctx, device="cuda")
    assert np.abs(wa - wb).max() <= 1e-5 and np.abs(wb.sum(-1) - 1.0).max() <= 1e-5


def test_forward_bag_on_a_partial_context(lib):
    """dtqn_forward_bag (the no-grad module forward of a bag network) on 100 of 256 rows, against the oracle's forward."""
    from autograd_helpers import make_inputs, make_module
    name, kw, seed = OVERFLOW[0]
    cfg = O.NetCfg(**kw)
    params = O.init_params(cfg, seed=seed, perturb=True)
    m = make_module(None, cfg, params, device="cuda", autograd=False)
    m.eval()
    obs, act, bag, _ = make_inputs(cfg, 3, 100, seed=5)
    with torch.no_grad():
        q = m(torch.as_tensor(obs, device="cuda"), torch.as_tensor(act, device="cuda"),
              bag_obss=torch.as_tensor(bag[0], device="cuda"), bag_actions=torch.as_tensor(bag[1], device="cuda")).cpu().numpy()
        q_ref = O.forward(params, cfg, torch.as_tensor(obs), torch.as_tensor(act), bag_obss=torch.as_tensor(bag[0]),
                          bag_actions=torch.as_tensor(bag[1])).numpy()
    assert q.shape == q_ref.shape == (3, 100, cfg.num_actions)
    qmax = float(np.abs(q_ref).max())
    print("forward_bag partial context: err", float(np.abs(q - q_ref).max()), "|Q|max", qmax)
    assert np.abs(q - q_ref).max() <= 1e-4 * max(1.0, qmax)
    check_forward_f64(cfg, params, obs, act, q, bag=bag, what="forward_bag on a partial context")


def test_agent_train_beyond_the_resident_tile_is_finite_and_deterministic(lib, monkeypatch, capfd):
    monkeypatch.setenv("DTQN_TL_TRACE", "1")
    sa, ta = agent_train_run(None, 11, device="cuda")
    assert launched(capfd.readouterr().err) == {"mfma": True, "resident": False, "mixed": False}
    monkeypatch.delenv("DTQN_TL_TRACE")
    sb, tb = agent_train_run(None, 11, device="cuda")
    for st in sa:
        assert st["nonfinite"] == 0.0 and all(np.isfinite(v) for v in st.values()), st
        assert st["td_error"] > 0 and st["grad_norm"] > 0
    assert sa[-1]["step"] == 4
    assert np.isfinite(ta).all() and np.array_equal(ta, tb)
    assert sa == sb
