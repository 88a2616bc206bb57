"""-m gpu: dropout at contexts beyond 256 rows on the device: the cases of tests/dropout_long_cases.py (the same inputs as on the
emulation, test_emu_dropout_long.py), the differentiable forward at 260 rows, and the embedding-site
mask of a row-block net measured on what the forward kernel wrote, rows from 256 up included."""
import numpy as np
import pytest

from oracle import dtqn_oracle as O

from dropout_long_cases import CASES, ENV, assert_trace, run_autograd_case, run_case, show
from helpers import make_td_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from dtqn_amd import engine
    engine.require_gpu()
    return engine.get_lib()


@pytest.mark.parametrize("name", sorted(CASES))
def test_td_update_with_dropout_beyond_256_rows(lib, name, monkeypatch, capfd):
    for k, v in ENV.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    worst = run_case(lib, name, device="cuda", test_lib=False, report_as=f"gpu_dropout_long_{name}")
    assert_trace(name, capfd.readouterr().err)
    show(name, worst)


def test_differentiable_forward_with_dropout_at_260_rows(lib):
    run_autograd_case(None, device="cuda")


def test_embedding_mask_of_a_row_block_net_at_260_rows(lib):
    """test_dropout_keep_rate_scaling_and_eval_mode_on_the_device at L 260 on a row-block net: x0 = dropout(embedding + position) in the
    activation record is 0 for a fraction p of the elements and the undropped value x 1 / (1 - p) for the rest, and the kept set is the
    oracle's rows_keep element for element -- rows 256 .. 259 among the compared ones; the masks of the next optimizer step are
    independent."""
    p, Bn, L, D = 0.3, 4, 260, 64
    kw = dict(obs_dim=3, num_actions=3, inner_embed_size=D, num_heads=4, num_layers=1, history_len=L)
    xs = {}
    for tag, cfg in (("p", O.NetCfg(dropout=p, **kw)), ("0", O.NetCfg(**kw))):
        net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=5, batch=Bn, T=L + 8, n_eps=6, mask=-5, device="cuda", test_lib=False, min_len=L)
        assert eng.net.tiled == 1 and eng.net.lp == 320
        eng.td.dropout_seed = 99
        eng.set_indices(np.arange(Bn, dtype=np.int32), np.zeros(Bn, dtype=np.int32))
        xs[tag] = []
        for step in range(2):
            eng.step_counter[1] = step
            eng.forward_backward(rep)
            act = eng.act.cpu().numpy()[:Bn * eng.net.act_stride].reshape(Bn, eng.net.act_stride)
            off = eng.net.ao_layer0 + eng.net.al_u1     # a post-LN row-block layer reads its input, x0, from u1 of layer 0
            xs[tag].append(act[:, off:off + eng.net.lp * D].reshape(Bn, eng.net.lp, D)[:, :L].copy())
    (xp0, xp1), x00 = xs["p"], xs["0"][0]
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    keep0, keep1 = xp0 != 0, xp1 != 0
    n = keep0.size
    assert abs(keep0.mean() - (1 - p)) < 4 * np.sqrt(p * (1 - p) / n)                 # keep rate
    assert abs(keep0[:, 256:].mean() - (1 - p)) < 4 * np.sqrt(p * (1 - p) / keep0[:, 256:].size)
    assert np.abs(xp0[keep0] - x00[keep0] * scale).max() <= 2e-6 * np.abs(x00).max() # survivors scaled by 1 / (1 - p)
    for b in range(Bn):
        want = O.rows_keep(O.DropSpec(p, 99, 0, 0), b, O.DROP_EMB, 0, np.arange(L), np.arange(D), D)
        assert np.array_equal(keep0[b] | (x00[b] == 0), want | (x00[b] == 0)), b     # the oracle's mask, element for element, rows 0 .. 259
        assert want[256:].size == 4 * D
    rate = p * p + (1 - p) * (1 - p)
    assert abs((keep0 == keep1).mean() - rate) < 4 * np.sqrt(rate * (1 - rate) / n)   # independent masks at the next optimizer step
