"""Cases of the batched-load optimizer kernel (dtqn_clip_adam_kernel), shared by the CPU-emulation tests (test_emu_adam_batched.py) and
their -m gpu twins (test_gpu_adam_batched.py): one case per load path of the kernel -- the first trip of the norm-partial and the
statistics loops inside the batch, their remainder loops, the stand-in address behind a NULL xstatus, the skipped update.
Updates are compared with OracleLearner through helpers.check_td_updates at its own tolerances (Adam step, statistics)."""
import numpy as np
import torch

from helpers import make_td_case, check_td_updates
from oracle import dtqn_oracle as O

CFG1 = dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=50)

# (network, case, what the optimizer launch must look like: statistics records, norm partials against the 256 threads of a block)
ORACLE_CASES = {
    "two_records_partial_last_block": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=8),
                                       dict(batch=2, T=12, n_eps=10, mask=-5), dict(updates=1, row_split=1, stat_parts=2, partial_last_block=True)),
    "cfg1_batch32_three_updates_tuf2": (CFG1, dict(batch=32, T=200, n_eps=40, mask=-5, tuf=2), dict(updates=3, row_split=4, stat_parts=128)),
    "stat_parts_remainder_loop": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=8),
                                  dict(batch=300, T=12, n_eps=40, mask=-5), dict(updates=1, stat_parts_over=256)),
    "norm_parts_remainder_loop": (dict(obs_dim=3, num_actions=3, inner_embed_size=128, num_heads=8, num_layers=2, history_len=8),
                                  dict(batch=2, T=12, n_eps=10, mask=-5), dict(updates=1, norm_parts_over=256)),
}


def _make(lib, device, netkw, casekw, seed=11):
    cfg = O.NetCfg(**netkw)
    kw = dict(casekw)
    gpu = device != "cpu"
    return (cfg,) + make_td_case(lib, cfg, seed=seed, device=device, test_lib=not gpu, **kw)


def run_oracle_case(lib, device, name):
    netkw, casekw, want = ORACLE_CASES[name]
    cfg, net, oracle, host, eng, rep = _make(lib, device, netkw, casekw)
    n_stat = eng.batch * max(1, eng.row_split)
    n_norm = int(eng.norm_partial.numel())
    if "row_split" in want:
        assert eng.row_split == want["row_split"]
    if "stat_parts" in want:
        assert n_stat == want["stat_parts"]
    if "stat_parts_over" in want:
        assert n_stat > want["stat_parts_over"]
    if "norm_parts_over" in want:
        assert int(lib.dtqn_td_norm_partials(eng._net_ref)) > want["norm_parts_over"] and n_norm > want["norm_parts_over"]
    if want.get("partial_last_block"):
        assert eng.net.n_trainable % 1024 != 0
    check_td_updates(cfg, net, oracle, host, eng, rep, want["updates"])
    if want["updates"] == 3:                                    # bias corrections at k = 1, 2, 3; target copy on step 2 (checked inside)
        assert int(eng.step_counter[1]) == 3 and int(eng.step_counter[2]) == 3


def _cfg1_engine(lib, device):
    cfg, net, oracle, host, eng, rep = _make(lib, device, CFG1, dict(batch=32, T=200, n_eps=40, mask=-5))
    eng.set_indices(*host.sample_indices(eng.batch))
    return eng, rep


def _snap(eng):
    return [t.clone() for t in (eng.theta_pol, eng.theta_tgt, eng.adam_m, eng.adam_v)]


def run_nan_grad_case(lib, device):
    """NaN written into grad (a value in a buffer): stats[11] = 1, nothing written, the next call reports 3."""
    eng, rep = _cfg1_engine(lib, device)
    eng.forward_backward(rep)
    eng.clip_adam()                                             # one good step first: the counters are not all zero
    assert eng.read_stats()["nonfinite"] == 0.0 and int(eng.step_counter[1]) == 1
    eng.forward_backward(rep)
    eng.grad[5] = float("nan")
    eng.recompute_gradnorm()                                    # the norm partials follow the poisoned gradient
    before, sc_before = _snap(eng), eng.step_counter.clone()
    eng.clip_adam()
    st = eng.read_stats()
    assert st["nonfinite"] == 1.0 and st["step"] == 2.0 and st["target_synced"] == 0.0 and not np.isfinite(st["grad_norm"])
    for a, b in zip(before, _snap(eng)):
        assert torch.equal(a, b), "a skipped update modified parameters or optimizer state"
    sc = eng.step_counter.cpu().numpy()
    assert sc[0] == int(sc_before[0]) and sc[1] == 1 and sc[2] == 3 - 1 and sc[3] == 1
    eng.forward_backward(rep)                                   # a clean gradient again: the flag is sticky
    eng.clip_adam()
    assert eng.read_stats()["nonfinite"] == 3.0 and int(eng.step_counter[1]) == 1 and int(eng.step_counter[2]) == 3
    for a, b in zip(before, _snap(eng)):
        assert torch.equal(a, b)


def run_xstatus_case(lib, device):
    """A non-NULL exchange status holding 0 (applied), then 1 (stats[11] = 2, nothing written): the address the NULL case replaces
    by its stand-in, both ways."""
    eng, rep = _cfg1_engine(lib, device)
    status = torch.zeros(1, dtype=torch.int32, device=eng.device)
    eng.td.xstatus = status.data_ptr()
    eng.forward_backward(rep)
    before = _snap(eng)
    eng.clip_adam()
    st = eng.read_stats()
    assert st["nonfinite"] == 0.0 and st["step"] == 1.0 and int(eng.step_counter[1]) == 1 and int(eng.step_counter[3]) == 0
    assert not torch.equal(before[0], eng.theta_pol) and not torch.equal(before[2], eng.adam_m)
    status.fill_(1)
    eng.forward_backward(rep)
    before = _snap(eng)
    eng.clip_adam()
    st = eng.read_stats()
    assert st["nonfinite"] == 2.0 and st["step"] == 2.0 and int(eng.step_counter[1]) == 1 and int(eng.step_counter[3]) == 1
    for a, b in zip(before, _snap(eng)):
        assert torch.equal(a, b), "a refused exchange sum modified parameters or optimizer state"
    eng.td.xstatus = None


def run_ring_case(lib, device):
    """Three calls: slots 0 .. 2 of the host ring carry twelve granules {value, tag = call index}, values = stats[] of that call."""
    eng, rep = _cfg1_engine(lib, device)
    stats = []
    for _ in range(3):
        eng.forward_backward(rep)
        eng.clip_adam()
        stats.append(eng.stats.detach().cpu().numpy().copy())  # (blocking: the kernel is done, its ring stores have landed)
    ring = eng.stats_ring_np
    for call in (1, 2, 3):
        slot = ring[call - 1]
        assert slot.shape == (12, 2)
        assert (slot[:, 1] == np.float32(call)).all(), (call, slot[:, 1])
        assert np.array_equal(slot[:, 0].view(np.uint32), stats[call - 1].view(np.uint32)), (call, slot[:, 0], stats[call - 1])
    assert stats[2][9] == 3.0 and not ring[3].any()
