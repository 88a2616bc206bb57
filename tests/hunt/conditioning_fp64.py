"""Why the dropout hunt reports the GRU + identity, d_model 128, two-layer family: the fp32 ORACLE evaluated against itself in fp64 is as far away
(7e-4 .. 1e-3 at |Q| 12) as the engine is from either -- conditioning of that family under the std-0.2 stress weights, not an engine error.
`python tests/hunt/conditioning_fp64.py`"""
# Is the gru + identity + D=128 + 2 layers + dropout family ill-conditioned, or is the engine wrong?  Evaluate the ORACLE itself in fp64
# (oracle.td_gradients64: the same parameters, inputs and keep masks, every operation in double) and in fp32 on the failing case: if
# fp32-oracle vs fp64-oracle differ by as much as engine vs fp32-oracle, it is conditioning.  The gradients get the same treatment, group by
# group (grad_f64_helpers.py): D32 is the fp32 oracle's own distance from float64, the last column the engine's in units of it.
import sys
import os
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import numpy as np
from dtqn_amd import _binding as B
from emu import emu_build
from oracle import dtqn_oracle as O
from grad_f64_helpers import check_gradient_f64
from helpers import make_td_case, oracle_batch, engine_probe
emu = B.load_library(emu_build.build())
kw = {'obs_dim': 2, 'num_actions': 6, 'inner_embed_size': 128, 'num_heads': 8, 'num_layers': 2, 'history_len': 70, 'gate': 'gru', 'identity': True, 'pos': 'sin', 'action_dim': 8, 'dropout': 0.3}
cfg = O.NetCfg(**kw)
# regenerate the same case as the hunt did is not possible (rng state); use a fresh seed and several batches
for seed in range(6):
    net, oracle, host, eng, rep = make_td_case(emu, cfg, seed=seed, batch=2, T=84, n_eps=5, mask=-5, history=55, tuf=10000)
    eps, starts = host.sample_indices(2)
    batch = oracle_batch(host, eps, starts, cfg.discrete)
    eng.set_indices(eps, starts)
    eng.forward_backward(rep)
    L, A = cfg.history_len, cfg.num_actions
    q3 = eng.q3.cpu().numpy().reshape(3, 2, eng.net.lp, eng.net.ap)[:, :, :L, :A]
    probe = engine_probe(cfg, eng.net, eng)
    drop = O.DropSpec(cfg.dropout, int(eng.td.dropout_seed), 0)
    args = (oracle.pol, oracle.tgt, cfg, batch, oracle.gamma, oracle.history)
    g32, out32 = O.td_gradients(*args, dict(probe, masks=list(probe["masks"])), drop)
    g64, out64 = O.td_gradients64(*args, dict(probe, masks=list(probe["masks"])), drop)
    e_o = max(float((out32[4 + w].detach().double() - out64[4 + w].detach()).abs().max()) for w in range(3))
    e_e = max(float(np.abs(q3[w] - out32[4 + w].detach().numpy()).max()) for w in range(3))
    e_e64 = max(float(np.abs(q3[w] - out64[4 + w].detach().numpy()).max()) for w in range(3))
    qmax = float(out32[4].detach().abs().max())
    fig = check_gradient_f64(cfg, eng.net, eng.grad.cpu().numpy(), g64, g32, assert_=False)
    print(f"seed {seed}: |Q|max {qmax:.2f}  engine vs fp32 oracle {e_e:.2e}   fp32 oracle vs fp64 oracle {e_o:.2e}   engine vs fp64 oracle {e_e64:.2e}"
          f"   gradient groups: D32 {fig['d32']:.2e} ({fig['d32_group']}), engine / D32 {fig['over_d32']:.2f} ({fig['group']})")
