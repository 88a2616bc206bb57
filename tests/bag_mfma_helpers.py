"""Shared by the matrix-core bag attention tests (tests/test_emu_bag_mfma.py on the CPU emulation, tests/test_gpu_bag_mfma.py on the
device): the networks whose resident bag backward does not fit LDS, the launch-trace reader, one TD update under DTQN_BAG_ATTN_MFMA, and
the gradient of the differentiable forward next to TdEngine.forward_backward's."""
import numpy as np
import torch

from oracle import dtqn_oracle as O

from autograd_helpers import make_inputs, make_module
from autograd_dropout_helpers import flat_grad
from helpers import check_td_updates, make_td_case, oracle_batch

LDS_BYTES = 160 * 1024


def resident_bwd_lds(cfg: O.NetCfg) -> int:
    """LDS request of tl_bag_attn_bwd_kernel at the full context (dtqn_limits.h dtqn_bag_attn_lds): k | v of the bag and an [L][bag] dS tile."""
    hd = cfg.inner_embed_size // cfg.num_heads
    return (2 * cfg.bag_size * hd + cfg.history_len * cfg.bag_size) * 4


# Networks dtqn_net_init admits whose resident backward request exceeds a workgroup's 160 KB: (name, NetCfg arguments, seed)
OVERFLOW = [
    ("d128_ctx256_bag160", dict(obs_dim=3, num_actions=4, inner_embed_size=128, num_heads=8, num_layers=1, history_len=256, bag_size=160), 17),
    ("d64_ctx512_bag80", dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=8, num_layers=1, history_len=512, bag_size=80), 17),
    ("gru_identity", dict(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=256, bag_size=176,
                          gate="gru", identity=True), 17),
    ("discrete_action_embedding", dict(obs_dim=5, num_actions=4, inner_embed_size=64, num_heads=8, num_layers=1, history_len=300,
                                       bag_size=136, discrete=True, vocab_sizes=7, action_dim=8), 17),
]

# bags every resident kernel covers: the knob alone decides the family
SMALL = [(ctx, bag, p) for ctx in (20, 100) for bag in (5, 37) for p in (0.0, 0.1)]


def small_cfg(ctx, bag, p):
    return O.NetCfg(obs_dim=3, num_actions=4, inner_embed_size=64, num_heads=4, num_layers=1, history_len=ctx, action_dim=4, bag_size=bag,
                    dropout=p)


def pad_token(cfg: O.NetCfg) -> int:
    """Observation value of the replay's padding rows: a token of the vocabulary on a discrete network (the tables are indexed by it)."""
    return cfg.vocab_sizes - 1 if cfg.discrete else -5


def launched(err: str) -> dict:
    new = [k in err for k in ("tl_bag_attn_mfma_kernel<", "tl_bag_attn_mfma_dkv_kernel<", "tl_bag_attn_mfma_dq_kernel<")]
    old = [k in err for k in ("tl_launch tl_bag_attn_kernel", "tl_launch tl_bag_attn_bwd_kernel")]
    return {"mfma": all(new), "resident": all(old), "mixed": any(new) and any(old)}


def one_update(lib, cfg, knob, monkeypatch, capfd, seed, batch, device="cpu", test_lib=True):
    """One TD update held against the oracle with DTQN_BAG_ATTN_MFMA=knob (None: unset) -> Q of the three forwards, gradient, trace."""
    monkeypatch.setenv("DTQN_TL_TRACE", "1")
    if knob is None:
        monkeypatch.delenv("DTQN_BAG_ATTN_MFMA", raising=False)
    else:
        monkeypatch.setenv("DTQN_BAG_ATTN_MFMA", knob)
    net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=seed, batch=batch, T=cfg.history_len + 8, n_eps=3, mask=pad_token(cfg), device=device,
                                               test_lib=test_lib)
    assert eng.net.tiled == 1
    capfd.readouterr()
    worst = check_td_updates(cfg, net, oracle, host, eng, rep, n_updates=1)
    err = capfd.readouterr().err
    print("bag attention", "knob", knob, "seed", seed, worst)
    return eng.q3.cpu().clone(), eng.grad.cpu().clone(), err


def bag_weights(lib, cfg, seed, batch, n, device="cpu"):
    """attn_weights [B, n, bag] of an eval-mode capturing forward on oracle weights."""
    params = O.init_params(cfg, seed=seed, perturb=True)
    m = make_module(lib if device == "cpu" else None, cfg, params, device=device, autograd=False)
    m.set_capture_attention(True)
    m.eval()
    obs, act, bag, _ = make_inputs(cfg, batch, n, seed=seed + 1)
    with torch.no_grad():
        q = m(torch.as_tensor(obs, device=device), torch.as_tensor(act, device=device),
              bag_obss=torch.as_tensor(bag[0], device=device), bag_actions=torch.as_tensor(bag[1], device=device))
    return q.cpu().numpy(), m.attn_weights.detach().cpu().numpy()


def td_and_autograd_gradients(lib, cfg, seed, batch, device="cpu", test_lib=True):
    """TdEngine.forward_backward's gradient and the gradient loss.backward() leaves on a module with the same weights, fed the same windows,
    bags and the dL/dQ of tl_loss_kernel (y = r + (1 - done) gamma Q_tgt(o')[argmax Q_pol(o')]; dQ[a] = 2 (Q[a] - y) / (B history))."""
    net, oracle, host, eng, rep = make_td_case(lib, cfg, seed=seed, batch=batch, T=cfg.history_len + 8, n_eps=3, mask=pad_token(cfg), device=device,
                                               test_lib=test_lib)
    Bn, L, A, gamma = eng.batch, cfg.history_len, cfg.num_actions, np.float32(0.99)
    eps, starts = host.sample_indices(Bn)
    eng.set_indices(eps, starts)
    rng = np.random.Generator(np.random.PCG64(seed))
    bo = rng.random((Bn, cfg.bag_size, cfg.obs_dim), dtype=np.float32)
    ba = rng.integers(0, cfg.num_actions, (Bn, cfg.bag_size, 1))
    eng.set_bag(bo, ba)
    eng.forward_backward(rep)
    tnet = eng.net
    q3 = torch.from_numpy(eng.q3.cpu().numpy().reshape(3, Bn, tnet.lp, tnet.ap)[:, :, :L, :A].copy())
    batch_ = oracle_batch(host, eps, starts, cfg.discrete)
    m = make_module(lib if device == "cpu" else None, cfg, oracle.pol, device=device)
    assert np.array_equal(m.flat.detach().cpu().numpy(), eng.theta_pol.cpu().numpy())
    dev = lambda x: torch.as_tensor(x, device=device)
    q = m(dev(batch_.obss), dev(batch_.actions), bag_obss=dev(bo), bag_actions=dev(ba))
    with torch.no_grad():
        amax = torch.argmax(q3[1], dim=2, keepdim=True)
        y = batch_.rewards + (1.0 - batch_.dones.float()) * (q3[2].gather(2, amax) * float(gamma))
        diff = q.detach().cpu().gather(2, batch_.actions) - y
        inv_count = np.float32(1.0) / (np.float32(Bn) * np.float32(L))
        dq = torch.zeros(Bn, L, A).scatter_(2, batch_.actions, 2.0 * diff * float(inv_count))
    m.zero_grad(set_to_none=True)
    q.backward(dq.to(q.device))
    return q.detach().cpu().numpy(), q3[0].numpy(), flat_grad(m), eng.grad.cpu().numpy()[:tnet.n_trainable].copy()


def agent_train_run(lib, seed, device="cpu", updates=4):
    """lib: the emulation library (CPU tests) or None (the hipcc-built engine on `device`).  DtqnAgent.train() with the device sampler (windows and bags drawn inside the update) at context 256 / bag 160, on a replay of random
    episodes long enough for the context to evict into the bag -> statistics of every update, parameters after the last."""
    import dtqn_amd.utils.random as rnd
    from dtqn_amd.agents.dtqn import DtqnAgent
    from dtqn_amd.networks.dtqn import DTQN
    name, kw, _ = OVERFLOW[0]
    cfg = O.NetCfg(**kw)
    T, n_eps, Bn = 300, 5, 4
    torch.manual_seed(seed)
    rnd.RNG.rng = np.random.Generator(np.random.PCG64(seed))

    def factory():
        m = DTQN(cfg.obs_dim, cfg.num_actions, cfg.embed_per_obs_dim, cfg.action_dim, cfg.inner_embed_size, cfg.num_heads, cfg.num_layers,
                 cfg.history_len, bag_size=cfg.bag_size, **({"_test_lib": lib} if lib is not None else {}))
        m._allow_cpu = lib is not None
        return m.to(device)
    agent = DtqnAgent(factory, buffer_size=(n_eps + 2) * T, device=torch.device(device), env_obs_length=cfg.obs_dim, max_env_steps=T,
                      obs_mask=-5, num_actions=cfg.num_actions, is_discrete_env=False, batch_size=Bn, context_len=cfg.history_len,
                      history=cfg.history_len, target_update_frequency=3, bag_size=cfg.bag_size, sampler="device", sample_seed=seed)
    rng = np.random.default_rng(seed)
    for _ in range(n_eps):
        n = int(rng.integers(270, T))
        obs = rng.uniform(-1, 1, (n + 1, cfg.obs_dim)).astype(np.float32)
        agent.context_reset(obs[0])
        for t in range(n):
            agent.observe(obs[t + 1], int(rng.integers(0, cfg.num_actions)), float(rng.uniform(-1, 1)), t == n - 1)
        agent.replay_buffer.flush()
    stats = []
    for _ in range(updates):
        agent.train()
        stats.append(agent.engine.read_stats())
    assert agent.num_train_steps == updates
    return stats, agent.policy_network.flat.detach().cpu().numpy().copy()
