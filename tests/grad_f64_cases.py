"""Small TD cases that make the groups of the float64 gradient check (grad_f64_helpers.py) bite, shared by tests/test_emu_td.py (CPU
emulation) and tests/test_gpu_td.py (device).  Each names the property of the drawn windows it exists for and asserts it on the first
update's draw, so that a change of the synthetic replay or of a seed cannot quietly turn it into an ordinary case."""
import numpy as np

# name -> (network, run arguments of helpers.make_td_case, records' rows lp)
CASES = {
    # batch 32 on the one-launch weight gradients (live-token contraction, skipped padding steps), records of 16 rows of which 8 are
    # dead (16-row records run one workgroup per sequence: row slices exist for 64-row records only); one window holds a single step of
    # its episode, one is full
    "b32_dead_tokens": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=8),
                        dict(seed=21, batch=32, T=14, n_eps=40, mask=-5, min_len=1), 16),
    # vocabulary rows: one token occurs exactly once in the batch, one never (its row of the table: exactly zero)
    "vocab_groups": (dict(obs_dim=2, num_actions=4, inner_embed_size=64, num_heads=8, num_layers=1, history_len=10, discrete=True, vocab_sizes=9),
                     dict(seed=27, batch=2, T=16, n_eps=6, mask=8), None),
    # loss on the last 3 of 10 rows, learned positions: rows 0 .. 6 of the position table get their gradient through attention only
    "short_history": (dict(obs_dim=3, num_actions=3, inner_embed_size=64, num_heads=8, num_layers=2, history_len=10),
                      dict(seed=21, batch=4, T=16, n_eps=8, mask=-5, history=3), None),
    "short_history_d48": (dict(obs_dim=3, num_actions=3, inner_embed_size=48, num_heads=6, num_layers=2, history_len=10),
                          dict(seed=21, batch=4, T=16, n_eps=8, mask=-5, history=3), None),
    # five actions over four loss rows: at least one row of the head's last layer is exactly zero, next to the padded action columns
    "action_never_taken": (dict(obs_dim=3, num_actions=5, inner_embed_size=64, num_heads=8, num_layers=1, history_len=10),
                           dict(seed=21, batch=2, T=16, n_eps=6, mask=-5, history=2), None),
}


def draw_property(name, cfg, host, history):
    """-> on_batch(it, eps, starts, batch) for helpers.check_td_updates: asserts the case's property on the first update's windows."""
    L = cfg.history_len

    def on_batch(it, eps, starts, batch):
        if it != 0:
            return
        live = np.minimum(host.episode_lengths[eps] - starts, L)          # steps of the window that belong to its episode
        if name == "b32_dead_tokens":
            assert (live == 1).any() and (live == L).any(), live
        elif name == "vocab_groups":
            counts = np.bincount(batch.obss.numpy().reshape(-1), minlength=cfg.vocab_sizes)
            assert (counts == 1).any() and (counts == 0).any(), counts
        elif name.startswith("short_history"):
            assert history == 3 < L and cfg.pos == "learned"
        elif name == "action_never_taken":
            taken = set(batch.actions[:, -history:].reshape(-1).tolist())
            assert len(taken) < cfg.num_actions == 5, taken
    return on_batch
