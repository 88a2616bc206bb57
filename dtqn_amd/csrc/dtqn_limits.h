// Coverage limits of the per-sequence fused kernels (one workgroup holds a whole context tile
// in LDS).  Anything beyond returns DTQN_ERR_CONFIG from dtqn_net_init.
#pragma once
#include <stddef.h>
#define DTQN_MAX_LP 64          /* padded context rows held in LDS (ctx_len <= 64) */
#define DTQN_MAX_D 128          /* d_model instantiations: 64, 128 (and 16/32 for tests) */
#define DTQN_MAX_HEAD_DIM 128   /* 4 .. 128 in the row-block attention kernels (whole-head tile while it fits LDS, key-blocked beyond: dtqn_attn_whole_tile); the whole-sequence kernels: 8, 16 (and 32: dtqn_ws_lite) */
#define DTQN_MAX_ACTIONS 64
#define DTQN_MAX_BAG 256        /* bag entries dtqn_replay_gather_bag draws from an episode; the attention kernels take a caller's bag of up to the padded context (dtqn_net_init) */
#define DTQN_MAX_DROP_BATCH 1048576   /* sequences per pass of a launch that draws dropout masks: the mask key holds the sequence in 20 bits (dtqn_device.hpp Drop.salt) */
#define DTQN_THREADS 256        /* 4 wave64 per workgroup */
#define DTQN_WAVES 4

// Row-block attention (dtqn_tiled.hip): the whole-tile kernels hold ONE head's rows in LDS -- the forward q | k | v, the backward
// q | k | v | dO plus the lse and delta rows.  A context whose backward tile exceeds 160 KB runs the key-blocked kernels instead
// (tl_attn_kb_*: 64 rows of k | v or q | dO at a time); dtqn_net_init admits those shapes only where the key-blocked kernels are meant to run.
static inline size_t dtqn_attn_tile_lds(int lp, int hd, int bwd) {
    return bwd ? ((size_t)lp * (4 * hd + 4) + 2 * (size_t)lp) * sizeof(float) : (size_t)lp * (3 * hd + 4) * sizeof(float);
}
static inline int dtqn_attn_whole_tile(int lp, int hd) { return dtqn_attn_tile_lds(lp, hd, 1) <= 160 * 1024; }

// Bag attention (dtqn_tiled.hip): the resident kernels (tl_bag_attn_kernel, tl_bag_attn_bwd_kernel) hold the bag's k | v rows of one head
// in LDS and, in the backward, an [n][bag] dS tile beside them (n = 0: the forward's request).  A bag whose backward request at the full
// context exceeds 160 KB runs the matrix-core kernels instead (tl_bag_attn_mfma_*: 64 bag entries or 64 query rows at a time).
static inline size_t dtqn_bag_attn_lds(int n, int bag, int hd) { return ((size_t)2 * bag * hd + (size_t)n * bag) * sizeof(float); }
static inline int dtqn_bag_attn_resident(int ctx, int bag, int hd) { return dtqn_bag_attn_lds(ctx, bag, hd) <= 160 * 1024; }

// Discrete observations (Embedding -> Flatten -> Linear(obs_dim * e, d), representations.py:25-52): what dtqn_net_init admits.  Every
// embedding launch of the row-block path fits the 160 KB of a workgroup inside these bounds at d_model 64 / 128 / 256 (bytes at the bounds,
// d_model 256, the largest):  tl_embed_kernel 132 096 (tl_embed_lds: the [64 + D][68] operand chunks, 64 x obs_dim tokens, the column map
// and a table of at most 2048 floats);  tl_embed_table_kernel 133 120 ([64][D + 4] + [64][132] tiles and the tokens);
// tl_embed_bwd_panel_kernel 132 368 + 256 (action_dim + 1) (dtqn_embed_bwd_panel_lds; dtqn_net_init evaluates it with the network's
// action_dim);  the bag passes are the same kernels with the same requests.
#define DTQN_MAX_OBS_TOKENS 128        /* obs_dim of a discrete observation */
#define DTQN_MAX_EMBED_COLS 1024       /* obs_dim * embed_per_obs: input columns of the embedding linear */
#define DTQN_MAX_TABLE_FLOATS 65536    /* vocab * embed_per_obs: floats of the embedding table */

// Embedding gradient of the row-block path (dtqn_tiled.hip).  The resident kernel (tl_embed_bwd_kernel) keeps d(e_in) of a 64-row block as
// ONE set of matrix-core items (at most 128 gathered columns) and private scatter tables of (row groups) x obs_dim x vocab x e floats in
// LDS; an observation beyond either runs the panel kernel (tl_embed_bwd_panel_kernel), whose LDS does not grow with obs_dim * vocab.
// (constexpr: the kernels lay their LDS out with the same two helpers)
// row groups of a 64-row block walked by different threads of the resident scatter: 4 if the 512 threads allow, else 2 or 1
static constexpr inline int dtqn_embed_bwd_row_groups(int ke) { return ke * 4 <= 512 ? 4 : ke * 2 <= 512 ? 2 : 1; }
// leading dimension of the W_e chunk / d(e_in) tile of ke columns: >= ke rounded up to 16, == 16 mod 64
static constexpr inline int dtqn_embed_bwd_ldk(int ke) { return ((((ke + 15) & ~15) - 16 + 63) / 64) * 64 + 16; }
#define DTQN_EMBED_BWD_PANEL 128       /* gathered columns per panel of the panel kernel */
static inline size_t dtqn_embed_bwd_lds(int discrete, int action_dim, int obs_dim, int vocab, int e) {
    const int ke = obs_dim * e, ldk = dtqn_embed_bwd_ldk(ke);
    size_t f = (size_t)64 * (action_dim + 1) + 64 + 4;                                     // action columns of dx0, actions
    if (discrete)                                                                          // dx0 chunk | W_e chunk | d(e_in) | tokens | tables
        f += (size_t)64 * 68 + (size_t)64 * ldk + (size_t)64 * ldk + (size_t)64 * obs_dim +
             (size_t)dtqn_embed_bwd_row_groups(ke) * obs_dim * vocab * e;
    return f * sizeof(float);
}
static inline int dtqn_embed_bwd_resident(int discrete, int action_dim, int obs_dim, int vocab, int e) {
    if (!discrete) return 1;                                                               // action embedding only: a few KB
    return (long long)obs_dim * e <= 128 && dtqn_embed_bwd_lds(discrete, action_dim, obs_dim, vocab, e) <= 150 * 1024;
}
static inline size_t dtqn_embed_bwd_panel_lds(int action_dim, int obs_dim) {
    const int ldk = dtqn_embed_bwd_ldk(DTQN_EMBED_BWD_PANEL);
    // action columns, actions | dx0 chunk | W_e chunk | d(e_in) of the panel | tokens | first-occurrence rows (one byte each)
    return ((size_t)64 * (action_dim + 1) + 64 + 4 + (size_t)64 * 68 + (size_t)2 * 64 * ldk + (size_t)64 * obs_dim) * sizeof(float) +
           (((size_t)64 * obs_dim + 3) & ~(size_t)3);
}

// The whole-sequence kernels exist as explicit instantiations <d_model, 16-row tiles, head_dim, waves> (dtqn_forward.hip:
// dispatch_fwd, dtqn_backward.hip: td_backward): X(d, mt, hd, nw).  TRAIN = forward and backward exist; the first entry of a
// (d, mt, hd) is the default wave count, the others are reached with DTQN_WAVES (A/B switch).  dtqn_net_init places a network on
// the smallest row-tile count of its (d, hd) that holds the context, and on the row-block tiled path when there is none -- a
// shape it accepts has a kernel behind every launch.
#define DTQN_WS_TRAIN_INSTANCES(X) \
    X(64, 1, 8, 8) X(64, 2, 8, 8) X(64, 4, 8, 8) X(64, 4, 8, 4) X(64, 4, 8, 16) X(64, 4, 16, 8) \
    X(128, 4, 16, 8) X(128, 4, 16, 4) X(16, 1, 8, 4) X(16, 1, 8, 8) X(32, 2, 8, 4) X(32, 1, 16, 4)
// forward only (the actor on a short prefix of the context runs the instantiation with fewer row tiles)
#define DTQN_WS_FWD_ONLY_INSTANCES(X) X(64, 2, 16, 8) X(64, 1, 16, 8) X(128, 2, 16, 8) X(128, 1, 16, 8)

// Smallest instantiated row-tile count >= mt_needed of (d, hd) and its default wave count; 0 if there is none.
static inline int dtqn_ws_pick(int d, int hd, int mt_needed, int* nw_out) {
    int best = 0, nw = 0;
#define DTQN_WS_PICK_(D_, MT_, HD_, NW_) \
    if (d == D_ && hd == HD_ && MT_ >= mt_needed && (best == 0 || MT_ < best)) { best = MT_; nw = NW_; }
    DTQN_WS_TRAIN_INSTANCES(DTQN_WS_PICK_)
#undef DTQN_WS_PICK_
    if (nw_out) *nw_out = nw;
    return best;
}

// "Lite" whole-sequence shapes: d_model 64 (after width padding) with head width 32, or any width-padded network at head width 8 / 16 / 32
// -- residual gate, post-LN, no dropout, context <= 64 rows (dtqn_net_init checks those).  They exist as the weights-through-LDS
// forward (four 16-row slices or one 64-row tile per sequence) and the four-slice backward chain only: acting, inference and the
// latency-mode TD update (dtqn_td_row_split == 4) run there; a TD update at a larger batch runs on the row-block twin
// (dtqn_td_prefers_tiled).  Before round 5 these shapes ran on the row-block kernels throughout (2.8 x slower at batch 32).
static inline int dtqn_ws_lite_shape(int d, int hd, int padded) { return d == 64 && (hd == 32 || (padded && (hd == 8 || hd == 16))); }
static inline int dtqn_ws_lite(int tiled, int d, int hd, int d_real) { return !tiled && dtqn_ws_lite_shape(d, hd, d_real > 0); }
