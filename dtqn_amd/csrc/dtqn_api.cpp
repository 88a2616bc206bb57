// Entry points that only sequence other entry points (no device code of their own).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "dtqn_actor.hpp"
#include "dtqn_deval.hpp"
#include "dtqn_devbag.hpp"
#include "dtqn_hip.h"
#include "dtqn_limits.h"
#include "dtqn_rollout.hpp"

extern "C" const char* dtqn_build_info(void) {
#ifdef DTQN_BUILD_INFO
    return DTQN_BUILD_INFO;
#else
    return "dtqn_hip (unstamped build)";
#endif
}

static void* g_profile_buffer = nullptr;
extern "C" int dtqn_debug_set_profile_buffer(void* dev_buffer) {
    g_profile_buffer = dev_buffer;
    return DTQN_OK;
}
extern "C" void* dtqn_debug_profile_buffer(void) { return g_profile_buffer; }

// Latency mode (two workgroups per sequence): only where it pays and is covered -- the whole-sequence kernels with a
// 64-row context tile, residual gate, post-LN, and few enough sequences that every workgroup is resident at once.
// compute units the residency rules below are written against: the device's own count (256 on an MI355X; fewer on a partition)
static int policy_cus() {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 256;
    return n;
}
extern "C" int dtqn_td_row_split(const DtqnNet* net, int batch) {
    if (!net || batch < 1) return 1;
    const int cus = policy_cus();
    const char* e = getenv("DTQN_ROW_SPLIT");                 // tests / tuning: 0 = never, 1 = whenever covered
    if (e != nullptr && e[0] == '0') return 1;
    const bool covered = !net->tiled && net->lp == 64 && !net->identity &&
                         (net->d_model == 64 || (net->d_model == 128 && net->gate == DTQN_GATE_RES));   // GRU: D <= 64
    if (!covered) return 1;
    if (e != nullptr && e[0] == '1') return 2;
    if (e != nullptr && e[0] == '4') return 4;
    // 256 CUs: all 3*B*2 forward (and B*4 backward) workgroups resident at once.  The value is the number of row slices
    // of the BACKWARD kernel (4 x 16 rows); the forward kernel never uses more than two (2 x 32 rows).
    if (3 * batch * 2 <= cus) return 4;
    // Beyond latency mode (round 5) the forward runs one workgroup per sequence, and the backward chain -- half / a quarter as long per
    // slice -- is still sliced while all its workgroups fit the chip at once.  Measured at config-1 shapes (TD-updates/s, whole |
    // sliced backward; profiles/r05_row_split_policy.txt): batch 48 5 559 | 8 136 (four slices), 64 5 450 | 7 883 (four), 96 4 405 |
    // 5 378 (two; four: 4 878), 128 4 245 | 5 142 (two; four: 4 683); at 192 / 256 (a round and a half / two rounds of two-slice
    // workgroups) 0.98 / 0.99 x, so BASELINE config 2 stays whole-sequence.  d_model 64 (both gates); d_model 128 was not measured.
    if (net->d_model == 64) {
        if (batch * 4 <= cus) return 4;
        if (batch * 2 <= cus) return 2;
    }
    return 1;
}
// 1: the TD update of `batch` sequences runs in latency mode -- sliced forward passes as well (two 32-row slices in the one-call update,
// four 16-row slices in the pipelined one, dtqn_td_fwd_slices4_ok) and, pipelined, the next update's target pass inside the backward
// launch.  0 with dtqn_td_row_split > 1: only the backward is sliced.
extern "C" int dtqn_td_latency_mode(const DtqnNet* net, int batch) {
    if (dtqn_td_row_split(net, batch) < 2) return 0;
    const char* e = getenv("DTQN_ROW_SPLIT");                 // forced slices (tests / tuning) are forced in both kernels:
    if (e != nullptr && (e[0] == '1' || e[0] == '4')) return 1;   // the two values dtqn_td_row_split treats as forced, nothing else
    return 3 * batch * 2 <= policy_cus() ? 1 : 0;
}
// Both kernel families cover D = 128 / residual gate / post-LN / 64-row contexts.  Measured at BASELINE config 3 shapes (updates/s,
// whole-sequence | row-block): B = 64 1681 | 1880, B = 128 1244 | 1391, B = 256 895 | 863, B = 512 459 | 499 -- the row-block
// kernels win wherever latency mode is out of reach, except around B = 256 (a round and a half of workgroups in several of their
// launches).  D = 64 stays whole-sequence (cfg 2: 2898 | 1697).
extern "C" int dtqn_td_prefers_tiled(const DtqnNet* net, int batch) {
    if (!net || batch < 1 || net->tiled) return 0;
    // head width 32 / width-padded networks on the whole-sequence side (dtqn_limits.h, dtqn_ws_lite) train there in latency mode only
    if (dtqn_ws_lite(net->tiled, net->d_model, net->head_dim, net->d_real))
        return dtqn_td_row_split(net, batch) == 4 && dtqn_td_latency_mode(net, batch) ? 0 : 1;
    const bool covered = net->d_model == 128 && net->gate == DTQN_GATE_RES && !net->identity && net->lp == 64 && net->dropout == 0.f &&
                         net->bag_size == 0;
    if (!covered) return 0;
    const char* e = getenv("DTQN_TRAIN_TILED");
    if (e != nullptr) return atoi(e) != 0 ? 1 : 0;
    return dtqn_td_row_split(net, batch) == 1 ? 1 : 0;
}
extern "C" int dtqn_td_xch_floats(const DtqnNet* net, int batch) {
    if (!net || batch < 1) return 0;
    // K | V (or dK | dV) hand-over records per (sequence of the three passes, layer): two slices send lp / 2 rows, four slices
    // 3 lp / 4 (dtqn_forward_body.hpp kv_xch_floats)
    return 3 * batch * net->num_layers * (3 * net->lp / 4) * 2 * net->d_model;
}
extern "C" int dtqn_td_xch_flags(const DtqnNet* net, int batch) {
    if (!net || batch < 1) return 0;
    // backward: one per 64-column head group (<= 4); + the event counters of the fused weight gradients (dtqn_wgrad_direct.hpp: kFuseWords)
    // forward with four slices: six (sender, receiver) pairs per (sequence, layer)
    return 3 * batch * net->num_layers * 6 + 16;
}

// DtqnAgent.train() after sampling (dtqn/agents/dtqn.py:215-269) on one GPU: five launches.
extern "C" int dtqn_td_update(const DtqnNet* net, const DtqnReplay* rp, const DtqnTd* td, void* stream) {
    int rc;
    if ((rc = dtqn_td_forward(net, rp, td, stream)) != DTQN_OK) return rc;
    if ((rc = dtqn_td_backward(net, rp, td, stream)) != DTQN_OK) return rc;
    if ((rc = dtqn_td_wgrad(net, td, stream)) != DTQN_OK) return rc;
    if ((rc = dtqn_td_reduce(net, td, stream)) != DTQN_OK) return rc;
    return dtqn_td_clip_adam(net, td, stream);
}

// The pipelined form of the same update (latency mode, dtqn_td_fwd_slices4_ok): the two policy passes as four row slices, the
// target pass inline unless the previous update's backward launch already carried it (have_target), the backward launch carrying the
// NEXT update's target pass when td_next is given, weight gradients, reduce, clip + Adam.  draw_step: the optimizer step this
// update carries (key of its window draw); the next update's is draw_step + 1.
extern "C" int dtqn_td_gradients_pipelined(const DtqnNet* net, const DtqnReplay* rp, const DtqnTd* td, const DtqnTd* td_next, int have_target,
                                           int draw_step, void* stream) {
    int rc;
    if (draw_step < 0) return DTQN_ERR_ARG;
    if ((rc = dtqn_td_forward_part(net, rp, td, 0, 2, 4, draw_step, stream)) != DTQN_OK) return rc;
    if (!have_target && (rc = dtqn_td_forward_part(net, rp, td, 2, 1, 4, draw_step, stream)) != DTQN_OK) return rc;
    rc = td_next != nullptr ? dtqn_td_backward_ahead(net, rp, td, td_next, draw_step + 1, stream) : dtqn_td_backward(net, rp, td, stream);
    if (rc != DTQN_OK) return rc;
    if ((rc = dtqn_td_wgrad(net, td, stream)) != DTQN_OK) return rc;
    return dtqn_td_reduce(net, td, stream);
}
extern "C" int dtqn_td_update_pipelined(const DtqnNet* net, const DtqnReplay* rp, const DtqnTd* td, const DtqnTd* td_next, int have_target,
                                        int draw_step, void* stream) {
    const int rc = dtqn_td_gradients_pipelined(net, rp, td, td_next, have_target, draw_step, stream);
    return rc != DTQN_OK ? rc : dtqn_td_clip_adam(net, td, stream);
}

// Rollout staging (north_star: "pinned hipMemcpyAsync into the device buffer").  Every HIP API call costs the host
// loop microseconds, so a step of the actor loop is one library call each, with as few runtime calls inside as possible:
//  * the producer's scatter kernel reads its records and observation rows straight out of the PINNED host staging
//    (device-mapped memory, a few dozen bytes per step): no copy is enqueued at all;
//  * the actor's context goes over with one hipMemcpyAsync (it is re-read by every lane of the embedding stage, so it
//    has to be in device memory), and the Q-values of the last row come back by the forward kernel writing them into
//    pinned host memory itself.
namespace dtqn {
int forward_infer(const DtqnNet* net, const float* theta, const float* obs, const uint8_t* actions, int batch, int n,
                  float* q_out, float* q_last_host, void* stream, float* xch, int32_t* xflags, const int32_t* last_rows, int in_rows,
                  uint32_t drop_seed, uint32_t drop_step, int train_mode);
int tiled_forward_actor(const DtqnNet* net, const float* theta, const float* obs, const uint8_t* actions, int batch, int n, int in_rows,
                        float* q_out, float* workspace, int train_mode, uint32_t drop_seed, uint32_t drop_step, hipStream_t stream, const int32_t* lens = nullptr);
}
extern "C" int dtqn_forward_tiled_strided(const DtqnNet* net, const float* theta, const float* obs, const uint8_t* actions,
                                          int batch, int n, int in_rows, float* q_out, float* workspace, void* stream);

extern "C" int dtqn_replay_push(const DtqnReplay* rp, const DtqnReplayRecord* recs_host, const float* obs_host, int n,
                                void* stream) {
    if (!rp || n < 0) return DTQN_ERR_ARG;
    if (n == 0) return DTQN_OK;
    if (!recs_host || !obs_host) return DTQN_ERR_ARG;
    return dtqn_replay_apply(rp, recs_host, obs_host, n, stream);
}

extern "C" int dtqn_actor_forward(const DtqnNet* net, const float* theta, const void* ctx_host, void* ctx_dev, int n,
                                  float* q_dev, float* q_last_host, float* workspace, int train_mode, uint32_t dropout_seed,
                                  uint32_t dropout_step, void* stream) {
    if (!net || !theta || !ctx_host || !ctx_dev || !q_dev || !q_last_host) return DTQN_ERR_ARG;
    if (n < 1 || n > net->ctx_len) return DTQN_ERR_ARG;                 // dtqn.py:170-173
    hipStream_t s = (hipStream_t)stream;
    const size_t obs_bytes = sizeof(float) * (size_t)net->ctx_len * net->obs_dim;
    if (hipMemcpyAsync(ctx_dev, ctx_host, obs_bytes + (size_t)net->ctx_len, hipMemcpyHostToDevice, s) != hipSuccess) return DTQN_ERR_LAUNCH;
    const float* obs = static_cast<const float*>(ctx_dev);
    const uint8_t* actions = static_cast<const uint8_t*>(ctx_dev) + obs_bytes;
    if (!net->tiled) {
        // batch 1 is the extreme of the small-batch regime: two workgroups for the one sequence once its upper half has
        // live rows (workspace = [hand-over tiles | flags], zeroed once by the caller)
        const bool split = workspace != nullptr && n > net->lp / 2 && dtqn_td_row_split(net, 1) >= 2;
        float* xch = split ? workspace : nullptr;
        int32_t* xflags = split ? reinterpret_cast<int32_t*>(workspace + dtqn_td_xch_floats(net, 1)) : nullptr;
        return dtqn::forward_infer(net, theta, obs, actions, 1, n, q_dev, q_last_host, stream, xch, xflags, nullptr, 0, dropout_seed, dropout_step, train_mode);
    }
    const int rc = dtqn::tiled_forward_actor(net, theta, obs, actions, 1, n, n, q_dev, workspace, train_mode, dropout_seed, dropout_step, s);
    if (rc != DTQN_OK) return rc;
    if (hipMemcpyAsync(q_last_host, q_dev + (size_t)(n - 1) * net->num_actions, sizeof(float) * net->num_actions,
                       hipMemcpyDeviceToHost, s) != hipSuccess)
        return DTQN_ERR_LAUNCH;
    return DTQN_OK;
}

// The forward both batched actor entry points run on the packed block (dtqn_actor.hpp)
using dtqn::ActorBlock, dtqn::actor_block;
// batch: sequences in the block (its first `batch` slots); ws_envs: the batch `workspace` was laid out for (>= batch).  Row-block nets
// leave Q in q_dev only; the whole-sequence kernels also write row len_s - 1 of sequence s to q_last_host[s] when that is given.
static int actor_batch_forward(const DtqnNet* net, const float* theta, const ActorBlock& b, int batch, int ws_envs, int n_max, float* q_dev,
                               float* q_last_host, float* workspace, int train_mode, uint32_t dropout_seed, uint32_t dropout_step,
                               void* stream) {
    const int L = net->ctx_len;
    if (net->tiled)
        return dtqn::tiled_forward_actor(net, theta, b.obs, b.actions, batch, n_max, L, q_dev, workspace, train_mode, dropout_seed,
                                         dropout_step, (hipStream_t)stream, b.lens);
    // few actors: two workgroups per sequence once the longest prefix reaches the upper half (workspace = hand-over tiles | flags)
    const bool split = workspace != nullptr && n_max > net->lp / 2 && dtqn_td_row_split(net, batch) >= 2;
    float* xch = split ? workspace : nullptr;
    int32_t* xflags = split ? reinterpret_cast<int32_t*>(workspace + dtqn_td_xch_floats(net, ws_envs)) : nullptr;
    return dtqn::forward_infer(net, theta, b.obs, b.actions, batch, n_max, q_dev, q_last_host, stream, xch, xflags, b.lens, L, dropout_seed,
                               dropout_step, train_mode);
}

// The same for N actors at once (vectorised rollout: N host environments per learner, one launch per vector step).
// ctx_host is PINNED: [N][ctx_len * obs_dim f32] observations | [N][ctx_len u8] actions | [N] int32 live rows n_i (1..ctx_len),
// copied to ctx_dev (same layout) in ONE hipMemcpyAsync.  Every sequence runs n_max = max n_i rows -- attention is causal, so
// the rows behind a shorter prefix cannot reach its last live row -- and Q of row n_i - 1 of sequence i lands in the pinned
// q_last_host[i][num_actions], written by the kernel (valid once `stream` has drained).  q_dev: [N][n_max][num_actions].
// workspace as dtqn_actor_forward with batch N: dtqn_forward_workspace_floats(net, N) floats, zeroed once.
extern "C" int dtqn_actor_forward_batch(const DtqnNet* net, const float* theta, const void* ctx_host, void* ctx_dev, int n_envs,
                                        int n_max, float* q_dev, float* q_last_host, float* workspace, int train_mode,
                                        uint32_t dropout_seed, uint32_t dropout_step, void* stream) {
    if (!net || !theta || !ctx_host || !ctx_dev || !q_dev || !q_last_host || n_envs < 1) return DTQN_ERR_ARG;
    if (n_max < 1 || n_max > net->ctx_len) return DTQN_ERR_ARG;                 // dtqn.py:170-173
    hipStream_t s = (hipStream_t)stream;
    // the live-row counts index q_dev (tiled path) and name the rows the kernel reports (whole-sequence path): the pinned host
    // copy is already written, so a bad count is refused here instead of becoming an out-of-bounds device access
    const ActorBlock h = actor_block(net, ctx_host, n_envs);
    for (int i = 0; i < n_envs; ++i)
        if (h.lens[i] < 1 || h.lens[i] > n_max) return DTQN_ERR_ARG;
    if (hipMemcpyAsync(ctx_dev, ctx_host, h.bytes, hipMemcpyHostToDevice, s) != hipSuccess) return DTQN_ERR_LAUNCH;
    const ActorBlock b = actor_block(net, ctx_dev, n_envs);
    const int rc = actor_batch_forward(net, theta, b, n_envs, n_envs, n_max, q_dev, q_last_host, workspace, train_mode, dropout_seed,
                                       dropout_step, stream);
    if (rc != DTQN_OK || !net->tiled) return rc;
    // row-block tiled nets: the forward leaves Q in q_dev; the last rows come back with one small copy per actor
    for (int i = 0; i < n_envs; ++i)
        if (hipMemcpyAsync(q_last_host + (size_t)i * net->num_actions, q_dev + ((size_t)i * n_max + (h.lens[i] - 1)) * net->num_actions,
                           sizeof(float) * net->num_actions, hipMemcpyDeviceToHost, s) != hipSuccess)
            return DTQN_ERR_LAUNCH;
    return DTQN_OK;
}

// Greedy evaluation on the same block (run.py:187-243 plays its evaluation episodes one forward per step): len_i == 0 marks
// environment i as idle.  The len block the caller staged is the one source of which environments are live: the host counts them
// here, the compaction kernel reads the same numbers in place, nothing is read back.  Compaction (pinned block -> sequences
// 0 .. live - 1 of ctx_dev, environment order), the forward of dtqn_actor_forward_batch over `live` sequences, then one kernel that
// writes Q of row len_i - 1 and its arg-max for every environment (-1 for an idle one) into pinned memory.
extern "C" int dtqn_actor_greedy_batch(const DtqnNet* net, const float* theta, const void* ctx_host, void* ctx_dev, int n_envs,
                                       int n_max, float* q_dev, float* q_last_host, int32_t* action_host, float* workspace,
                                       int train_mode, uint32_t dropout_seed, uint32_t dropout_step, void* stream) {
    if (!net || !theta || !ctx_host || !ctx_dev || !q_dev || !q_last_host || !action_host || n_envs < 1) return DTQN_ERR_ARG;
    if (n_max < 0 || n_max > net->ctx_len) return DTQN_ERR_ARG;                 // dtqn.py:170-173
    const ActorBlock h = actor_block(net, ctx_host, n_envs);
    int live = 0;
    for (int i = 0; i < n_envs; ++i) {
        if (h.lens[i] < 0 || h.lens[i] > n_max) return DTQN_ERR_ARG;
        live += h.lens[i] > 0 ? 1 : 0;
    }
    dtqn::set_last_actor_live(live);
    if (live == 0) {                      // nothing to launch: the answer is host memory, written here
        for (int i = 0; i < n_envs; ++i) action_host[i] = -1;
        return DTQN_OK;
    }
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = dtqn::actor_compact(net, ctx_host, ctx_dev, n_envs, n_max, s)) != DTQN_OK) return rc;
    const ActorBlock b = actor_block(net, ctx_dev, n_envs);
    // (the kernel's own pinned Q rows would land at the sequence's index, not the environment's: the rows are taken from q_dev)
    if ((rc = actor_batch_forward(net, theta, b, live, n_envs, n_max, q_dev, nullptr, workspace, train_mode, dropout_seed, dropout_step,
                                  stream)) != DTQN_OK)
        return rc;
    return dtqn::actor_greedy_rows(h.lens, q_dev, q_last_host, action_host, n_envs, n_max, net->num_actions, s);
}

// The forward of dtqn_actor_forward_batch on a context block that lives in a device-resident state (`block`: its byte offset in
// d->state; d: DtqnRollout or DtqnEval, the same field names) -- no host copy, the ragged lengths are read on the device.
template <class Desc>
static int resident_forward(const DtqnNet* net, const float* theta, const Desc* d, size_t block, int n_max, int train_mode, uint32_t dropout_seed,
                            uint32_t dropout_step, void* stream) {
    if (!theta || !d->q_dev || (!net->tiled && !d->q_last)) return DTQN_ERR_ARG;
    if (n_max < 1 || n_max > net->ctx_len) return DTQN_ERR_ARG;                 // dtqn.py:170-173
    const ActorBlock b = actor_block(net, static_cast<uint8_t*>(d->state) + block, d->n_envs);
    return actor_batch_forward(net, theta, b, d->n_envs, d->n_envs, n_max, d->q_dev, d->q_last, d->workspace, train_mode, dropout_seed, dropout_step,
                               stream);
}

// Device-resident rollout (dtqn_rollout.hip): that forward on the block that holds the contexts, then the one-workgroup step kernel.
// Two launches, nothing between.
extern "C" int dtqn_rollout_step(const DtqnNet* net, const float* theta, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, int cur,
                                 int n_max, float epsilon, int store, long long authorize, int run_forward, int train_mode, uint32_t dropout_seed,
                                 uint32_t dropout_step, void* stream) {
    int rc = dtqn::rollout_check(net, rp, ro);
    if (rc != DTQN_OK) return rc;
    if (cur != 0 && cur != 1) return DTQN_ERR_ARG;
    if (run_forward) {
        rc = resident_forward(net, theta, ro, dtqn::rollout_layout(net, rp, ro).off[6 + cur], n_max, train_mode, dropout_seed, dropout_step, stream);
        if (rc != DTQN_OK) return rc;
    }
    return dtqn::rollout_step_launch(net, rp, ro, vstep, cur, n_max, epsilon, store, authorize, run_forward ? 1 : 0, (hipStream_t)stream);
}

// The rollout's and the bag descriptor's checks for the bag entry points: DTQN_ERR_CONFIG for a network without a bag.
static int rollout_bag_check(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, const DtqnDevBag* bag) {
    if (!bag) return DTQN_ERR_ARG;
    const int rc = dtqn::rollout_check_bags(net, rp, ro);
    return rc != DTQN_OK ? rc : dtqn::devbag_check(net, ro, bag);
}

extern "C" int dtqn_rollout_reset_bag(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, const DtqnDevBag* bag, uint32_t vstep,
                                      void* stream) {
    int rc = rollout_bag_check(net, rp, ro, bag);
    if (rc != DTQN_OK) return rc;
    if ((rc = dtqn::rollout_reset_launch(net, rp, ro, vstep, (hipStream_t)stream)) != DTQN_OK) return rc;
    return dtqn::devbag_stage_launch(net, rp, ro, bag, 0, 1, 0, (hipStream_t)stream);
}

// Device-resident rollout of a bag network (dtqn_devbag.hip): up to five launches, nothing between -- the actor forward with the bags,
// the rollout's step kernel, the bags' bookkeeping, and where a choice can be due the candidate forward and the selection.
extern "C" int dtqn_rollout_step_bag(const DtqnNet* net, const float* theta, const DtqnReplay* rp, const DtqnRollout* ro, const DtqnDevBag* bag,
                                     uint32_t vstep, int cur, int n_max, float epsilon, int store, long long authorize, int run_forward,
                                     int train_mode, uint32_t dropout_seed, uint32_t dropout_step, int may_choose, void* stream) {
    int rc = rollout_bag_check(net, rp, ro, bag);
    if (rc != DTQN_OK) return rc;
    if (cur != 0 && cur != 1) return DTQN_ERR_ARG;
    if (!theta || !ro->q_dev) return DTQN_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const dtqn::RolloutLayout l = dtqn::rollout_layout(net, rp, ro);
    const dtqn::DevBagViews v = dtqn::devbag_views(net, bag);
    const int N = ro->n_envs, L = net->ctx_len;
    if (run_forward) {
        if (n_max < 1 || n_max > L) return DTQN_ERR_ARG;                        // dtqn.py:170-173
        const ActorBlock b = actor_block(net, static_cast<uint8_t*>(ro->state) + l.off[6 + cur], N);
        rc = dtqn::tiled_forward_bag_resident(net, theta, b.obs, b.actions, v.bag_obs, v.bag_act, N, n_max, L, ro->q_dev, bag->workspace, train_mode,
                                              dropout_seed, dropout_step, s, b.lens, nullptr, nullptr);
        if (rc != DTQN_OK) return rc;
    }
    if ((rc = dtqn::rollout_step_launch(net, rp, ro, vstep, cur, n_max, epsilon, store, authorize, run_forward ? 1 : 0, s)) != DTQN_OK) return rc;
    if ((rc = dtqn::devbag_stage_launch(net, rp, ro, bag, cur, 0, may_choose ? 1 : 0, s)) != DTQN_OK) return rc;
    if (!may_choose) return DTQN_OK;
    // the K + 1 candidate bags of environment i on its one context after the transition: the full L rows of the block the step wrote
    const ActorBlock out = actor_block(net, static_cast<uint8_t*>(ro->state) + l.off[6 + (cur ^ 1)], N);
    rc = dtqn::tiled_forward_bag_resident(net, theta, out.obs, out.actions, v.cand_obs, v.cand_act, N * (net->bag_size + 1), L, L, bag->q_cand,
                                          bag->workspace, 0, 0u, 0u, s, nullptr, v.seq_ctx, v.seq_start);
    if (rc != DTQN_OK) return rc;
    return dtqn::devbag_select_launch(net, bag, s);
}

// Device-resident evaluation (dtqn_deval.hip): the same in eval mode (no dropout key is taken) on the evaluation's state.
extern "C" int dtqn_deval_step(const DtqnNet* net, const float* theta, const DtqnEval* ev, uint32_t key, uint32_t step, int cur, int n_max,
                               int episodes, void* stream) {
    int rc = dtqn::deval_check(net, ev);
    if (rc != DTQN_OK) return rc;
    if (cur != 0 && cur != 1) return DTQN_ERR_ARG;
    if (episodes < 0 || episodes > ev->max_episodes) return DTQN_ERR_ARG;
    rc = resident_forward(net, theta, ev, dtqn::deval_layout(net, ev).off[8 + cur], n_max, 0, 0u, 0u, stream);
    if (rc != DTQN_OK) return rc;
    return dtqn::deval_step_launch(net, ev, key, step, cur, n_max, episodes, (hipStream_t)stream);
}

// Device-resident evaluation of a bag network: dtqn_deval_begin / _step with one bag per environment (dtqn_devbag.hip) -- up to five
// launches per step, nothing between.  DTQN_ERR_CONFIG for a network without a bag.
static int deval_bag_check(const DtqnNet* net, const DtqnEval* ev, const DtqnDevBag* bag) {
    if (!bag) return DTQN_ERR_ARG;
    const int rc = dtqn::deval_check_bags(net, ev);
    return rc != DTQN_OK ? rc : dtqn::devbag_check_eval(net, ev, bag);
}

extern "C" int dtqn_deval_begin_bag(const DtqnNet* net, const DtqnEval* ev, const DtqnDevBag* bag, uint32_t key, int episodes, void* stream) {
    int rc = deval_bag_check(net, ev, bag);
    if (rc != DTQN_OK) return rc;
    if (episodes < 0 || episodes > ev->max_episodes) return DTQN_ERR_ARG;
    if ((rc = dtqn::deval_begin_launch(net, ev, key, episodes, (hipStream_t)stream)) != DTQN_OK) return rc;
    return dtqn::devbag_stage_launch_eval(net, ev, bag, 0, 1, 0, (hipStream_t)stream);
}

extern "C" int dtqn_deval_step_bag(const DtqnNet* net, const float* theta, const DtqnEval* ev, const DtqnDevBag* bag, uint32_t key, uint32_t step,
                                   int cur, int n_max, int episodes, int may_choose, void* stream) {
    int rc = deval_bag_check(net, ev, bag);
    if (rc != DTQN_OK) return rc;
    if (cur != 0 && cur != 1) return DTQN_ERR_ARG;
    if (episodes < 0 || episodes > ev->max_episodes) return DTQN_ERR_ARG;
    if (!theta || !ev->q_dev) return DTQN_ERR_ARG;
    const int N = ev->n_envs, L = net->ctx_len;
    if (n_max < 1 || n_max > L) return DTQN_ERR_ARG;                            // dtqn.py:170-173
    hipStream_t s = (hipStream_t)stream;
    const dtqn::DevalLayout l = dtqn::deval_layout(net, ev);
    const dtqn::DevBagViews v = dtqn::devbag_views(net, bag);
    const ActorBlock b = actor_block(net, static_cast<uint8_t*>(ev->state) + l.off[8 + cur], N);
    rc = dtqn::tiled_forward_bag_resident(net, theta, b.obs, b.actions, v.bag_obs, v.bag_act, N, n_max, L, ev->q_dev, bag->workspace, 0, 0u, 0u, s,
                                          b.lens, nullptr, nullptr);
    if (rc != DTQN_OK) return rc;
    if ((rc = dtqn::deval_step_launch(net, ev, key, step, cur, n_max, episodes, s)) != DTQN_OK) return rc;
    if ((rc = dtqn::devbag_stage_launch_eval(net, ev, bag, cur, 0, may_choose ? 1 : 0, s)) != DTQN_OK) return rc;
    if (!may_choose) return DTQN_OK;
    // the K + 1 candidate bags of environment i on its one context after the transition: the layers once per environment, on the full L
    // rows of the block the step wrote
    const ActorBlock out = actor_block(net, static_cast<uint8_t*>(ev->state) + l.off[8 + (cur ^ 1)], N);
    rc = dtqn::tiled_forward_bag_candidates(net, theta, out.obs, out.actions, v.cand_obs, v.cand_act, N, net->bag_size + 1, L, bag->q_cand,
                                            bag->workspace, s);
    if (rc != DTQN_OK) return rc;
    return dtqn::devbag_select_launch(net, bag, s);
}

// The differentiable forward without dropout (the function the no-grad forward computes): the _drop entry points with the masks off.
extern "C" int dtqn_forward_train(const DtqnNet* net, const float* theta, const float* obs, const uint8_t* actions, const float* bag_obs,
                                  const uint8_t* bag_actions, int batch, int n, float* q_out, float* workspace, void* stream) {
    return dtqn_forward_train_drop(net, theta, obs, actions, bag_obs, bag_actions, batch, n, q_out, workspace, 0u, -1, stream);
}
extern "C" int dtqn_backward_dq(const DtqnNet* net, const float* theta, const float* obs, const uint8_t* actions, const float* bag_obs,
                                const uint8_t* bag_actions, int batch, int n, const float* dq, float* workspace, float* grad, float* dobs,
                                void* stream) {
    return dtqn_backward_dq_drop(net, theta, obs, actions, bag_obs, bag_actions, batch, n, dq, workspace, grad, dobs, 0u, -1, stream);
}
