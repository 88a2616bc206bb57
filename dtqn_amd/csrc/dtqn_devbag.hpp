// Device-resident bags (dtqn_devbag.hip): one persistent-memory bag per environment of the device-resident rollout, the layout of
// their state allocation and the launches dtqn_api.cpp sequences around the rollout's step kernel.
#pragma once
#include <hip/hip_runtime.h>

#include "dtqn_hip.h"

namespace dtqn {

// Byte offsets of the sections of DtqnDevBag::state (include/dtqn_hip.h lists them), every section 16-byte aligned.
struct DevBagLayout {
    size_t off[DTQN_DEVBAG_OFFSETS];
    size_t bytes;
};
inline DevBagLayout devbag_layout(const DtqnNet* net, const DtqnDevBag* bag) {
    DevBagLayout l;
    const size_t N = (size_t)bag->n_envs, K = (size_t)net->bag_size, O = (size_t)net->obs_dim, C = K + 1;
    const size_t sizes[DTQN_DEVBAG_OFFSETS] = {4 * N * K * O, N * K, 4 * N, 4 * N * C * K * O, N * C * K, 4 * N, 4 * N * C, 4 * N, 8 * DTQN_DEVBAG_COUNTERS,
                                               4 * 2 * N * C};
    size_t at = 0;
    for (int k = 0; k < DTQN_DEVBAG_OFFSETS; ++k) {
        l.off[k] = at;
        at += (sizes[k] + 15) & ~(size_t)15;
    }
    l.bytes = at;
    return l;
}

// DTQN_OK when the bag descriptor fits the network and the rollout it rides on; DTQN_ERR_CONFIG: no bag, dropout, too many candidates.
int devbag_check(const DtqnNet* net, const DtqnRollout* ro, const DtqnDevBag* bag);
// The same for the bags of the device-resident evaluation, which admits dropout: it never runs train mode.
int devbag_check_eval(const DtqnNet* net, const DtqnEval* ev, const DtqnDevBag* bag);
// The sections the forwards read: the bags (actor forward), the candidates and their sequence -> context index table (candidate forward).
struct DevBagViews {
    const float *bag_obs, *cand_obs;
    const uint8_t *bag_act, *cand_act;
    const int32_t *seq_ctx, *seq_start;
};
DevBagViews devbag_views(const DtqnNet* net, const DtqnDevBag* bag);
// reset_all != 0: every bag and every candidate slot cleared (after the rollout's reset); else the bookkeeping of one vector step, after
// the rollout's step kernel has run on block `cur` (it reads `last`, `elapsed` and row 0 of block `cur` out of the rollout's state).
int devbag_stage_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, const DtqnDevBag* bag, int cur, int reset_all,
                        int may_choose, hipStream_t stream);
// The same kernel behind the evaluation's step kernel: `last`, `elapsed` and row 0 of block `cur` out of the evaluation's state.
int devbag_stage_launch_eval(const DtqnNet* net, const DtqnEval* ev, const DtqnDevBag* bag, int cur, int reset_all, int may_choose,
                             hipStream_t stream);
int devbag_select_launch(const DtqnNet* net, const DtqnDevBag* bag, hipStream_t stream);

// dtqn_tiled.hip: the row-block forward of a bag network on resident arrays.  lens: ragged prefixes or nullptr (n rows each); seq_src /
// seq_start (device [batch] each, or both nullptr): sequence s reads context seq_src[s] of obs / actions from row seq_start[s].
int tiled_forward_bag_resident(const DtqnNet* net, const float* theta, const float* obs, const uint8_t* actions, const float* bag_obs,
                               const uint8_t* bag_actions, int batch, int n, int in_rows, float* q_out, float* workspace, int train_mode,
                               uint32_t drop_seed, uint32_t drop_step, hipStream_t stream, const int32_t* lens, const int32_t* seq_src,
                               const int32_t* seq_start);

// The candidate forward on a shared trunk: eval-mode Q of n_ctx whole contexts under n_cand candidate bags each (cand_obs
// [n_ctx][n_cand][K][O], cand_act [n_ctx][n_cand][K]) -> q_out [n_ctx][n_cand][L][A]; the layers run once per context.  workspace:
// dtqn_bag_candidates_workspace_floats(net, n_ctx, n_cand) floats.
int tiled_forward_bag_candidates(const DtqnNet* net, const float* theta, const float* obs, const uint8_t* actions, const float* cand_obs,
                                 const uint8_t* cand_act, int n_ctx, int n_cand, int in_rows, float* q_out, float* workspace, hipStream_t stream);

}  // namespace dtqn
