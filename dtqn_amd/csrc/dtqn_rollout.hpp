// Device-resident rollout: the layout of its one state allocation and the launches dtqn_api.cpp sequences (dtqn_rollout.hip).  The
// environments, the draws and the step bookkeeping it shares with the device-resident evaluation are in dtqn_devenv.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "dtqn_actor.hpp"
#include "dtqn_hip.h"

namespace dtqn {

// Byte offsets of the sections of DtqnRollout::state (include/dtqn_hip.h lists them), every section 16-byte aligned.
struct RolloutLayout {
    size_t off[DTQN_ROLLOUT_OFFSETS];
    size_t bytes;
    size_t block_bytes;
};
inline RolloutLayout rollout_layout(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro) {
    RolloutLayout l;
    const int n_envs = ro->n_envs;
    const size_t N = (size_t)n_envs, T = (size_t)rp->max_steps, O = (size_t)net->obs_dim, K = (size_t)ro->pending_slots;
    l.block_bytes = (actor_block(net, nullptr, n_envs).bytes + 15) & ~(size_t)15;
    const size_t counters = 8 * (DTQN_ROLLOUT_STATUS_WORDS / 2);      // i64 each: two granules of the status record
    const size_t sizes[DTQN_ROLLOUT_OFFSETS] = {counters,            8 * N * 4,     4 * N * DTQN_DEVENV_STATE_INTS, 4 * N, 8 * N,     4 * N * DTQN_DEVENV_LAST_INTS,
                                                l.block_bytes,       l.block_bytes, 4 * N * (T + 1) * O,            N * T, 4 * N * T, N * T,
                                                4 * K * (T + 1) * O, K * T,         4 * K * T,                      K * T, 4 * K};
    size_t at = 0;
    for (int k = 0; k < DTQN_ROLLOUT_OFFSETS; ++k) {
        l.off[k] = at;
        at += (sizes[k] + 15) & ~(size_t)15;
    }
    l.bytes = at;
    return l;
}

// DTQN_OK when the descriptor, the network and the replay fit the kernels (flat f32 observations of the environment's width, ...)
int rollout_check(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro);
// ... and the same check for the callers that admit a bag network (dtqn_devbag.hpp)
int rollout_check_bags(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro);
int rollout_reset_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, hipStream_t stream);
// q_rows: where the step kernel finds Q of the last live row -- q_last [N][A] (stride 0) or q_dev with n_max rows per sequence
int rollout_step_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, int cur, int n_max, float epsilon,
                        int store, long long authorize, int have_q, hipStream_t stream);
int rollout_commit_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, long long authorize, hipStream_t stream);

}  // namespace dtqn
