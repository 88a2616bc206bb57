// Device-resident greedy evaluation: the layout of its one state allocation and the launches dtqn_api.cpp sequences (dtqn_deval.hip).
// The environments, the draws and the step bookkeeping it shares with the device-resident rollout are in dtqn_devenv.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include "dtqn_actor.hpp"
#include "dtqn_hip.h"

namespace dtqn {

constexpr int kDevalResultBytes = DTQN_DEVAL_RESULT_BYTES;  // f64 return | i32 length | i32 success | i32 environment | i32 vector step it finished in

// Byte offsets of the sections of DtqnEval::state (include/dtqn_hip.h lists them), every section 16-byte aligned.
struct DevalLayout {
    size_t off[DTQN_DEVAL_OFFSETS];
    size_t bytes;
    size_t block_bytes;
};
inline DevalLayout deval_layout(const DtqnNet* net, const DtqnEval* ev) {
    DevalLayout l;
    const size_t N = (size_t)ev->n_envs, O = (size_t)net->obs_dim, K = (size_t)ev->max_episodes;
    l.block_bytes = (actor_block(net, nullptr, ev->n_envs).bytes + 15) & ~(size_t)15;
    const size_t counters = 8 * (DTQN_DEVAL_STATUS_WORDS / 2);        // i64 each: two granules of the status record
    const size_t sizes[DTQN_DEVAL_OFFSETS] = {counters,                      8 * N * 4, 4 * N * DTQN_DEVENV_STATE_INTS, 4 * N,         8 * N, 4 * N,
                                              4 * N * DTQN_DEVENV_LAST_INTS, 4 * N * O, l.block_bytes,                  l.block_bytes, kDevalResultBytes * K};
    size_t at = 0;
    for (int k = 0; k < DTQN_DEVAL_OFFSETS; ++k) {
        l.off[k] = at;
        at += (sizes[k] + 15) & ~(size_t)15;
    }
    l.bytes = at;
    return l;
}

// DTQN_OK when the descriptor and the network fit the kernels (flat f32 observations of the environment's width, ...)
int deval_check(const DtqnNet* net, const DtqnEval* ev);
// ... and the same check for the callers that admit a bag network (dtqn_devbag.hpp)
int deval_check_bags(const DtqnNet* net, const DtqnEval* ev);
int deval_begin_launch(const DtqnNet* net, const DtqnEval* ev, uint32_t key, int episodes, hipStream_t stream);
// Q of the last live rows: q_last [N][A] (whole-sequence networks) or q_dev with n_max rows per sequence (row-block ones)
int deval_step_launch(const DtqnNet* net, const DtqnEval* ev, uint32_t key, uint32_t step, int cur, int n_max, int episodes, hipStream_t stream);

}  // namespace dtqn
