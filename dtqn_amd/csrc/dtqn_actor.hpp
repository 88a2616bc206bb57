// Host-side pieces the batched actor entry points share (dtqn_actor.hip, dtqn_image.hip, dtqn_api.cpp), and the one arg-max of a Q row.
#pragma once
#include <hip/hip_runtime.h>

#include "dtqn_hip.h"

namespace dtqn {

// The packed block of the batched actor entry points, pinned host copy and device copy alike:
// [N][ctx_len * obs_dim] f32 observations | [N][ctx_len] u8 actions, padded to 4 bytes | [N] i32 live rows.
struct ActorBlock {
    float* obs;
    uint8_t* actions;
    int32_t* lens;
    size_t bytes;
};
inline ActorBlock actor_block(const DtqnNet* net, const void* base, int n_envs) {
    const size_t obs_bytes = sizeof(float) * (size_t)n_envs * net->ctx_len * net->obs_dim;
    const size_t act_bytes = (((size_t)n_envs * net->ctx_len) + 3) & ~(size_t)3;       // keeps the int32 block 4-byte aligned
    uint8_t* p = static_cast<uint8_t*>(const_cast<void*>(base));
    return ActorBlock{reinterpret_cast<float*>(p), p + obs_bytes, reinterpret_cast<int32_t*>(p + obs_bytes + act_bytes),
                      obs_bytes + act_bytes + sizeof(int32_t) * (size_t)n_envs};
}

// The greedy action of a Q row, by the rule of torch.argmax / np.argmax: the first maximum, and a NaN counts as the maximum.  The one
// copy: actor_greedy_kernel, the device-resident rollout and the device-resident evaluation call it.
__device__ __forceinline__ int first_argmax(const float* q, int n) {
    float best = q[0];
    int arg = 0;
    for (int k = 1; k < n; ++k) {
        const float v = q[k];
        if (v > best || (v != v && best == best)) {
            best = v;
            arg = k;
        }
    }
    return arg;
}

// Greedy evaluation (dtqn_actor_greedy_batch / dtqn_img_actor_greedy_batch): len_i == 0 marks environment i as idle.
// The live contexts of the pinned block ctx_host (layout of dtqn_actor_forward_batch) -> sequences 0 .. live - 1 of ctx_dev, in
// environment order, rows [0, n_max) each; the compacted live-row counts -> the len block of ctx_dev.
int actor_compact(const DtqnNet* net, const void* ctx_host, void* ctx_dev, int n_envs, int n_max, hipStream_t stream);
// q: [live][n_max][A] of the compacted sequences; lens: [n_envs] (0 = idle; device or pinned host memory).  Live environment i:
// q_last[i][A] <- Q of row len_i - 1 of its sequence, action[i] <- the arg-max (first maximum); idle: action[i] <- -1, q_last untouched.
int actor_greedy_rows(const int32_t* lens, const float* q, float* q_last, int32_t* action, int n_envs, int n_max, int A, hipStream_t stream);
void set_last_actor_live(int live);

}  // namespace dtqn
