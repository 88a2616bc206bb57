// Pieces the batched actor entry points share (dtqn_actor.hip, dtqn_image.hip; dtqn_api.cpp declares the launchers itself: it is
// host-only C++).
#pragma once
#include "dtqn_device.hpp"

namespace dtqn {

// Fixed-order compaction inside one workgroup of NT threads: thread t brings the count c of its own contiguous range and gets the
// number of items the threads in front of it hold (inclusive scan in LDS, sums[NT]); no atomics.  Every thread of the workgroup calls it.
template <int NT>
__device__ __forceinline__ int block_scan_exclusive(int32_t* sums, int t, int c) {
    __syncthreads();                     // (a caller may scan twice through the same array)
    sums[t] = c;
    __syncthreads();
    for (int off = 1; off < NT; off <<= 1) {
        const int v = t >= off ? sums[t - off] : 0;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    return sums[t] - c;
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
