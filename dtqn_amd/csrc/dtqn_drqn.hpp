// DRQN baseline (include/dtqn_hip.h, DrqnNet): launch geometry and workspace layout shared by dtqn_drqn.hip's entry points.
#pragma once
#include "dtqn_device.hpp"

namespace dtqn {

constexpr int kDrqnSeqs = 16;          // sequences per workgroup of the scans: the M dimension of the f32 16x16x4 fragment
// (the scans run D / 16 waves: wave w owns the hidden units [16 w, 16 w + 16) of its 16 sequences)
constexpr int kDrqnMaxCtx = 512;

// workspace: [lengths: int32 x up4(B)] [records: B n rec_row] [gradient records: B n grec_row]
__host__ __device__ inline size_t drqn_hdr_floats(int batch) { return (size_t)((batch + 3) & ~3); }

// One strided product on the matrix core, a 16 x 16 output tile per wave (drqn_gemm_kernel):
//   C[r][c] = epi( sum_k A[r sar + k sak] * B[k sbk + c sbc] )      r < R, c < Cn, k < K
// The contraction runs k-ascending in chains of 256 terms that are then added in order, per tile: the result does not depend on the grid.
struct DrqnGemm {
    const float* A; long long sar, sak;
    const float* B; long long sbk, sbc;
    float* C; long long ldc;
    int R, Cn, K;
    const float* bias1;       // [Cn] added in the epilogue (or nullptr)
    const float* bias2;
    int relu;                 // epilogue: max(., 0)
    const float* gate;        // epilogue: the value passes where gate[r ldgate + c] > 0 (ReLU backward), else 0
    long long ldgate;
    // token masks (rows of the packed batch at or beyond their sequence's length are never read):
    const int32_t* lens;      // [B] on the device; nullptr = no masking
    int n;                    // rows per sequence (token m = b n + t)
    int k_tokens;             // the contraction index is a token: B's row k is taken as 0 / pad_fill where token k is padding
    int k_shift;              // ... and B's row k is the row of token k - 1 of the same sequence (0 at t = 0): h_{t-1} for weight_hh
    int r_tokens;             // the output row is a token: `gate` of a padding row is pad_fill
    const float* pad_fill;    // [Cn] the value a padding row holds is max(pad_fill[c], 0) (ReLU(ffn.0 bias): the head of zero); nullptr = 0
};

}  // namespace dtqn
