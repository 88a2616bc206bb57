// DRQN baseline on gfx950 (include/dtqn_hip.h, DrqnNet): observation embedding -> LSTM -> Linear, ReLU, Linear
// (dtqn/networks/drqn.py:38-66, torch.nn.LSTM gate order i | f | g | o).
//
//   token-parallel products   drqn_gemm_kernel: one strided product on the f32 16x16x4 matrix core, a 16 x 16 output tile per wave,
//                             used for the embedding Linear, the input projection of all tokens at once, the head and -- in the
//                             backward -- every data gradient and every weight gradient (contraction over the tokens, in token order)
//   forward scan              drqn_scan_kernel<D>: 16 sequences per workgroup for all time steps (the M dimension of the fragment); D / 16
//                             waves, wave w owns the hidden units [16 w, 16 w + 16) and the four gate columns of each, so the cell update is
//                             lane-local; h_t goes round through a double-buffered LDS tile, one barrier per step.  weight_hh: at D = 64 the
//                             wave's share (64 registers) stays in registers for the whole scan; at 128 / 256 it is streamed from L2 every step
//   reverse scan              drqn_bptt_kernel<D>: the same ownership; d(gates) of a step goes through LDS into dh_{t-1} = d(gates) W_hh
// No workgroup waits for another, no float atomics; every sum has one order, whatever the grid.
#include <vector>

#include "dtqn_drqn.hpp"
#include "dtqn_frag16.hpp"

namespace dtqn {

__global__ __launch_bounds__(256) void drqn_gemm_kernel(DrqnGemm g) {
    const Thr t = make_thr();
    const int ctiles = (g.Cn + 15) >> 4, rtiles = (g.R + 15) >> 4;
    const int tile = (int)blockIdx.x * 4 + t.wave;
    if (tile >= ctiles * rtiles) return;                    // (wave-uniform; the kernel has no barrier)
    const int rt = tile / ctiles, ct = tile - rt * ctiles;
    const int row = rt * 16 + t.i, col = ct * 16 + t.i;     // this lane's row of the A operand and column of the B operand
    const bool rok = row < g.R, cok = col < g.Cn;
    const float* ap = g.A + (long long)(rok ? row : 0) * g.sar;
    const float* bp = g.B + (long long)(cok ? col : 0) * g.sbc;
    const float fill = (g.pad_fill != nullptr && cok) ? fmaxf(g.pad_fill[col], 0.f) : 0.f;
    f32x4 acc = zero4(), tot = zero4();
    for (int k0 = 0; k0 < g.K; k0 += 4) {
        const int k = k0 + t.kq;
        float a = 0.f, b = 0.f;
        if (k < g.K) {
            if (rok) a = ap[(long long)k * g.sak];
            if (cok) {
                if (g.k_tokens) {
                    const int bb = k / g.n, tt = k - bb * g.n;
                    const bool pad = tt >= g.lens[bb];
                    if (g.k_shift) b = (tt == 0 || pad) ? 0.f : bp[(long long)(k - 1) * g.sbk];
                    else b = pad ? fill : bp[(long long)k * g.sbk];
                } else {
                    b = bp[(long long)k * g.sbk];
                }
            }
        }
        acc = mfma16(a, b, acc);
        if ((k0 & 255) == 252) {            // two-level sum: a chain of 256 terms, then the chains in order (weight gradients contract thousands of tokens)
#pragma unroll
            for (int r = 0; r < 4; ++r) { tot[r] += acc[r]; acc[r] = 0.f; }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += tot[r];
    if (!cok) return;
    const float bsum = (g.bias1 != nullptr ? g.bias1[col] : 0.f) + (g.bias2 != nullptr ? g.bias2[col] : 0.f);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int orow = rt * 16 + t.kq * 4 + r;
        if (orow >= g.R) continue;
        float v = acc[r] + bsum;
        if (g.relu) v = fmaxf(v, 0.f);
        if (g.gate != nullptr) {
            bool on;
            if (g.r_tokens && (orow % g.n) >= g.lens[orow / g.n]) on = g.pad_fill != nullptr && g.pad_fill[col] > 0.f;
            else on = g.gate[(long long)orow * g.ldgate + col] > 0.f;
            v = on ? v : 0.f;
        }
        g.C[(long long)orow * g.ldc + col] = v;
    }
}

// out[c] (and out2[c]) = sum over the M rows of Y[m][c], in one fixed order: the bias gradients
__global__ __launch_bounds__(256) void drqn_colsum_kernel(const float* __restrict__ Y, long long ld, int M, int N, float* __restrict__ out,
                                                         float* __restrict__ out2) {
    const int c = (int)(blockIdx.x * 256 + threadIdx.x);
    if (c >= N) return;
    float s = 0.f, part = 0.f;                 // two-level sum: 64 rows at a time, then the parts in order
    for (int m = 0; m < M; ++m) {
        part += Y[(long long)m * ld + c];
        if ((m & 63) == 63) { s += part; part = 0.f; }
    }
    s += part;
    out[c] = s;
    if (out2 != nullptr) out2[c] = s;
}

__device__ __forceinline__ int drqn_token(const float* __restrict__ obs, long long idx, int V) {
    const int tok = (int)obs[idx];
    return tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
}

// discrete observations: e[m][o E + j] = table[token(m, o)][j] into the row records (columns ke .. kep are zero)
__global__ __launch_bounds__(256) void drqn_gather_kernel(const float* __restrict__ obs, const float* __restrict__ tab, float* __restrict__ e,
                                                         long long ld, int M, int O, int E, int V, int kep) {
    const long long id = (long long)blockIdx.x * 256 + threadIdx.x;
    if (id >= (long long)M * kep) return;
    const int m = (int)(id / kep), k = (int)(id - (long long)m * kep);
    float v = 0.f;
    if (k < O * E) {
        const int o = k / E, j = k - o * E;
        v = tab[(size_t)drqn_token(obs, (long long)m * O + o, V) * E + j];
    }
    e[(long long)m * ld + k] = v;
}

// d(table)[v][j] = sum over tokens m (ascending), positions o (ascending) with token(m, o) == v of de[m][o E + j]: one thread per table
// element walks the batch in one order (de of a padding row is zero: nothing reaches it from d(gates) = 0)
__global__ __launch_bounds__(256) void drqn_table_grad_kernel(const float* __restrict__ obs, const float* __restrict__ de, long long ld, int M,
                                                             int O, int E, int V, float* __restrict__ out) {
    const int id = (int)(blockIdx.x * 256 + threadIdx.x);
    if (id >= V * E) return;
    const int v = id / E, j = id - v * E;
    float s = 0.f;
    for (int m = 0; m < M; ++m)
        for (int o = 0; o < O; ++o)
            if (drqn_token(obs, (long long)m * O + o, V) == v) s += de[(long long)m * ld + o * E + j];
    out[id] = s;
}

__device__ __forceinline__ float drqn_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// rec: the row records (rec_row floats per token); the gate record holds x W_ih^T + b_ih + b_hh on entry
template <int D, bool TRAIN>
__global__ __launch_bounds__(D * 4) void drqn_scan_kernel(const float* __restrict__ Whh, float* __restrict__ rec, int rec_row, int o_gates, int o_c,
                                                       int o_h, const int32_t* __restrict__ lens, const float* __restrict__ h0,
                                                       const float* __restrict__ c0, float* __restrict__ h_n, float* __restrict__ c_n, int B, int n) {
    constexpr int IPW = 1, LDH = D + 4, NT = D * 4;   // one 16-unit tile per wave (D / 16 waves); row stride of the h tile
    float* hs = reinterpret_cast<float*>(dtqn_smem);   // [2][16][LDH]
    const Thr t = make_thr();
    const int b0 = (int)blockIdx.x * kDrqnSeqs;
    for (int x = t.tid; x < 16 * D; x += NT) {
        const int s = x / D, d = x - s * D, b = b0 + s;
        hs[s * LDH + d] = (h0 != nullptr && b < B) ? h0[(size_t)b * D + d] : 0.f;
    }
    int len[4];
    float cst[IPW][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = b0 + t.kq * 4 + r;
        len[r] = b < B ? lens[b] : 0;
#pragma unroll
        for (int it = 0; it < IPW; ++it) {
            const int col = (t.wave * IPW + it) * 16 + t.i;
            cst[it][r] = (c0 != nullptr && b < B) ? c0[(size_t)b * D + col] : 0.f;
        }
    }
    float4 wres[4][4];                                 // D = 64: this wave's rows of weight_hh for the whole scan
    if constexpr (D == 64) {
#pragma unroll
        for (int q = 0; q < 4; ++q) frag16_fetch<64>(wres[q], Whh + (size_t)(q * D + t.wave * 16 + t.i) * D, t);
    }
    __syncthreads();
    for (int ts = 0; ts < n; ++ts) {
        const float* hc = hs + (ts & 1) * 16 * LDH;
        float* hn = hs + ((ts & 1) ^ 1) * 16 * LDH;
#pragma unroll
        for (int it = 0; it < IPW; ++it) {
            const int col = (t.wave * IPW + it) * 16 + t.i;
            f32x4 acc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int b = min(b0 + t.kq * 4 + r, B - 1);
                const float* gp = rec + ((size_t)b * n + ts) * rec_row + o_gates + col;
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q][r] = gp[q * D];
            }
#pragma unroll 1
            for (int kc = 0; kc < D / 64; ++kc) {       // (one 64-column slice of weight_hh in registers at a time)
                float4 wf[4][4];
                if constexpr (D == 64) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int s = 0; s < 4; ++s) wf[q][s] = wres[q][s];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) frag16_fetch<64>(wf[q], Whh + (size_t)(q * D + col) * D + kc * 64, t);
                }
                const float* xp = hc + t.i * LDH + kc * 64 + t.kq * 4;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float4 a = ld4(xp + 16 * s);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = mfma16(a.x, wf[q][s].x, acc[q]);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = mfma16(a.y, wf[q][s].y, acc[q]);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = mfma16(a.z, wf[q][s].z, acc[q]);
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[q] = mfma16(a.w, wf[q][s].w, acc[q]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int srow = t.kq * 4 + r, b = b0 + srow;
                const bool live = ts < len[r];
                const float ig = drqn_sigmoid(acc[0][r]), fg = drqn_sigmoid(acc[1][r]), gg = tanhf(acc[2][r]), og = drqn_sigmoid(acc[3][r]);
                const float c_new = fg * cst[it][r] + ig * gg;
                const float h_new = og * tanhf(c_new);
                hn[srow * LDH + col] = live ? h_new : hc[srow * LDH + col];
                if (live) cst[it][r] = c_new;
                if (b < B) {
                    float* rp = rec + ((size_t)b * n + ts) * rec_row;
                    rp[o_h + col] = live ? h_new : 0.f;
                    if (TRAIN && live) {
                        rp[o_gates + col] = ig; rp[o_gates + D + col] = fg; rp[o_gates + 2 * D + col] = gg; rp[o_gates + 3 * D + col] = og;
                        rp[o_c + col] = c_new;
                    }
                }
            }
        }
        __syncthreads();
    }
    const float* hf = hs + (n & 1) * 16 * LDH;
#pragma unroll
    for (int it = 0; it < IPW; ++it) {
        const int col = (t.wave * IPW + it) * 16 + t.i;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int srow = t.kq * 4 + r, b = b0 + srow;
            if (b < B) {
                if (h_n != nullptr) h_n[(size_t)b * D + col] = hf[srow * LDH + col];
                if (c_n != nullptr) c_n[(size_t)b * D + col] = cst[it][r];
            }
        }
    }
}

// Backpropagation through time from the zero state: reads the activated gates and cell rows of live rows, dh of the head; writes
// d(gate pre-activations) of every row (zeros at padding rows)
template <int D>
__global__ __launch_bounds__(D * 4) void drqn_bptt_kernel(const float* __restrict__ Whh, const float* __restrict__ rec, int rec_row, int o_gates,
                                                       int o_c, float* __restrict__ grec, int grec_row, int o_dh, int o_dg,
                                                       const int32_t* __restrict__ lens, int B, int n) {
    constexpr int IPW = 1, LDG = 4 * D + 4;
    float* dgs = reinterpret_cast<float*>(dtqn_smem);  // [16][LDG]: d(gates) of the step, the A operand of dh_{t-1}
    const Thr t = make_thr();
    const int b0 = (int)blockIdx.x * kDrqnSeqs;
    int len[4];
    float dhc[IPW][4], dcc[IPW][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int b = b0 + t.kq * 4 + r;
        len[r] = b < B ? lens[b] : 0;
#pragma unroll
        for (int it = 0; it < IPW; ++it) { dhc[it][r] = 0.f; dcc[it][r] = 0.f; }
    }
    for (int ts = n - 1; ts >= 0; --ts) {
#pragma unroll
        for (int it = 0; it < IPW; ++it) {
            const int col = (t.wave * IPW + it) * 16 + t.i;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int srow = t.kq * 4 + r, b = b0 + srow;
                float di = 0.f, df = 0.f, dg = 0.f, dob = 0.f;
                if (ts < len[r]) {
                    const float* rp = rec + ((size_t)b * n + ts) * rec_row;
                    const float ig = rp[o_gates + col], fg = rp[o_gates + D + col], gg = rp[o_gates + 2 * D + col], og = rp[o_gates + 3 * D + col];
                    const float c_prev = ts > 0 ? rp[o_c + col - rec_row] : 0.f;
                    const float tc = tanhf(rp[o_c + col]);
                    const float dh = grec[((size_t)b * n + ts) * grec_row + o_dh + col] + dhc[it][r];
                    const float dc = dcc[it][r] + dh * og * (1.0f - tc * tc);
                    dob = dh * tc * og * (1.0f - og);
                    di = dc * gg * ig * (1.0f - ig);
                    dg = dc * ig * (1.0f - gg * gg);
                    df = dc * c_prev * fg * (1.0f - fg);
                    dcc[it][r] = dc * fg;
                }
                float* lp = dgs + srow * LDG + col;
                lp[0] = di; lp[D] = df; lp[2 * D] = dg; lp[3 * D] = dob;
                if (b < B) {
                    float* gp = grec + ((size_t)b * n + ts) * grec_row + o_dg + col;
                    gp[0] = di; gp[D] = df; gp[2 * D] = dg; gp[3 * D] = dob;
                }
            }
        }
        __syncthreads();
        // dh_{t-1}[seq][unit] = sum over the 4D gate columns g (ascending in two interleaved chains) of d(gates)[seq][g] W_hh[g][unit]
#pragma unroll
        for (int it = 0; it < IPW; ++it) {
            const int col = (t.wave * IPW + it) * 16 + t.i;
            const float* xp = dgs + t.i * LDG + t.kq * 4;
            const float* wp = Whh + (size_t)(t.kq * 4) * D + col;
            f32x4 a0 = zero4(), a1 = zero4();
            for (int s = 0; s < (4 * D) / 16; ++s) {
                const float4 a = ld4(xp + 16 * s);
                const float* w = wp + (size_t)(16 * s) * D;
                a0 = mfma16(a.x, w[0], a0);
                a1 = mfma16(a.y, w[D], a1);
                a0 = mfma16(a.z, w[2 * D], a0);
                a1 = mfma16(a.w, w[3 * D], a1);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) dhc[it][r] = a0[r] + a1[r];
        }
        __syncthreads();
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------
static int drqn_launch_gemm(const DrqnGemm& g, hipStream_t s) {
    const int tiles = ((g.R + 15) / 16) * ((g.Cn + 15) / 16);
    if (tiles <= 0 || g.K <= 0) return DTQN_ERR_ARG;
    hipLaunchKernelGGL(drqn_gemm_kernel, dim3((tiles + 3) / 4), dim3(256), 0, s, g);
    return DTQN_OK;
}
static DrqnGemm drqn_gemm(const float* A, long long sar, long long sak, const float* B, long long sbk, long long sbc, float* C, long long ldc,
                          int R, int Cn, int K) {
    DrqnGemm g = {};
    g.A = A; g.sar = sar; g.sak = sak; g.B = B; g.sbk = sbk; g.sbc = sbc; g.C = C; g.ldc = ldc; g.R = R; g.Cn = Cn; g.K = K;
    g.n = 1;
    return g;
}

template <int D, bool TRAIN>
static void drqn_launch_scan(const DrqnNet* net, const float* theta, float* rec, const int32_t* dlens, const float* h0, const float* c0,
                             float* h_n, float* c_n, int B, int n, hipStream_t s) {
    const size_t lds = (size_t)2 * 16 * (D + 4) * sizeof(float);
    static size_t attr_lds[kMaxDevices] = {};
    raise_lds_limit(reinterpret_cast<const void*>(&drqn_scan_kernel<D, TRAIN>), lds, attr_lds);
    hipLaunchKernelGGL((drqn_scan_kernel<D, TRAIN>), dim3((B + kDrqnSeqs - 1) / kDrqnSeqs), dim3(D * 4), lds, s, theta + net->off_w_hh, rec,
                       net->rec_row, net->rec_gates, net->rec_c, net->rec_h, dlens, h0, c0, h_n, c_n, B, n);
}
template <int D>
static void drqn_launch_bptt(const DrqnNet* net, const float* theta, const float* rec, float* grec, const int32_t* dlens, int B, int n,
                             hipStream_t s) {
    const size_t lds = (size_t)16 * (4 * D + 4) * sizeof(float);
    static size_t attr_lds[kMaxDevices] = {};
    raise_lds_limit(reinterpret_cast<const void*>(&drqn_bptt_kernel<D>), lds, attr_lds);
    hipLaunchKernelGGL((drqn_bptt_kernel<D>), dim3((B + kDrqnSeqs - 1) / kDrqnSeqs), dim3(D * 4), lds, s, theta + net->off_w_hh, rec,
                       net->rec_row, net->rec_gates, net->rec_c, grec, net->grec_row, net->grec_dh, net->grec_dg, dlens, B, n);
}

static bool drqn_net_ok(const DrqnNet* net) {
    return net != nullptr && (net->d_model == 64 || net->d_model == 128 || net->d_model == 256) && net->rec_row > 0 && net->n_theta > 0;
}

static int drqn_forward_impl(const DrqnNet* net, const float* theta, const float* obs, const int32_t* lengths, const float* h0, const float* c0,
                             int B, int n, float* q_out, float* h_n, float* c_n, float* ws, void* stream, bool train) {
    if (!drqn_net_ok(net)) return DTQN_ERR_CONFIG;
    if (!theta || !obs || !q_out || !ws || B < 1 || n < 1 || n > net->ctx_len || (h0 == nullptr) != (c0 == nullptr)) return DTQN_ERR_ARG;
    if ((long long)B * n > (1ll << 24)) return DTQN_ERR_ARG;
    std::vector<int32_t> hl((size_t)B, n);
    if (lengths != nullptr) {
        for (int b = 0; b < B; ++b) {
            if (lengths[b] < 1 || lengths[b] > n) return DTQN_ERR_ARG;
            hl[b] = lengths[b];
        }
    }
    hipStream_t s = (hipStream_t)stream;
    (void)hipGetLastError();
    int32_t* dlens = reinterpret_cast<int32_t*>(ws);
    if (hipMemcpyAsync(dlens, hl.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, s) != hipSuccess) return DTQN_ERR_LAUNCH;
    if (hipStreamSynchronize(s) != hipSuccess) return DTQN_ERR_LAUNCH;          // `hl` goes with this frame
    const int D = net->d_model, A = net->num_actions, M = B * n, RR = net->rec_row;
    float* rec = ws + drqn_hdr_floats(B);
    int rc = DTQN_OK;
    // observation embedding
    if (net->discrete) {
        const long long cells = (long long)M * net->kep;
        hipLaunchKernelGGL(drqn_gather_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, obs, theta + net->off_obs_tab, rec + net->rec_e,
                           (long long)RR, M, net->obs_dim, net->embed_per_obs, net->vocab, net->kep);
    }
    {
        DrqnGemm g = net->discrete ? drqn_gemm(rec + net->rec_e, RR, 1, theta + net->off_obs_w, 1, net->ke, rec + net->rec_x, RR, M, D, net->ke)
                                   : drqn_gemm(obs, net->obs_dim, 1, theta + net->off_obs_w, 1, net->ke, rec + net->rec_x, RR, M, D, net->ke);
        g.bias1 = theta + net->off_obs_b;
        if ((rc = drqn_launch_gemm(g, s)) != DTQN_OK) return rc;
    }
    {   // input projection of every token, both biases
        DrqnGemm g = drqn_gemm(rec + net->rec_x, RR, 1, theta + net->off_w_ih, 1, D, rec + net->rec_gates, RR, M, 4 * D, D);
        g.bias1 = theta + net->off_b_ih; g.bias2 = theta + net->off_b_hh;
        if ((rc = drqn_launch_gemm(g, s)) != DTQN_OK) return rc;
    }
#define DRQN_SCAN(D_)                                                                                              \
    if (train) drqn_launch_scan<D_, true>(net, theta, rec, dlens, h0, c0, h_n, c_n, B, n, s);                     \
    else drqn_launch_scan<D_, false>(net, theta, rec, dlens, h0, c0, h_n, c_n, B, n, s)
    if (D == 64) { DRQN_SCAN(64); } else if (D == 128) { DRQN_SCAN(128); } else { DRQN_SCAN(256); }
#undef DRQN_SCAN
    {   // head: Linear, ReLU, Linear on every row
        DrqnGemm g = drqn_gemm(rec + net->rec_h, RR, 1, theta + net->off_head1_w, 1, D, rec + net->rec_z1, RR, M, D, D);
        g.bias1 = theta + net->off_head1_b; g.relu = 1;
        if ((rc = drqn_launch_gemm(g, s)) != DTQN_OK) return rc;
        DrqnGemm q = drqn_gemm(rec + net->rec_z1, RR, 1, theta + net->off_head2_w, 1, D, q_out, A, M, A, D);
        q.bias1 = theta + net->off_head2_b;
        if ((rc = drqn_launch_gemm(q, s)) != DTQN_OK) return rc;
    }
    return hipGetLastError() == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}

}  // namespace dtqn

using namespace dtqn;

extern "C" int dtqn_drqn_net_init(DrqnNet* net) {
    if (!net) return DTQN_ERR_ARG;
    const int O = net->obs_dim, A = net->num_actions, e = net->embed_per_obs, D = net->d_model, L = net->ctx_len, V = net->vocab;
    net->rec_row = 0; net->n_theta = 0; net->n_trainable = 0;
    if (O < 1 || A < 1 || A > DTQN_MAX_ACTIONS || !(D == 64 || D == 128 || D == 256) || L < 1 || L > kDrqnMaxCtx) return DTQN_ERR_CONFIG;
    if (net->discrete) {
        if (V < 1 || e < 1 || O > DTQN_MAX_OBS_TOKENS || (long long)O * e > DTQN_MAX_EMBED_COLS || (long long)V * e > DTQN_MAX_TABLE_FLOATS)
            return DTQN_ERR_CONFIG;
    } else if (O > DTQN_MAX_EMBED_COLS) {
        return DTQN_ERR_CONFIG;
    }
    auto up4 = [](int x) { return (x + 3) & ~3; };
    net->ke = net->discrete ? O * e : O;
    net->kep = up4(net->ke);
    net->ap = up4(A);
    int pos = 0;
    auto take = [&](int nfl) { const int at = pos; pos += up4(nfl); return at; };       // every tensor starts on a 16-byte boundary
    net->off_obs_tab = net->discrete ? take(V * e) : -1;
    net->off_obs_w = take(D * net->ke);
    net->off_obs_b = take(D);
    net->off_w_ih = take(4 * D * D);
    net->off_w_hh = take(4 * D * D);
    net->off_b_ih = take(4 * D);
    net->off_b_hh = take(4 * D);
    net->off_head1_w = take(D * D);
    net->off_head1_b = take(D);
    net->off_head2_w = take(A * D);
    net->off_head2_b = take(A);
    net->n_trainable = pos;
    net->n_theta = pos;
    pos = 0;
    net->rec_x = take(D);
    net->rec_gates = take(4 * D);
    net->rec_c = take(D);
    net->rec_h = take(D);
    net->rec_z1 = take(D);
    net->rec_e = net->discrete ? take(net->kep) : -1;
    net->rec_row = pos;
    pos = 0;
    net->grec_dh = take(D);
    net->grec_dg = take(4 * D);
    net->grec_dz1 = take(D);
    net->grec_dx = take(D);
    net->grec_de = net->discrete ? take(net->kep) : -1;
    net->grec_row = pos;
    return DTQN_OK;
}

extern "C" long long dtqn_drqn_workspace_floats(const DrqnNet* net, int batch, int n, int training) {
    if (!drqn_net_ok(net) || batch < 1 || n < 1 || n > net->ctx_len) return 0;
    const long long M = (long long)batch * n;
    return (long long)drqn_hdr_floats(batch) + M * net->rec_row + (training ? M * net->grec_row : 0);
}

extern "C" int dtqn_drqn_forward(const DrqnNet* net, const float* theta, const float* obs, const int32_t* lengths, const float* h0,
                                 const float* c0, int batch, int n, float* q_out, float* h_n, float* c_n, float* workspace, void* stream) {
    return drqn_forward_impl(net, theta, obs, lengths, h0, c0, batch, n, q_out, h_n, c_n, workspace, stream, false);
}

extern "C" int dtqn_drqn_forward_train(const DrqnNet* net, const float* theta, const float* obs, const int32_t* lengths, int batch, int n,
                                       float* q_out, float* h_n, float* c_n, float* workspace, void* stream) {
    return drqn_forward_impl(net, theta, obs, lengths, nullptr, nullptr, batch, n, q_out, h_n, c_n, workspace, stream, true);
}

extern "C" int dtqn_drqn_backward(const DrqnNet* net, const float* theta, const float* obs, int batch, int n, const float* dq, float* workspace,
                                  float* grad_out, void* stream) {
    if (!drqn_net_ok(net)) return DTQN_ERR_CONFIG;
    if (!theta || !obs || !dq || !workspace || !grad_out || batch < 1 || n < 1 || n > net->ctx_len) return DTQN_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int D = net->d_model, A = net->num_actions, B = batch, M = B * n, RR = net->rec_row, GR = net->grec_row;
    const int32_t* dlens = reinterpret_cast<const int32_t*>(workspace);
    const float* rec = workspace + drqn_hdr_floats(B);
    float* grec = workspace + drqn_hdr_floats(B) + (size_t)M * RR;
    (void)hipGetLastError();
    if (hipMemsetAsync(grad_out, 0, (size_t)net->n_trainable * sizeof(float), s) != hipSuccess) return DTQN_ERR_LAUNCH;   // (the alignment gaps)
    int rc = DTQN_OK;
    auto run = [&](DrqnGemm g, bool k_tokens, bool shift, const float* fill) {
        if (rc != DTQN_OK) return;
        g.lens = dlens; g.n = n; g.k_tokens = k_tokens ? 1 : 0; g.k_shift = shift ? 1 : 0; g.pad_fill = fill;
        rc = drqn_launch_gemm(g, s);
    };
    auto colsum = [&](const float* Y, long long ld, int N, float* out, float* out2) {
        hipLaunchKernelGGL(drqn_colsum_kernel, dim3((N + 255) / 256), dim3(256), 0, s, Y, ld, M, N, out, out2);
    };
    const float* b1 = theta + net->off_head1_b;
    {   // head: dz1 = (dq W_2) where ReLU passed; dW_2 = dq^T z1, db_2; dh = dz1 W_1; dW_1 = dz1^T h, db_1
        DrqnGemm g = drqn_gemm(dq, A, 1, theta + net->off_head2_w, D, 1, grec + net->grec_dz1, GR, M, D, A);
        g.gate = rec + net->rec_z1; g.ldgate = RR; g.r_tokens = 1;
        run(g, false, false, b1);
        run(drqn_gemm(dq, 1, A, rec + net->rec_z1, RR, 1, grad_out + net->off_head2_w, D, A, D, M), true, false, b1);
        colsum(dq, A, A, grad_out + net->off_head2_b, nullptr);
        run(drqn_gemm(grec + net->grec_dz1, GR, 1, theta + net->off_head1_w, D, 1, grec + net->grec_dh, GR, M, D, D), false, false, nullptr);
        run(drqn_gemm(grec + net->grec_dz1, 1, GR, rec + net->rec_h, RR, 1, grad_out + net->off_head1_w, D, D, D, M), true, false, nullptr);
        colsum(grec + net->grec_dz1, GR, D, grad_out + net->off_head1_b, nullptr);
    }
    if (rc != DTQN_OK) return rc;
    if (D == 64) drqn_launch_bptt<64>(net, theta, rec, grec, dlens, B, n, s);
    else if (D == 128) drqn_launch_bptt<128>(net, theta, rec, grec, dlens, B, n, s);
    else drqn_launch_bptt<256>(net, theta, rec, grec, dlens, B, n, s);
    // LSTM weights: dW_ih = dG^T x, dW_hh = dG^T h_{t-1}, both bias gradients = the column sums of dG
    run(drqn_gemm(grec + net->grec_dg, 1, GR, rec + net->rec_x, RR, 1, grad_out + net->off_w_ih, D, 4 * D, D, M), true, false, nullptr);
    run(drqn_gemm(grec + net->grec_dg, 1, GR, rec + net->rec_h, RR, 1, grad_out + net->off_w_hh, D, 4 * D, D, M), true, true, nullptr);
    colsum(grec + net->grec_dg, GR, 4 * D, grad_out + net->off_b_ih, grad_out + net->off_b_hh);
    // embedding: dx = dG W_ih; dW_obs = dx^T e, db_obs; discrete: de = dx W_obs scattered into the table
    run(drqn_gemm(grec + net->grec_dg, GR, 1, theta + net->off_w_ih, D, 1, grec + net->grec_dx, GR, M, D, 4 * D), false, false, nullptr);
    if (net->discrete)
        run(drqn_gemm(grec + net->grec_dx, 1, GR, rec + net->rec_e, RR, 1, grad_out + net->off_obs_w, net->ke, D, net->ke, M), true, false, nullptr);
    else
        run(drqn_gemm(grec + net->grec_dx, 1, GR, obs, net->obs_dim, 1, grad_out + net->off_obs_w, net->ke, D, net->ke, M), true, false, nullptr);
    colsum(grec + net->grec_dx, GR, D, grad_out + net->off_obs_b, nullptr);
    if (net->discrete) {
        run(drqn_gemm(grec + net->grec_dx, GR, 1, theta + net->off_obs_w, net->ke, 1, grec + net->grec_de, GR, M, net->ke, D), false, false, nullptr);
        const int cells = net->vocab * net->embed_per_obs;
        hipLaunchKernelGGL(drqn_table_grad_kernel, dim3((cells + 255) / 256), dim3(256), 0, s, obs, grec + net->grec_de, (long long)GR, M,
                           net->obs_dim, net->embed_per_obs, net->vocab, grad_out + net->off_obs_tab);
    }
    if (rc != DTQN_OK) return rc;
    return hipGetLastError() == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}
