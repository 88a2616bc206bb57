// Greedy evaluation on the batched actor (dtqn_actor_greedy_batch, dtqn_img_actor_greedy_batch): the two kernels around the forward.
// An evaluation plays N environments whose episodes end at different times, so some of the N contexts of a step are idle
// (len_i == 0).  The live ones are compacted in environment order in front of the forward, whose grid then covers the live count,
// and behind it one small kernel writes Q of the last live row and its arg-max -- the greedy action (dtqn.py:103) -- for every
// environment into pinned memory: the host reads N ints instead of taking N arg-maxes.
#include "dtqn_actor.hpp"
#include "dtqn_device.hpp"

namespace dtqn {

constexpr int AT = 256;                  // threads per workgroup

#define ACTOR_LAUNCH(kernel, grid, stream, args)                                           \
    do {                                                                                   \
        (void)hipGetLastError();                                                           \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(AT), 0, stream, args);                 \
        if (hipGetLastError() != hipSuccess) return DTQN_ERR_LAUNCH;                       \
    } while (0)

struct ActorCompactArgs {
    const float* obs_h;        // pinned host block, read in place (device-mapped, like dtqn_replay_push): [N][L O] f32
    const uint8_t* act_h;      // [N][L] u8
    const int32_t* lens_h;     // [N], 0 = idle
    float* obs_d;              // the same layout, sequences 0 .. live - 1
    uint8_t* act_d;
    int32_t* lens_d;
    int n_envs, L, O, n_max, blocks_per_env;
};
// blocks_per_env workgroups per environment.  Each counts the live environments in front of its own (a fixed-order sum in LDS: the
// sequence its environment becomes), an idle one leaves, a live one moves its share of the n_max rows the forward reads.
__global__ __launch_bounds__(AT) void actor_compact_kernel(ActorCompactArgs a) {
    __shared__ int32_t sums[AT];
    const int t = (int)threadIdx.x;
    const int i = (int)blockIdx.x / a.blocks_per_env, blk = (int)blockIdx.x - i * a.blocks_per_env;
    int c = 0;
    for (int k = t; k < i; k += AT) c += a.lens_h[k] > 0 ? 1 : 0;
    sums[t] = c;
    __syncthreads();
    for (int off = AT / 2; off > 0; off >>= 1) {
        if (t < off) sums[t] += sums[t + off];
        __syncthreads();
    }
    const int j = sums[0], len = a.lens_h[i];
    if (len <= 0) return;
    const int nf = a.n_max * a.O;
    const float* so = a.obs_h + (size_t)i * a.L * a.O;
    float* dobs = a.obs_d + (size_t)j * a.L * a.O;
    for (int k = blk * AT + t; k < nf; k += a.blocks_per_env * AT) dobs[k] = so[k];
    if (blk == 0) {
        for (int k = t; k < a.n_max; k += AT) a.act_d[(size_t)j * a.L + k] = a.act_h[(size_t)i * a.L + k];
        if (t == 0) a.lens_d[j] = len;
    }
}

struct ActorGreedyArgs {
    const int32_t* lens;       // [N], 0 = idle
    const float* q;            // [live][n_max][A]
    float* q_last;             // [N][A], pinned host memory
    int32_t* action;           // [N], pinned host memory
    int n_envs, n_max, A;
};
// One workgroup: thread t owns a contiguous range of environments, the live counts go through the scan, so environment i finds its
// sequence without a map.  The action is first_argmax of the row (dtqn_actor.hpp).
__global__ __launch_bounds__(AT) void actor_greedy_kernel(ActorGreedyArgs a) {
    __shared__ int32_t sums[AT];
    const int N = a.n_envs, A = a.A, per = (N + AT - 1) / AT;
    const int t = (int)threadIdx.x, i0 = t * per < N ? t * per : N, i1 = i0 + per < N ? i0 + per : N;
    int c = 0;
    for (int i = i0; i < i1; ++i) c += a.lens[i] > 0 ? 1 : 0;
    int j = block_scan_exclusive<AT>(sums, t, c);
    for (int i = i0; i < i1; ++i) {
        const int len = a.lens[i];
        if (len <= 0) {
            a.action[i] = -1;
            continue;
        }
        const float* row = a.q + ((size_t)j * a.n_max + (len - 1)) * A;
        for (int k = 0; k < A; ++k) a.q_last[(size_t)i * A + k] = row[k];
        a.action[i] = first_argmax(row, A);
        ++j;
    }
}

int actor_compact(const DtqnNet* net, const void* ctx_host, void* ctx_dev, int n_envs, int n_max, hipStream_t stream) {
    const int L = net->ctx_len, O = net->obs_dim;
    const ActorBlock h = actor_block(net, ctx_host, n_envs), d = actor_block(net, ctx_dev, n_envs);
    ActorCompactArgs a;
    a.obs_h = h.obs; a.act_h = h.actions; a.lens_h = h.lens;
    a.obs_d = d.obs; a.act_d = d.actions; a.lens_d = d.lens;
    a.n_envs = n_envs; a.L = L; a.O = O; a.n_max = n_max;
    const long long per = ((long long)n_max * O + 4 * AT - 1) / (4 * AT);        // four floats per thread, at most 64 workgroups per environment
    a.blocks_per_env = per < 1 ? 1 : per > 64 ? 64 : (int)per;
    if ((long long)n_envs * a.blocks_per_env > 0x7fffffffLL) return DTQN_ERR_ARG;
    ACTOR_LAUNCH(actor_compact_kernel, n_envs * a.blocks_per_env, stream, a);
    return DTQN_OK;
}

int actor_greedy_rows(const int32_t* lens, const float* q, float* q_last, int32_t* action, int n_envs, int n_max, int A, hipStream_t stream) {
    ActorGreedyArgs a;
    a.lens = lens; a.q = q; a.q_last = q_last; a.action = action; a.n_envs = n_envs; a.n_max = n_max; a.A = A;
    ACTOR_LAUNCH(actor_greedy_kernel, 1, stream, a);
    return DTQN_OK;
}

static int g_last_actor_live = 0;        // live sequences of the last greedy launch (tests: dtqn_debug_last_actor_live)
void set_last_actor_live(int live) { g_last_actor_live = live; }

}  // namespace dtqn

extern "C" int dtqn_debug_last_actor_live(void) { return dtqn::g_last_actor_live; }
