// Device-resident bags (gfx950): the persistent-memory bag of every environment of the device-resident rollout, kept on the GPU.
//
// Replaces, per vector step of a bag network, the host work of DtqnAgent.observe / _bag_insert (agents/dtqn.py): Context.add_transition's
// evicted pair -> Bag.add, and with a full bag one module forward over K + 1 candidate bags and a blocking .item() per environment.
// Two kernels around the candidate forward (dtqn_api.cpp sequences them behind the rollout's step kernel):
//   dtqn_devbag_stage_kernel   one workgroup.  Reads what the step kernel left -- `last` (did the episode end), `elapsed` (did the window
//                              slide) and row 0 of the block the step READ, the observation the slide evicted -- and per environment
//                              clears the bag, appends the pair, or writes the K + 1 candidate bags and raises `choosing`.
//                              The pair's action is the one Context.add_transition hands its caller: it returns a VIEW of the action
//                              row it then overwrites (utils/context.py:65-67, as the reference's), so the host bag stores the evicted
//                              observation with the action of the step that evicted it.  The device stores the same pair.
//   dtqn_devbag_select_kernel  one workgroup per environment.  scores[c] = mean over the L rows of max_a Q of candidate c, one thread per
//                              candidate summing t ascending in f32 (a fixed order, nothing combined across threads); the first maximum
//                              (torch.argmax) becomes the bag.
// Plain vector stores only; no thread keeps an indexed private array.
#include "dtqn_devbag.hpp"
#include "dtqn_deval.hpp"
#include "dtqn_devenv.hpp"
#include "dtqn_rollout.hpp"

namespace dtqn {

struct DevBagArgs {
    float* bag_obs;                    // [N][K][O]
    uint8_t* bag_act;                  // [N][K]
    int32_t* bag_pos;                  // [N]
    float* cand_obs;                   // [N][K+1][K][O]
    uint8_t* cand_act;                 // [N][K+1][K]
    int32_t* choosing;                 // [N]; inside the stage kernel it carries the environment's operation (kBag*)
    float* scores;                     // [N][K+1]
    int32_t* choice;                   // [N]
    long long* counters;               // [DTQN_DEVBAG_COUNTERS]
    int32_t* seq_ctx;                  // [2][N (K+1)]
    const int32_t* last;               // the rollout's state: [N][kLastInts], [N], and row 0 of the block the step kernel read
    const int32_t* elapsed;
    const float* obs_in;
    const float* q_cand;               // [N (K+1)][L][A]
    float obs_mask;
    int N, K, O, L, A;
    int reset_all, may_choose;
};

constexpr int kBagNone = 0, kBagChoose = 1, kBagClear = 2, kBagAppend = 3;       // (kBagChoose is what `choosing` keeps after the kernel)

// Entries in the bag of environment i, inside [0, K] whatever set_state wrote.
__device__ __forceinline__ int devbag_pos(const DevBagArgs& a, int i) {
    const int p = a.bag_pos[i];
    return p < 0 ? 0 : (p < a.K ? p : a.K);
}
// An action as the action embedding can take it.
__device__ __forceinline__ uint8_t devbag_action(const DevBagArgs& a, int act) { return (uint8_t)(act < 0 ? 0 : (act < a.A ? act : a.A - 1)); }
// The action that goes with the observation environment i evicted: this step's (see the head of the file).
__device__ __forceinline__ uint8_t devbag_evicted_action(const DevBagArgs& a, int i) { return devbag_action(a, a.last[(size_t)i * kLastInts]); }

// One counter of the bag state moves; the select kernel's workgroups share it.  An integer sum: the order of the additions cannot show.
__device__ __forceinline__ void devbag_count(long long* counter) {
#if defined(__HIP__)
    atomicAdd(reinterpret_cast<unsigned long long*>(counter), 1ull);
#else   // the host build of the kernels (tests)
    __atomic_fetch_add(counter, 1ll, __ATOMIC_RELAXED);
#endif
}

__global__ __launch_bounds__(DTQN_THREADS) void dtqn_devbag_stage_kernel(DevBagArgs a) {
    const int tid = (int)threadIdx.x, N = a.N, K = a.K, O = a.O, C = a.K + 1;
    // ---- A: what every environment does in this step; the index table of the candidate forward's embedding --------------------------
    for (int i = tid; i < N; i += DTQN_THREADS) {
        int op = kBagNone;
        if (a.reset_all || a.last[(size_t)i * kLastInts + 2]) op = kBagClear;            // Bag.reset (context_reset)
        else if (a.elapsed[i] >= a.L) op = devbag_pos(a, i) < K ? kBagAppend : (a.may_choose ? kBagChoose : kBagNone);
        a.choosing[i] = op;
    }
    for (int s = tid; s < N * C; s += DTQN_THREADS) {
        a.seq_ctx[s] = s / C;
        a.seq_ctx[(size_t)N * C + s] = 0;
    }
    __syncthreads();
    // ---- B: every thread, entry (environment i, candidate c, bag entry k) ----------------------------------------------------------
    for (long long idx = tid; idx < (long long)N * C * K; idx += DTQN_THREADS) {
        const int k = (int)(idx % K), c = (int)((idx / K) % C), i = (int)(idx / ((long long)K * C));
        const int op = a.choosing[i];
        if (op == kBagNone) continue;
        float* entry = a.bag_obs + ((size_t)i * K + k) * O;
        float* cand = a.cand_obs + (((size_t)i * C + c) * K + k) * O;
        const float* evicted = a.obs_in + (size_t)i * a.L * O;                          // Context.add_transition: the old row 0
        if (op == kBagClear) {
            if (c == 0) {
                for (int o = 0; o < O; ++o) entry[o] = a.obs_mask;
                a.bag_act[(size_t)i * K + k] = 0;
            }
            if (a.reset_all) {                                                         // the slots a candidate forward may read before a choice
                for (int o = 0; o < O; ++o) cand[o] = a.obs_mask;
                a.cand_act[((size_t)i * C + c) * K + k] = 0;
            }
        } else if (op == kBagAppend) {
            if (c == 0 && k == devbag_pos(a, i)) {
                for (int o = 0; o < O; ++o) entry[o] = evicted[o];
                a.bag_act[(size_t)i * K + k] = devbag_evicted_action(a, i);
            }
        } else {                                                                       // candidate c < K: entry c replaced; candidate K: the bag
            for (int o = 0; o < O; ++o) cand[o] = c == k ? evicted[o] : entry[o];
            a.cand_act[((size_t)i * C + c) * K + k] = c == k ? devbag_evicted_action(a, i) : devbag_action(a, a.bag_act[(size_t)i * K + k]);
        }
    }
    __syncthreads();
    // ---- C: the counters (one thread, environment order), then every environment's own words ------------------------------------
    if (tid == 0 && !a.reset_all) {
        long long appends = 0, choices = 0, clears = 0;
        for (int i = 0; i < N; ++i) {
            const int op = a.choosing[i];
            appends += op == kBagAppend ? 1 : 0;
            choices += op == kBagChoose ? 1 : 0;
            clears += op == kBagClear ? 1 : 0;
        }
        a.counters[0] += appends;
        a.counters[1] += choices;
        a.counters[3] += clears;
    }
    __syncthreads();
    for (int i = tid; i < N; i += DTQN_THREADS) {
        const int op = a.choosing[i];
        if (op == kBagClear) a.bag_pos[i] = 0;
        if (op == kBagAppend) a.bag_pos[i] = devbag_pos(a, i) + 1;
        a.choosing[i] = op == kBagChoose ? 1 : 0;
        a.choice[i] = -1;
        if (a.reset_all)
            for (int c = 0; c < C; ++c) a.scores[(size_t)i * C + c] = 0.f;
    }
}

__global__ __launch_bounds__(DTQN_THREADS) void dtqn_devbag_select_kernel(DevBagArgs a) {
    __shared__ float score_l[DTQN_DEVBAG_MAX_CANDIDATES];
    __shared__ int keep_l;
    const int tid = (int)threadIdx.x, i = (int)blockIdx.x, K = a.K, O = a.O, C = a.K + 1, L = a.L, A = a.A;
    if (!a.choosing[i]) return;                                       // the whole workgroup: `choice` is -1 since the stage kernel
    // mean over time of max_a Q (torch.mean(torch.max(q, 2)[0], 1)): candidate c is one thread's, t ascending
    for (int c = tid; c < C; c += DTQN_THREADS) {
        const float* q = a.q_cand + ((size_t)i * C + c) * L * A;
        float sum = 0.f;
        for (int t = 0; t < L; ++t) {
            float m = q[(size_t)t * A];
            for (int k = 1; k < A; ++k) {
                const float v = q[(size_t)t * A + k];
                m = (v > m || v != v) ? v : m;                        // a NaN is the maximum, as in torch.max
            }
            sum += m;
        }
        const float s = sum / (float)L;
        score_l[c] = s;
        a.scores[(size_t)i * C + c] = s;
    }
    __syncthreads();
    if (tid == 0) keep_l = first_argmax(score_l, C);
    __syncthreads();
    const int keep = keep_l;
    if (keep < K) {                                                   // (candidate K is the bag as it is)
        const float* src = a.cand_obs + ((size_t)i * C + keep) * K * O;
        for (int idx = tid; idx < K * O; idx += DTQN_THREADS) a.bag_obs[(size_t)i * K * O + idx] = src[idx];
        for (int k = tid; k < K; k += DTQN_THREADS) a.bag_act[(size_t)i * K + k] = a.cand_act[((size_t)i * C + keep) * K + k];
    }
    if (tid == 0) {
        a.choice[i] = keep;
        a.choosing[i] = 0;
        if (keep == K) devbag_count(a.counters + 2);
    }
}

static DevBagArgs devbag_args(const DtqnNet* net, const DtqnDevBag* bag) {
    const DevBagLayout l = devbag_layout(net, bag);
    uint8_t* base = static_cast<uint8_t*>(bag->state);
    DevBagArgs a{};
    a.bag_obs = reinterpret_cast<float*>(base + l.off[0]);
    a.bag_act = base + l.off[1];
    a.bag_pos = reinterpret_cast<int32_t*>(base + l.off[2]);
    a.cand_obs = reinterpret_cast<float*>(base + l.off[3]);
    a.cand_act = base + l.off[4];
    a.choosing = reinterpret_cast<int32_t*>(base + l.off[5]);
    a.scores = reinterpret_cast<float*>(base + l.off[6]);
    a.choice = reinterpret_cast<int32_t*>(base + l.off[7]);
    a.counters = reinterpret_cast<long long*>(base + l.off[8]);
    a.seq_ctx = reinterpret_cast<int32_t*>(base + l.off[9]);
    a.q_cand = bag->q_cand;
    a.obs_mask = bag->obs_mask;
    a.N = bag->n_envs; a.K = net->bag_size; a.O = net->obs_dim; a.L = net->ctx_len; a.A = net->num_actions;
    return a;
}

// The descriptor against the network and the environment count of the state it rides on.
static int devbag_check_desc(const DtqnNet* net, int n_envs, const DtqnDevBag* bag, bool dropout_ok) {
    if (net->bag_size < 1 || !net->tiled || (net->dropout > 0.f && !dropout_ok) || net->bag_size + 1 > DTQN_DEVBAG_MAX_CANDIDATES) return DTQN_ERR_CONFIG;
    if (!bag->state || !bag->q_cand || !bag->workspace || bag->n_envs < 1 || bag->n_envs != n_envs) return DTQN_ERR_ARG;
    if (!(bag->obs_mask == bag->obs_mask)) return DTQN_ERR_ARG;
    // q_cand's floats and the state's offsets stay inside an int
    if ((long long)bag->n_envs * (net->bag_size + 1) * net->ctx_len * net->num_actions > 0x7fffffffLL) return DTQN_ERR_ARG;
    return devbag_layout(net, bag).bytes > 0x7fffffffull ? DTQN_ERR_ARG : DTQN_OK;
}
int devbag_check(const DtqnNet* net, const DtqnRollout* ro, const DtqnDevBag* bag) {
    if (!net || !ro || !bag) return DTQN_ERR_ARG;
    return devbag_check_desc(net, ro->n_envs, bag, false);
}
int devbag_check_eval(const DtqnNet* net, const DtqnEval* ev, const DtqnDevBag* bag) {
    if (!net || !ev || !bag) return DTQN_ERR_ARG;
    return devbag_check_desc(net, ev->n_envs, bag, true);
}

DevBagViews devbag_views(const DtqnNet* net, const DtqnDevBag* bag) {
    const DevBagArgs a = devbag_args(net, bag);
    return DevBagViews{a.bag_obs, a.cand_obs, a.bag_act, a.cand_act, a.seq_ctx, a.seq_ctx + (size_t)a.N * (a.K + 1)};
}

int devbag_stage_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, const DtqnDevBag* bag, int cur, int reset_all,
                        int may_choose, hipStream_t stream) {
    DevBagArgs a = devbag_args(net, bag);
    const RolloutLayout l = rollout_layout(net, rp, ro);
    uint8_t* base = static_cast<uint8_t*>(ro->state);
    const ActorBlock in = actor_block(net, base + l.off[6 + (cur & 1)], ro->n_envs);
    a.last = reinterpret_cast<const int32_t*>(base + l.off[5]);
    a.elapsed = reinterpret_cast<const int32_t*>(base + l.off[3]);
    a.obs_in = in.obs;
    a.reset_all = reset_all; a.may_choose = may_choose;
    return devenv_launch(dtqn_devbag_stage_kernel, a, stream);
}

int devbag_stage_launch_eval(const DtqnNet* net, const DtqnEval* ev, const DtqnDevBag* bag, int cur, int reset_all, int may_choose,
                             hipStream_t stream) {
    DevBagArgs a = devbag_args(net, bag);
    const DevalLayout l = deval_layout(net, ev);
    uint8_t* base = static_cast<uint8_t*>(ev->state);
    const ActorBlock in = actor_block(net, base + l.off[8 + (cur & 1)], ev->n_envs);
    a.last = reinterpret_cast<const int32_t*>(base + l.off[6]);
    a.elapsed = reinterpret_cast<const int32_t*>(base + l.off[3]);
    a.obs_in = in.obs;
    a.reset_all = reset_all; a.may_choose = may_choose;
    return devenv_launch(dtqn_devbag_stage_kernel, a, stream);
}

int devbag_select_launch(const DtqnNet* net, const DtqnDevBag* bag, hipStream_t stream) {
    const DevBagArgs a = devbag_args(net, bag);
    (void)hipGetLastError();   // drop stale errors left by other users of the runtime
    hipLaunchKernelGGL(dtqn_devbag_select_kernel, dim3(a.N), dim3(DTQN_THREADS), 0, stream, a);
    return hipGetLastError() == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}

}  // namespace dtqn

using namespace dtqn;

extern "C" long long dtqn_devbag_state_bytes(const DtqnNet* net, const DtqnDevBag* bag, int32_t* offsets) {
    if (!net || !bag || bag->n_envs < 1 || net->bag_size < 1 || net->obs_dim < 1) return -1;
    const DevBagLayout l = devbag_layout(net, bag);
    if (l.bytes > 0x7fffffffull) return -1;
    if (offsets != nullptr)
        for (int k = 0; k < DTQN_DEVBAG_OFFSETS; ++k) offsets[k] = (int32_t)l.off[k];
    return (long long)l.bytes;
}

extern "C" int dtqn_devbag_get_state(const DtqnNet* net, const DtqnDevBag* bag, void* host, void* stream) {
    if (!net || !bag || !host || !bag->state || bag->n_envs < 1 || net->bag_size < 1) return DTQN_ERR_ARG;
    return devenv_copy_state(host, bag->state, devbag_layout(net, bag).bytes, hipMemcpyDeviceToHost, stream);
}
extern "C" int dtqn_devbag_set_state(const DtqnNet* net, const DtqnDevBag* bag, const void* host, void* stream) {
    if (!net || !bag || !host || !bag->state || bag->n_envs < 1 || net->bag_size < 1) return DTQN_ERR_ARG;
    return devenv_copy_state(bag->state, host, devbag_layout(net, bag).bytes, hipMemcpyHostToDevice, stream);
}
