// Device-resident greedy evaluation (gfx950): a quota of episodes played by N CarFlag / Memory / tabular POMDP environments behind the batched actor
// forward, with no host work per step.
//
// Replaces, per vector step, the host work of VectorEvaluator.evaluate (agents/vector.py): the awaited read-back of the greedy
// actions, N numpy environment steps and N contexts re-staged.  The training rollout (dtqn_rollout.hip) cannot do the job with
// epsilon = 0: its environments restart for ever.  Here exactly `episodes` episodes are dealt out in a fixed order -- environment i
// plays episodes i, i + N, ... -- and an environment with none left goes idle.  One workgroup, as the rollout and for its reason:
// the order in which finished episodes are accounted for is a loop order, not a race.
//
// Draws: an episode is a function of (seed, key, episode index) alone -- every draw is hash_u32 of the (seed, key) mix, the step within
// the episode, the episode index and the draw kind; neither the environment slot nor the vector step enters.  The same episode is
// played whatever N plays it.
//
// Phases of dtqn_deval_step_kernel, separated by workgroup barriers (one thread per environment unless noted):
//   A  live environments: first arg-max of the Q row (a NaN counts as the maximum), environment step, time limit, return, the `last`
//      record and the newest observation
//   B  every thread: the contexts of the environments that play on, block `cur` -> block `cur ^ 1` (Context.add_transition); an idle
//      environment is carried over with len = 1 and its row 0.  Thread 0 meanwhile:
//   C  environments in index order: an episode that finished now -> its row of the results table; the counters
//   D  finished environments: episode e + N -- reset and a fresh context if it is inside the quota, idle otherwise
//   E  thread 0: the counters -> state and, as {word, tag} granules of one 8-byte store each, -> the pinned status record
//
// This file holds what is the evaluation's alone: the quota (deal and idle), the results table and its counters.  The environments,
// the draws, the arg-max, the context slide, the `last` record and the status post are those of dtqn_devenv.hpp, shared with the
// rollout.
#include "dtqn_deval.hpp"
#include "dtqn_devenv.hpp"

namespace dtqn {

struct DevalArgs : DevEnvArgs {
    int32_t* episode;                  // [N] the episode in progress, -1 = idle
    float* obs_new;                    // [N][O] the observation the last step returned
    uint8_t* results;
    int episodes;
    uint32_t seed, key, step;
};

constexpr uint32_t kDevalMix = 0xE7A1u;    // (seed, key) -> the seed of this evaluation's draws

// The draws of step t of `episode` (its reset: t = 0, base 0): neither the environment slot nor the vector step enters.
__device__ __forceinline__ DrawKey deval_key(const DevalArgs& a, int t, int episode) {
    return DrawKey{hash_u32(a.seed, a.key, 0u, kDevalMix), (uint32_t)t, (uint32_t)episode};
}

// Environment i after a step it did not take (idle) or before its first: action and episode -1, the rest 0.
__device__ __forceinline__ void deval_blank_last(const DevalArgs& a, int i) {
    int32_t* last = a.last + (size_t)i * kLastInts;
    for (int k = 0; k < kLastInts; ++k) last[k] = 0;
    last[0] = last[6] = -1;
}

// Environment i takes `episode`, or goes idle when the quota has none left: len = 1 and a valid row 0 (the forward addresses row
// len - 1; a length of 0 never reaches it).
__device__ __forceinline__ void deval_deal(const DevalArgs& a, int i, long long episode) {
    if (episode < (long long)a.episodes) {
        env_start(a, i, deval_key(a, 0, (int)episode), 0u);
        a.episode[i] = (int)episode;
        return;
    }
    float* row = a.obs_out + (size_t)i * a.L * a.env.O;
    for (int k = 0; k < a.env.O; ++k) row[k] = 0.f;
    a.act_out[(size_t)i * a.L] = 0;
    a.len_out[i] = 1;
    a.elapsed[i] = 0;
    a.ep_ret[i] = 0.0;
    a.episode[i] = -1;
}

// tag: bit 30 | the key's low 14 bits | step + 1 (0 for dtqn_deval_begin) -- never 0, and every launch of an evaluation posts another one.
__device__ __forceinline__ void deval_post(const DevalArgs& a, uint32_t step_plus_1, const long long (&vals)[kEnvCounters]) {
    env_post(a, 0x40000000u | ((a.key & 0x3fffu) << 16) | (step_plus_1 & 0xffffu), vals);
}

__global__ __launch_bounds__(DTQN_THREADS) void dtqn_deval_begin_kernel(DevalArgs a) {
    const int tid = (int)threadIdx.x, N = a.n_envs;
    for (int k = tid; k < a.episodes * (kDevalResultBytes / 4); k += DTQN_THREADS) reinterpret_cast<int32_t*>(a.results)[k] = 0;
    for (int i = tid; i < N; i += DTQN_THREADS) {
        deval_deal(a, i, i);
        for (int k = 0; k < a.env.O; ++k) a.obs_new[(size_t)i * a.env.O + k] = 0.f;
        deval_blank_last(a, i);
    }
    if (tid == 0) {
        const long long vals[kEnvCounters] = {0, 0, 0, 0, bits_of_f64(0.0), N < a.episodes ? N : a.episodes, 0, 0};
        deval_post(a, 0u, vals);
    }
}

__global__ __launch_bounds__(DTQN_THREADS) void dtqn_deval_step_kernel(DevalArgs a) {
    const int tid = (int)threadIdx.x, N = a.n_envs, L = a.L, O = a.env.O;
    // ---- A: greedy action, environment step, time limit, return ---------------------------------------------------------------
    for (int i = tid; i < N; i += DTQN_THREADS) {
        const int episode = a.episode[i];
        if (episode < 0 || episode >= a.episodes) {                   // idle: no step, nothing counted
            deval_blank_last(a, i);
            continue;
        }
        const int t = env_elapsed(a, i);
        const int action = first_argmax(env_q_row(a, i, t), a.env.A);
        double reward;
        bool done, success;
        a.env.step(i, action, deval_key(a, t, episode), reward, done, success);
        const bool truncated = env_time_limit(a, t + 1, done);        // (a truncated step counts as not done in the context)
        a.env.write_obs(i, a.obs_new + (size_t)i * O);
        env_account(a, i, t + 1, action, 0, done, truncated, success, episode, reward);
    }
    __syncthreads();
    // ---- B: contexts of the environments that play on, into the other block; idle environments: row 0 and len = 1 carried over;
    //         finished ones: phase D starts a fresh context or an idle one ------------------------------------------------------------
    for (int idx = tid; idx < N * L; idx += DTQN_THREADS) {
        const int i = idx / L, r = idx - i * L;
        const int32_t* last = a.last + (size_t)i * kLastInts;
        if (last[2]) continue;
        if (last[6] >= 0) {
            env_slide_row(a, i, r, a.obs_new + (size_t)i * O);
        } else if (r == 0) {
            const float* src = a.obs_in + (size_t)i * L * O;
            float* dst = a.obs_out + (size_t)i * L * O;
            for (int k = 0; k < O; ++k) dst[k] = src[k];
            a.act_out[(size_t)i * L] = a.act_in[(size_t)i * L];
            a.len_out[i] = 1;
        }
    }
    // ---- C: thread 0, environments in index order: results rows and the counters -------------------------------------------------
    long long finished = 0, steps = 0, successes = 0, len_sum = 0, live = 0;
    double ret_sum = 0.0;
    if (tid == 0) {
        finished = a.counters[0]; steps = a.counters[1]; successes = a.counters[2]; len_sum = a.counters[3];
        ret_sum = f64_of_bits(a.counters[4]);
        for (int i = 0; i < N; ++i) {
            const int32_t* last = a.last + (size_t)i * kLastInts;
            const int episode = last[6];
            if (episode < 0) continue;
            steps += 1;
            if (!last[2]) { live += 1; continue; }
            const double ret = a.ep_ret[i];
            const int n = a.elapsed[i], ok = (last[5] || ret > 0.0) ? 1 : 0;
            uint8_t* row = a.results + (size_t)episode * kDevalResultBytes;
            *reinterpret_cast<double*>(row) = ret;
            int32_t* w = reinterpret_cast<int32_t*>(row + 8);
            w[0] = n; w[1] = ok; w[2] = i; w[3] = (int32_t)a.step;
            finished += 1;
            successes += ok;
            len_sum += n;
            ret_sum += ret;
            if ((long long)episode + N < (long long)a.episodes) live += 1;
        }
    }
    __syncthreads();
    // ---- D: what finished takes episode e + N, or goes idle (after C has read its return and length) ------------------------------
    for (int i = tid; i < N; i += DTQN_THREADS) {
        const int32_t* last = a.last + (size_t)i * kLastInts;
        if (!last[2]) continue;
        deval_deal(a, i, (long long)last[6] + N);
    }
    // ---- E: counters and the status record -----------------------------------------------------------------------------------------
    if (tid == 0) {
        const long long vals[kEnvCounters] = {finished, steps, successes, len_sum, bits_of_f64(ret_sum), live, (long long)a.step + 1, 0};
        deval_post(a, a.step + 1u, vals);
    }
}

static DevalArgs deval_args(const DtqnNet* net, const DtqnEval* ev, uint32_t key, int cur, int episodes) {
    const DevalLayout l = deval_layout(net, ev);
    uint8_t* base = static_cast<uint8_t*>(ev->state);
    DevalArgs a{};
    devenv_fill(a, net, ev, l.off, 6, 8, cur);
    a.episode = reinterpret_cast<int32_t*>(base + l.off[5]);
    a.obs_new = reinterpret_cast<float*>(base + l.off[7]);
    a.results = base + l.off[10];
    a.episodes = episodes;
    a.seed = ev->seed; a.key = key;
    return a;
}

static int deval_check_net(const DtqnNet* net, const DtqnEval* ev, int bags) {
    if (!net || !ev || !ev->state || !ev->status_host || ev->n_envs < 1 || ev->max_episodes < 1) return DTQN_ERR_ARG;
    return devenv_check(net, ev, bags);
}
int deval_check(const DtqnNet* net, const DtqnEval* ev) { return deval_check_net(net, ev, 0); }
// The twin that admits a bag network: the bag path's entry points (dtqn_api.cpp) and get_state / set_state, which launch no forward.
int deval_check_bags(const DtqnNet* net, const DtqnEval* ev) { return deval_check_net(net, ev, 1); }

int deval_begin_launch(const DtqnNet* net, const DtqnEval* ev, uint32_t key, int episodes, hipStream_t stream) {
    return devenv_launch(dtqn_deval_begin_kernel, deval_args(net, ev, key, 1, episodes), stream);         // a begin writes the `out` block: block 0
}

int deval_step_launch(const DtqnNet* net, const DtqnEval* ev, uint32_t key, uint32_t step, int cur, int n_max, int episodes, hipStream_t stream) {
    DevalArgs a = deval_args(net, ev, key, cur, episodes);
    a.step = step;
    devenv_q_rows(a, net, ev, n_max);
    if (a.q_rows == nullptr) return DTQN_ERR_ARG;
    return devenv_launch(dtqn_deval_step_kernel, a, stream);
}

}  // namespace dtqn

using namespace dtqn;

extern "C" long long dtqn_deval_state_bytes(const DtqnNet* net, const DtqnEval* ev, int32_t* offsets) {
    if (!net || !ev || ev->n_envs < 1 || ev->max_episodes < 1 || net->obs_dim < 1 || net->ctx_len < 1) return -1;
    const DevalLayout l = deval_layout(net, ev);
    if (l.bytes > 0x7fffffffull) return -1;
    if (offsets != nullptr)
        for (int k = 0; k < DTQN_DEVAL_OFFSETS; ++k) offsets[k] = (int32_t)l.off[k];
    return (long long)l.bytes;
}

extern "C" int dtqn_deval_begin(const DtqnNet* net, const DtqnEval* ev, uint32_t key, int episodes, void* stream) {
    const int rc = deval_check(net, ev);
    if (rc != DTQN_OK) return rc;
    if (episodes < 0 || episodes > ev->max_episodes) return DTQN_ERR_ARG;
    return deval_begin_launch(net, ev, key, episodes, (hipStream_t)stream);
}

extern "C" int dtqn_deval_get_state(const DtqnNet* net, const DtqnEval* ev, void* host, void* stream) {
    if (!host || deval_check_bags(net, ev) != DTQN_OK) return DTQN_ERR_ARG;
    return devenv_copy_state(host, ev->state, deval_layout(net, ev).bytes, hipMemcpyDeviceToHost, stream);
}
extern "C" int dtqn_deval_set_state(const DtqnNet* net, const DtqnEval* ev, const void* host, void* stream) {
    if (!host || deval_check_bags(net, ev) != DTQN_OK) return DTQN_ERR_ARG;
    return devenv_copy_state(ev->state, host, deval_layout(net, ev).bytes, hipMemcpyHostToDevice, stream);
}
