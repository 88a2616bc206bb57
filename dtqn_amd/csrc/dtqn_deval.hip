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
#include "dtqn_deval.hpp"
#include "dtqn_device.hpp"

namespace dtqn {

struct DevalArgs {
    long long* counters;
    double* env_f64;
    int32_t* env_i32;
    int32_t* elapsed;
    double* ep_ret;
    int32_t* episode;
    int32_t* last;
    float* obs_new;
    float *obs_in, *obs_out;
    uint8_t *act_in, *act_out;
    int32_t *len_in, *len_out;
    uint8_t* results;
    const float* q_rows;               // Q of the last live rows: [N][A] (q_seq_rows == 0) or [N][q_seq_rows][A], row len_i - 1
    unsigned long long* status;
    int q_seq_rows;
    int kind, n_envs, cap, pairs, episodes;
    int L, O, A;
    uint32_t seed, key, step;
    PomdpTables pomdp;                 // DTQN_ROLLOUT_POMDP: the packed tables
};

constexpr uint32_t kDevalMix = 0xE7A1u;    // (seed, key) -> the seed of this evaluation's draws
constexpr uint32_t kDevalReset = 0;        // step 0 of an episode: CarFlag side, position (2 draws); Memory shuffle and first card (<= 17)
constexpr uint32_t kDevalCard = 40;        // Memory: the card shown after step t
constexpr uint32_t kDevalPomdpState = 48;  // tabular POMDP: the next state and observation of step t (its reset: kDevalReset, + 1 at step 0)
constexpr uint32_t kDevalPomdpObs = 49;
constexpr uint32_t kDevalPad = 41;         // the action of context row 0 (Context.reset fills its action rows with random draws)

__device__ __forceinline__ uint32_t deval_seed(const DevalArgs& a) { return hash_u32(a.seed, a.key, 0u, kDevalMix); }
// u in [0, 1) from 32 counter-based bits, in DOUBLE: hash * 2^-32 is exact there; in f32 it can round up to 1.0
__device__ __forceinline__ double deval_u(uint32_t s, int t, int episode, uint32_t kind) {
    return (double)hash_u32(s, (uint32_t)t, (uint32_t)episode, kind) * (1.0 / 4294967296.0);
}

__device__ __forceinline__ double deval_f64(long long b) { double d; __builtin_memcpy(&d, &b, 8); return d; }
__device__ __forceinline__ long long deval_bits(double d) { long long b; __builtin_memcpy(&b, &d, 8); return b; }

__device__ __forceinline__ void deval_write_obs(const DevalArgs& a, int i, float* dst) {
    if (a.kind == DTQN_ROLLOUT_CARFLAG) {
        const double* s = a.env_f64 + (size_t)i * 4;
        for (int k = 0; k < 3; ++k) dst[k] = (float)s[k];             // f32 only where the observation is stored
    } else if (a.kind == DTQN_ROLLOUT_POMDP) {
        dst[0] = (float)a.env_i32[(size_t)i * kRolloutEnvInts + 1];
    } else {
        const int32_t* shown = a.env_i32 + (size_t)i * kRolloutEnvInts + 1 + 2 * a.pairs;
        for (int k = 0; k < a.O; ++k) dst[k] = (float)shown[k];
    }
}

// Environment i starts `episode`: state, the first observation -> row 0 of the block a step writes.
__device__ __forceinline__ void deval_start_episode(const DevalArgs& a, int i, int episode) {
    const uint32_t s = deval_seed(a);
    const uint32_t e = (uint32_t)episode;
    if (a.kind == DTQN_ROLLOUT_CARFLAG)
        rollout_carflag_reset(a.env_f64 + (size_t)i * 4, hash_u32(s, 0u, e, kDevalReset), hash_u32(s, 0u, e, kDevalReset + 1),
                              hash_u32(s, 0u, e, kDevalReset + 2));
    else if (a.kind == DTQN_ROLLOUT_POMDP) {
        double* rec = a.env_f64 + (size_t)i * 4;                      // the draws, recorded: [2], [3] those of this reset
        const double u_state = deval_u(s, 0, episode, kDevalReset), u_obs = deval_u(s, 0, episode, kDevalReset + 1);
        rollout_pomdp_reset(a.env_i32 + (size_t)i * kRolloutEnvInts, a.pomdp, u_state, u_obs);
        rec[2] = u_state;
        rec[3] = u_obs;
    } else
        rollout_memory_reset(a.env_i32 + (size_t)i * kRolloutEnvInts, a.pairs, [&](int k) { return deval_u(s, 0, episode, kDevalReset + (uint32_t)k); });
    deval_write_obs(a, i, a.obs_out + (size_t)i * a.L * a.O);
    a.act_out[(size_t)i * a.L] = (uint8_t)(int)(deval_u(s, 0, episode, kDevalPad) * (double)a.A);
    a.len_out[i] = 1;
    a.elapsed[i] = 0;
    a.ep_ret[i] = 0.0;
    a.episode[i] = episode;
}

// Environment i has no episode left: len = 1 and a valid row 0 (the forward addresses row len - 1; a length of 0 never reaches it).
__device__ __forceinline__ void deval_go_idle(const DevalArgs& a, int i) {
    float* row = a.obs_out + (size_t)i * a.L * a.O;
    for (int k = 0; k < a.O; ++k) row[k] = 0.f;
    a.act_out[(size_t)i * a.L] = 0;
    a.len_out[i] = 1;
    a.elapsed[i] = 0;
    a.ep_ret[i] = 0.0;
    a.episode[i] = -1;
}

// Counters -> state and the status record, every granule {word, tag} one system-scope 8-byte store; one thread.  tag: bit 30 | the
// key's low 14 bits | step + 1 (0 for dtqn_deval_begin) -- never 0, and every launch of an evaluation posts another one.
__device__ __forceinline__ void deval_post(const DevalArgs& a, uint32_t step_plus_1, const long long (&vals)[kDevalCounters]) {
    const unsigned long long tag = (unsigned long long)(0x40000000u | ((a.key & 0x3fffu) << 16) | (step_plus_1 & 0xffffu)) << 32;
    for (int k = 0; k < kDevalCounters; ++k) {
        a.counters[k] = vals[k];
        DTQN_SYSTEM_STORE(a.status + 2 * k, tag | ((unsigned long long)vals[k] & 0xffffffffull));
        DTQN_SYSTEM_STORE(a.status + 2 * k + 1, tag | ((unsigned long long)vals[k] >> 32));
    }
}

__global__ __launch_bounds__(DTQN_THREADS) void dtqn_deval_begin_kernel(DevalArgs a) {
    const int tid = (int)threadIdx.x, N = a.n_envs;
    const int playing = N < a.episodes ? N : a.episodes;
    for (int k = tid; k < a.episodes * (kDevalResultBytes / 4); k += DTQN_THREADS) reinterpret_cast<int32_t*>(a.results)[k] = 0;
    for (int i = tid; i < N; i += DTQN_THREADS) {
        if (i < playing) deval_start_episode(a, i, i);
        else deval_go_idle(a, i);
        for (int k = 0; k < a.O; ++k) a.obs_new[(size_t)i * a.O + k] = 0.f;
        int32_t* last = a.last + (size_t)i * kRolloutLastInts;
        for (int k = 0; k < kRolloutLastInts; ++k) last[k] = 0;
        last[0] = last[6] = -1;
    }
    if (tid == 0) {
        const long long vals[kDevalCounters] = {0, 0, 0, 0, deval_bits(0.0), playing, 0, 0};
        deval_post(a, 0u, vals);
    }
}

__global__ __launch_bounds__(DTQN_THREADS) void dtqn_deval_step_kernel(DevalArgs a) {
    const int tid = (int)threadIdx.x, N = a.n_envs, L = a.L, O = a.O, A = a.A;
    // ---- A: greedy action, environment step, time limit, return ---------------------------------------------------------------
    for (int i = tid; i < N; i += DTQN_THREADS) {
        int32_t* last = a.last + (size_t)i * kRolloutLastInts;
        const int episode = a.episode[i];
        if (episode < 0 || episode >= a.episodes) {                   // idle: no step, nothing counted
            for (int k = 0; k < kRolloutLastInts; ++k) last[k] = 0;
            last[0] = last[6] = -1;
            continue;
        }
        int t = a.elapsed[i];                                         // steps so far = the context's timestep
        t = t < 0 ? 0 : (t < a.cap ? t : a.cap - 1);                  // (a state written by dtqn_deval_set_state stays inside the cap)
        int len = t + 1 < L ? t + 1 : L;
        if (a.q_seq_rows > 0 && len > a.q_seq_rows) len = a.q_seq_rows;           // (n_max bounds every live-row count; stay inside q_dev if not)
        const float* q = a.q_rows + (a.q_seq_rows > 0 ? ((size_t)i * a.q_seq_rows + (len - 1)) * A : (size_t)i * A);
        float best = q[0];
        int action = 0;
        for (int k = 1; k < A; ++k) {
            const float v = q[k];
            if (v > best || (v != v && best == best)) { best = v; action = k; }   // first maximum, a NaN counts as it: torch.argmax
        }
        double reward;
        bool done, success;
        if (a.kind == DTQN_ROLLOUT_CARFLAG) {
            rollout_carflag_step(a.env_f64 + (size_t)i * 4, action, reward, done, success);
        } else if (a.kind == DTQN_ROLLOUT_POMDP) {
            double* rec = a.env_f64 + (size_t)i * 4;                  // the draws, recorded: [0], [1] those of this step
            const uint32_t s = deval_seed(a);
            const double u_state = deval_u(s, t, episode, kDevalPomdpState), u_obs = deval_u(s, t, episode, kDevalPomdpObs);
            rollout_pomdp_step(a.env_i32 + (size_t)i * kRolloutEnvInts, a.pomdp, action, u_state, u_obs, reward, done, success);
            rec[0] = u_state;
            rec[1] = u_obs;
        } else {
            rollout_memory_step(a.env_i32 + (size_t)i * kRolloutEnvInts, a.pairs, action, deval_u(deval_seed(a), t, episode, kDevalCard), reward, done, success);
        }
        // gym TimeLimit (time_limit.py): the cap ends the episode; a truncated step counts as not done in the context
        const int steps = t + 1;
        bool truncated = false;
        if (steps >= a.cap) { truncated = !done; done = true; }
        deval_write_obs(a, i, a.obs_new + (size_t)i * O);
        a.elapsed[i] = steps;
        a.ep_ret[i] += reward;
        last[0] = action;
        last[1] = 0;
        last[2] = done ? 1 : 0;
        last[3] = truncated ? 0 : (done ? 1 : 0);
        last[4] = truncated ? 1 : 0;
        last[5] = success ? 1 : 0;
        last[6] = episode;
        last[7] = (int32_t)__float_as_uint((float)reward);
    }
    __syncthreads();
    // ---- B: contexts of the environments that play on: Context.add_transition (utils/context.py:53-70) into the other block; idle
    //         environments: row 0 and len = 1 carried over -----------------------------------------------------------------------------
    for (int idx = tid; idx < N * L; idx += DTQN_THREADS) {
        const int i = idx / L, r = idx - i * L;
        const int32_t* last = a.last + (size_t)i * kRolloutLastInts;
        if (last[2]) continue;                                        // finished: phase D starts a fresh context or an idle one
        float* dst = a.obs_out + ((size_t)i * L + r) * O;
        if (last[6] < 0) {
            if (r == 0) {
                const float* src = a.obs_in + (size_t)i * L * O;
                for (int k = 0; k < O; ++k) dst[k] = src[k];
                a.act_out[(size_t)i * L] = a.act_in[(size_t)i * L];
                a.len_out[i] = 1;
            }
            continue;
        }
        const int ts = a.elapsed[i];                                  // the context's timestep after this transition
        const int newest = ts < L - 1 ? ts : L - 1, shift = ts >= L ? 1 : 0;
        if (r > newest) continue;
        if (r == newest) {
            const float* src = a.obs_new + (size_t)i * O;
            for (int k = 0; k < O; ++k) dst[k] = src[k];
            a.act_out[(size_t)i * L + r] = (uint8_t)last[0];
        } else {
            const float* src = a.obs_in + ((size_t)i * L + r + shift) * O;
            for (int k = 0; k < O; ++k) dst[k] = src[k];
            a.act_out[(size_t)i * L + r] = a.act_in[(size_t)i * L + r + shift];
        }
        if (r == 0) a.len_out[i] = newest + 1;
    }
    // ---- C: thread 0, environments in index order: results rows and the counters -------------------------------------------------
    long long finished = 0, steps = 0, successes = 0, len_sum = 0, live = 0;
    double ret_sum = 0.0;
    if (tid == 0) {
        finished = a.counters[0]; steps = a.counters[1]; successes = a.counters[2]; len_sum = a.counters[3];
        ret_sum = deval_f64(a.counters[4]);
        for (int i = 0; i < N; ++i) {
            const int32_t* last = a.last + (size_t)i * kRolloutLastInts;
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
        const int32_t* last = a.last + (size_t)i * kRolloutLastInts;
        if (!last[2]) continue;
        const long long next = (long long)last[6] + N;
        if (next < (long long)a.episodes) deval_start_episode(a, i, (int)next);
        else deval_go_idle(a, i);
    }
    // ---- E: counters and the status record -----------------------------------------------------------------------------------------
    if (tid == 0) {
        const long long vals[kDevalCounters] = {finished, steps, successes, len_sum, deval_bits(ret_sum), live, (long long)a.step + 1, 0};
        deval_post(a, a.step + 1u, vals);
    }
}

static DevalArgs deval_args(const DtqnNet* net, const DtqnEval* ev, uint32_t key, int cur, int episodes) {
    const DevalLayout l = deval_layout(net, ev);
    uint8_t* base = static_cast<uint8_t*>(ev->state);
    const ActorBlock in = actor_block(net, base + l.off[8 + (cur & 1)], ev->n_envs), out = actor_block(net, base + l.off[8 + ((cur & 1) ^ 1)], ev->n_envs);
    DevalArgs a{};
    a.counters = reinterpret_cast<long long*>(base + l.off[0]);
    a.env_f64 = reinterpret_cast<double*>(base + l.off[1]);
    a.env_i32 = reinterpret_cast<int32_t*>(base + l.off[2]);
    a.elapsed = reinterpret_cast<int32_t*>(base + l.off[3]);
    a.ep_ret = reinterpret_cast<double*>(base + l.off[4]);
    a.episode = reinterpret_cast<int32_t*>(base + l.off[5]);
    a.last = reinterpret_cast<int32_t*>(base + l.off[6]);
    a.obs_new = reinterpret_cast<float*>(base + l.off[7]);
    a.obs_in = in.obs; a.act_in = in.actions; a.len_in = in.lens;
    a.obs_out = out.obs; a.act_out = out.actions; a.len_out = out.lens;
    a.results = base + l.off[10];
    a.status = static_cast<unsigned long long*>(ev->status_host);
    a.kind = ev->env_kind; a.n_envs = ev->n_envs; a.cap = ev->max_episode_steps; a.pairs = ev->num_pairs; a.episodes = episodes;
    a.L = net->ctx_len; a.O = net->obs_dim; a.A = net->num_actions;
    a.seed = ev->seed; a.key = key;
    if (ev->env_kind == DTQN_ROLLOUT_POMDP)
        a.pomdp = pomdp_tables(ev->pomdp_tables, ev->pomdp_states, ev->pomdp_actions, ev->pomdp_obs, ev->pomdp_first_obs_action);
    return a;
}

int deval_check(const DtqnNet* net, const DtqnEval* ev) {
    if (!net || !ev || !ev->state || !ev->status_host || ev->n_envs < 1 || ev->max_episodes < 1) return DTQN_ERR_ARG;
    if (net->img_c > 0 || net->bag_size > 0) return DTQN_ERR_CONFIG;
    if (ev->max_episode_steps < 1) return DTQN_ERR_ARG;
    if (ev->env_kind == DTQN_ROLLOUT_CARFLAG) {
        if (net->obs_dim != 3 || net->num_actions != 3) return DTQN_ERR_ARG;
    } else if (ev->env_kind == DTQN_ROLLOUT_MEMORY) {
        if (ev->num_pairs < 1 || 1 + 4 * ev->num_pairs > kRolloutEnvInts) return DTQN_ERR_ARG;
        if (net->obs_dim != 2 * ev->num_pairs || net->num_actions != 2 * ev->num_pairs) return DTQN_ERR_ARG;
    } else if (ev->env_kind == DTQN_ROLLOUT_POMDP) {
        if (pomdp_check(net, ev->pomdp_tables, ev->pomdp_states, ev->pomdp_obs, ev->pomdp_first_obs_action) != DTQN_OK) return DTQN_ERR_ARG;
        if (net->num_actions != ev->pomdp_actions) return DTQN_ERR_ARG;
    } else {
        return DTQN_ERR_ARG;
    }
    if (net->num_actions > 255) return DTQN_ERR_ARG;
    return DTQN_OK;
}

int deval_begin_launch(const DtqnNet* net, const DtqnEval* ev, uint32_t key, int episodes, hipStream_t stream) {
    DevalArgs a = deval_args(net, ev, key, 1, episodes);              // a begin writes the `out` block: block 0
    (void)hipGetLastError();   // drop stale errors left by other users of the runtime
    hipLaunchKernelGGL(dtqn_deval_begin_kernel, dim3(1), dim3(DTQN_THREADS), 0, stream, a);
    return hipGetLastError() == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}

int deval_step_launch(const DtqnNet* net, const DtqnEval* ev, uint32_t key, uint32_t step, int cur, int n_max, int episodes, hipStream_t stream) {
    DevalArgs a = deval_args(net, ev, key, cur, episodes);
    a.step = step;
    a.q_rows = net->tiled ? ev->q_dev : ev->q_last;
    a.q_seq_rows = net->tiled ? n_max : 0;
    if (a.q_rows == nullptr) return DTQN_ERR_ARG;
    (void)hipGetLastError();   // drop stale errors left by other users of the runtime
    hipLaunchKernelGGL(dtqn_deval_step_kernel, dim3(1), dim3(DTQN_THREADS), 0, stream, a);
    return hipGetLastError() == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
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
    if (!host || deval_check(net, ev) != DTQN_OK) return DTQN_ERR_ARG;
    const DevalLayout l = deval_layout(net, ev);
    return hipMemcpyAsync(host, ev->state, l.bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}
extern "C" int dtqn_deval_set_state(const DtqnNet* net, const DtqnEval* ev, const void* host, void* stream) {
    if (!host || deval_check(net, ev) != DTQN_OK) return DTQN_ERR_ARG;
    const DevalLayout l = deval_layout(net, ev);
    return hipMemcpyAsync(ev->state, host, l.bytes, hipMemcpyHostToDevice, (hipStream_t)stream) == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}
