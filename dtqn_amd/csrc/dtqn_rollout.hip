// Device-resident rollout (gfx950): N CarFlag / Memory / tabular POMDP environments stepped behind the batched actor forward.
//
// Replaces, per vector step, the host work of VectorActor.step_all (agents/vector.py): the epsilon-greedy draw, N numpy environment
// steps, N Context.add_transition calls with their re-staging, and the record-by-record replay of finished episodes through
// dtqn_replay_push.  One workgroup: the work is a few hundred bytes per environment, and one workgroup makes the order in which
// finished episodes take their replay slots a loop order instead of a race (no atomic decides placement).
//
// Phases of dtqn_rollout_step_kernel, separated by workgroup barriers (one thread per environment unless noted):
//   A  action (first arg-max of the Q row | counter-based draws | forced), environment step, time limit, the transition -> staging
//   B  every thread: the rolling contexts, block `cur` -> block `cur ^ 1`, slid by one row where the window is full
//   C  every thread: the pending episodes the host has authorised -> replay slot (pos0 + k) mod E, cleansed tail included; then,
//      environments in index order, the episodes that finished in this step -> the pending ring
//   D  finished environments: reset, fresh context (row 0) in block `cur ^ 1`, staging row 0
//   E  cumulative counters -> state and, as {word, tag} granules of one 8-byte store each, -> the pinned status record
#include "dtqn_device.hpp"
#include "dtqn_rollout.hpp"

namespace dtqn {

struct RolloutArgs {
    DtqnReplay rp;
    long long* counters;
    double* env_f64;
    int32_t* env_i32;
    int32_t* elapsed;
    double* ep_ret;
    int32_t* last;
    float *obs_in, *obs_out;
    uint8_t *act_in, *act_out;
    int32_t *len_in, *len_out;
    float* stage_obs;
    uint8_t* stage_act;
    float* stage_rew;
    uint8_t* stage_done;
    float* pend_obs;                   // finished episodes that wait for the host's go-ahead: [K][T+1][O] | [K][T] | [K][T] | [K][T] | [K]
    uint8_t* pend_act;
    float* pend_rew;
    uint8_t* pend_done;
    int32_t* pend_len;
    long long authorize;               // episodes (counted since attach) this launch may write into the replay
    int pend_slots;
    const float* q_rows;               // Q of the last live rows: [N][A] (q_seq_rows == 0) or [N][q_seq_rows][A], row len_i - 1
    const int32_t* forced;
    unsigned long long* status;
    int q_seq_rows, have_q;
    int kind, n_envs, cap, pairs, pos0, store;
    int L, O, A;
    uint32_t seed, vstep, draw_base;
    float epsilon;
    PomdpTables pomdp;                 // DTQN_ROLLOUT_POMDP: the packed tables
};

// u in [0, 1) from 32 counter-based bits, in DOUBLE: hash * 2^-32 is exact there; in f32 it can round up to 1.0
__device__ __forceinline__ double rollout_u(uint32_t seed, uint32_t vstep, int env, uint32_t draw) {
    return (double)hash_u32(seed, vstep, (uint32_t)env, draw) * (1.0 / 4294967296.0);
}

__device__ __forceinline__ double rollout_f64(long long b) { double d; __builtin_memcpy(&d, &b, 8); return d; }
__device__ __forceinline__ long long rollout_bits(double d) { long long b; __builtin_memcpy(&b, &d, 8); return b; }

constexpr uint32_t kDrawReset = 2;         // draws 0 / 1: explore, random action; 2 ..: the reset of a finished episode
constexpr uint32_t kDrawCard = 40;         // Memory: the next shown card
constexpr uint32_t kDrawPad = 41;          // the action of context row 0 (Context.reset fills its action rows with random draws)
constexpr uint32_t kDrawPomdpState = 48;   // tabular POMDP: the step's next state and observation (its reset: base, base + 1)
constexpr uint32_t kDrawPomdpObs = 49;
constexpr uint32_t kDrawResetAll = 64;     // dtqn_rollout_reset: a range of its own (a step with the same vstep may reset too)

// The first observation of a fresh episode -> staging row 0 and context row 0 of the block a step writes; environment state.
__device__ __forceinline__ void rollout_reset_env(const RolloutArgs& a, int i, uint32_t base) {
    const int O = a.O, L = a.L, T = a.rp.max_steps;
    float* srow = a.stage_obs + (size_t)i * (T + 1) * O;
    float* crow = a.obs_out + (size_t)i * L * O;
    if (a.kind == DTQN_ROLLOUT_CARFLAG) {
        double* s = a.env_f64 + (size_t)i * 4;
        rollout_carflag_reset(s, hash_u32(a.seed, a.vstep, (uint32_t)i, base), hash_u32(a.seed, a.vstep, (uint32_t)i, base + 1),
                              hash_u32(a.seed, a.vstep, (uint32_t)i, base + 2));
        for (int k = 0; k < 3; ++k) srow[k] = crow[k] = (float)s[k];
    } else if (a.kind == DTQN_ROLLOUT_POMDP) {
        int32_t* e = a.env_i32 + (size_t)i * kRolloutEnvInts;
        double* rec = a.env_f64 + (size_t)i * 4;                      // the draws, recorded: [2], [3] those of this reset
        const double u_state = rollout_u(a.seed, a.vstep, i, base), u_obs = rollout_u(a.seed, a.vstep, i, base + 1);
        rollout_pomdp_reset(e, a.pomdp, u_state, u_obs);
        rec[2] = u_state;
        rec[3] = u_obs;
        srow[0] = crow[0] = (float)e[1];
    } else {
        const int C = 2 * a.pairs;
        int32_t* e = a.env_i32 + (size_t)i * kRolloutEnvInts;
        rollout_memory_reset(e, a.pairs, [&](int k) { return rollout_u(a.seed, a.vstep, i, base + (uint32_t)k); });
        const int32_t* shown = e + 1 + C;
        for (int k = 0; k < C; ++k) srow[k] = crow[k] = (float)shown[k];
    }
    a.act_out[(size_t)i * L] = (uint8_t)(int)(rollout_u(a.seed, a.vstep, i, base + kDrawPad) * (double)a.A);
    a.len_out[i] = 1;
    a.elapsed[i] = 0;
    a.ep_ret[i] = 0.0;
}

__global__ __launch_bounds__(DTQN_THREADS) void dtqn_rollout_reset_kernel(RolloutArgs a) {
    for (int i = (int)threadIdx.x; i < a.n_envs; i += DTQN_THREADS) {
        rollout_reset_env(a, i, kDrawResetAll);
        for (int k = 0; k < kRolloutLastInts; ++k) a.last[(size_t)i * kRolloutLastInts + k] = 0;
    }
}

// Pending episodes [committed, upto) -> the replay, by every thread of the workgroup (uniform control flow): store_obs + store x n + the
// slot's cleansed tail (dtqn_replay_apply kind 0) in one pass; episode k since attach takes slot (pos0 + k) mod E.  The HOST chooses
// `upto` from a status record it has seen, so it knows which launch writes the replay (and moves ReplayBuffer.version only then).
__device__ __forceinline__ void rollout_commit_pending(const RolloutArgs& a, long long& committed, long long upto) {
    const int tid = (int)threadIdx.x, O = a.O, T = a.rp.max_steps;
    for (long long e = committed; e < upto; ++e) {
        const int p = (int)(e % a.pend_slots), slot = (int)(((long long)a.pos0 + e) % a.rp.num_episodes);
        int n = a.pend_len[p];
        n = n < 0 ? 0 : (n < T ? n : T);
        float* obs = a.rp.obs + (size_t)slot * (T + 1) * O;
        uint8_t* act = a.rp.actions + (size_t)slot * (T + 1);
        float* rew = a.rp.rewards + (size_t)slot * T;
        uint8_t* don = a.rp.dones + (size_t)slot * T;
        const float* sobs = a.pend_obs + (size_t)p * (T + 1) * O;
        for (int k = tid; k < (T + 1) * O; k += DTQN_THREADS) obs[k] = k < (n + 1) * O ? sobs[k] : a.rp.obs_mask;
        for (int k = tid; k < T + 1; k += DTQN_THREADS) act[k] = k < n ? a.pend_act[(size_t)p * T + k] : (uint8_t)0;
        for (int k = tid; k < T; k += DTQN_THREADS) {
            rew[k] = k < n ? a.pend_rew[(size_t)p * T + k] : 0.f;
            don[k] = k < n ? a.pend_done[(size_t)p * T + k] : (uint8_t)1;
        }
        if (tid == 0) a.rp.ep_len[slot] = n;
        __syncthreads();                                              // (more pending episodes than slots: a later one may take this slot)
    }
    if (upto > committed) committed = upto;
}

// Counters -> state and the status record, every granule {word, tag} one system-scope 8-byte store (agents/dtqn.py _drain_stats); one thread.
__device__ __forceinline__ void rollout_post(const RolloutArgs& a, const long long (&vals)[kRolloutCounters]) {
    const unsigned long long tag = (unsigned long long)((a.vstep + 1u) & 0x7fffffffu) << 32;
    for (int k = 0; k < kRolloutCounters; ++k) {
        a.counters[k] = vals[k];
        DTQN_SYSTEM_STORE(a.status + 2 * k, tag | ((unsigned long long)vals[k] & 0xffffffffull));
        DTQN_SYSTEM_STORE(a.status + 2 * k + 1, tag | ((unsigned long long)vals[k] >> 32));
    }
}

// The pending episodes up to `authorize` -> the replay, and nothing else (DeviceVectorActor.sync: what finished last is written out).
__global__ __launch_bounds__(DTQN_THREADS) void dtqn_rollout_commit_kernel(RolloutArgs a) {
    long long committed = a.counters[0];
    const long long staged = a.counters[6];
    rollout_commit_pending(a, committed, a.authorize < staged ? a.authorize : staged);
    if (threadIdx.x == 0) {
        const long long vals[kRolloutCounters] = {committed, a.counters[1], a.counters[2], a.counters[3], a.counters[4], a.counters[5], staged, a.counters[7]};
        rollout_post(a, vals);
    }
}

__global__ __launch_bounds__(DTQN_THREADS) void dtqn_rollout_step_kernel(RolloutArgs a) {
    const int tid = (int)threadIdx.x, N = a.n_envs, L = a.L, O = a.O, A = a.A, T = a.rp.max_steps;
    // ---- A: action, environment step, time limit, staging -------------------------------------------------------------------
    for (int i = tid; i < N; i += DTQN_THREADS) {
        int t = a.elapsed[i];                                         // steps so far = the context's timestep
        t = t < 0 ? 0 : (t < a.cap ? t : a.cap - 1);                  // (a state written by dtqn_rollout_set_state stays inside the staging)
        const int forced = a.forced != nullptr ? a.forced[i] : -1;
        const bool explore = rollout_u(a.seed, a.vstep, i, 0) < (double)a.epsilon;
        int action;
        if (forced >= 0) {
            action = forced < A ? forced : A - 1;
        } else if (explore || !a.have_q) {
            action = (int)(rollout_u(a.seed, a.vstep, i, 1) * (double)A);
        } else {
            int len = t + 1 < L ? t + 1 : L;
            if (a.q_seq_rows > 0 && len > a.q_seq_rows) len = a.q_seq_rows;       // (n_max bounds every live-row count; stay inside q_dev if not)
            const float* q = a.q_rows + (a.q_seq_rows > 0 ? ((size_t)i * a.q_seq_rows + (len - 1)) * A : (size_t)i * A);
            float best = q[0];
            action = 0;
            for (int k = 1; k < A; ++k)
                if (q[k] > best) { best = q[k]; action = k; }         // first maximum, as torch.argmax
        }
        double reward;
        bool done, success;
        if (a.kind == DTQN_ROLLOUT_CARFLAG) {
            rollout_carflag_step(a.env_f64 + (size_t)i * 4, action, reward, done, success);
        } else if (a.kind == DTQN_ROLLOUT_POMDP) {
            double* rec = a.env_f64 + (size_t)i * 4;                  // the draws, recorded: [0], [1] those of this step
            const double u_state = rollout_u(a.seed, a.vstep, i, kDrawPomdpState), u_obs = rollout_u(a.seed, a.vstep, i, kDrawPomdpObs);
            rollout_pomdp_step(a.env_i32 + (size_t)i * kRolloutEnvInts, a.pomdp, action, u_state, u_obs, reward, done, success);
            rec[0] = u_state;
            rec[1] = u_obs;
        } else {
            rollout_memory_step(a.env_i32 + (size_t)i * kRolloutEnvInts, a.pairs, action, rollout_u(a.seed, a.vstep, i, kDrawCard), reward, done, success);
        }
        // gym TimeLimit (time_limit.py): the cap ends the episode; a truncated step is stored as not done (run.py:113)
        const int steps = t + 1;
        bool truncated = false;
        if (steps >= a.cap) { truncated = !done; done = true; }
        const bool stored_done = truncated ? false : done;
        float* srow = a.stage_obs + ((size_t)i * (T + 1) + steps) * O;
        if (a.kind == DTQN_ROLLOUT_CARFLAG) {
            const double* s = a.env_f64 + (size_t)i * 4;
            for (int k = 0; k < 3; ++k) srow[k] = (float)s[k];        // f32 only where the observation is stored
        } else if (a.kind == DTQN_ROLLOUT_POMDP) {
            srow[0] = (float)a.env_i32[(size_t)i * kRolloutEnvInts + 1];
        } else {
            const int32_t* shown = a.env_i32 + (size_t)i * kRolloutEnvInts + 1 + 2 * a.pairs;
            for (int k = 0; k < O; ++k) srow[k] = (float)shown[k];
        }
        a.stage_act[(size_t)i * T + t] = (uint8_t)action;
        a.stage_rew[(size_t)i * T + t] = (float)reward;
        a.stage_done[(size_t)i * T + t] = stored_done ? 1 : 0;
        a.elapsed[i] = steps;
        a.ep_ret[i] += reward;
        int32_t* last = a.last + (size_t)i * kRolloutLastInts;
        last[0] = action;
        last[1] = forced < 0 && (explore || !a.have_q) ? 1 : 0;
        last[2] = done ? 1 : 0;
        last[3] = stored_done ? 1 : 0;
        last[4] = truncated ? 1 : 0;
        last[5] = success ? 1 : 0;
        last[6] = done ? 1 : 0;
        last[7] = (int32_t)__float_as_uint((float)reward);
    }
    __syncthreads();
    // ---- B: contexts of the environments that play on: Context.add_transition (utils/context.py:53-70) into the other block ------
    // (sliding in place would read rows another thread has already overwritten: the copy is the price, N L (O + 1/4) words)
    for (int idx = tid; idx < N * L; idx += DTQN_THREADS) {
        const int i = idx / L, r = idx - i * L;
        if (a.last[(size_t)i * kRolloutLastInts + 2]) continue;       // finished: phase D starts a fresh context
        const int ts = a.elapsed[i];                                  // the context's timestep after this transition
        const int newest = ts < L - 1 ? ts : L - 1, shift = ts >= L ? 1 : 0;
        if (r > newest) continue;
        float* dst = a.obs_out + ((size_t)i * L + r) * O;
        if (r == newest) {
            const float* src = a.stage_obs + ((size_t)i * (T + 1) + ts) * O;
            for (int k = 0; k < O; ++k) dst[k] = src[k];
            a.act_out[(size_t)i * L + r] = a.stage_act[(size_t)i * T + ts - 1];
        } else {
            const float* src = a.obs_in + ((size_t)i * L + r + shift) * O;
            for (int k = 0; k < O; ++k) dst[k] = src[k];
            a.act_out[(size_t)i * L + r] = a.act_in[(size_t)i * L + r + shift];
        }
        if (r == 0) a.len_out[i] = newest + 1;
    }
    // ---- C: authorised pending episodes -> the replay; what finished now -> the pending ring, in environment order; accounting ----
    long long committed = a.counters[0], steps = a.counters[1], successes = a.counters[2], finished = a.counters[3], len_sum = a.counters[4];
    long long staged = a.counters[6], dropped = a.counters[7];
    double ret_sum = rollout_f64(a.counters[5]);
    steps += N;
    rollout_commit_pending(a, committed, a.authorize < staged ? a.authorize : staged);
    for (int i = 0; i < N; ++i) {                                     // uniform control flow: every thread reads the same flags
        const int32_t* last = a.last + (size_t)i * kRolloutLastInts;
        if (!last[2]) continue;
        const int n = a.elapsed[i];
        finished += 1;
        successes += last[5];
        len_sum += n;
        ret_sum += a.ep_ret[i];
        if (!a.store) continue;
        if (staged - committed >= a.pend_slots) {                     // the host ran further ahead than it promised: counted, never overwritten
            dropped += 1;
            continue;
        }
        const int p = (int)(staged % a.pend_slots);
        staged += 1;
        const float* sobs = a.stage_obs + (size_t)i * (T + 1) * O;
        float* pobs = a.pend_obs + (size_t)p * (T + 1) * O;
        for (int k = tid; k < (n + 1) * O; k += DTQN_THREADS) pobs[k] = sobs[k];
        for (int k = tid; k < n; k += DTQN_THREADS) {
            a.pend_act[(size_t)p * T + k] = a.stage_act[(size_t)i * T + k];
            a.pend_rew[(size_t)p * T + k] = a.stage_rew[(size_t)i * T + k];
            a.pend_done[(size_t)p * T + k] = a.stage_done[(size_t)i * T + k];
        }
        if (tid == 0) a.pend_len[p] = n;
    }
    __syncthreads();
    // ---- D: reset what finished (after C has read its staging) ---------------------------------------------------------------
    for (int i = tid; i < N; i += DTQN_THREADS)
        if (a.last[(size_t)i * kRolloutLastInts + 2]) rollout_reset_env(a, i, kDrawReset);
    // ---- E: counters and the status record ------------------------------------------------------------------------------------
    if (tid == 0) {
        const long long vals[kRolloutCounters] = {committed, steps, successes, finished, len_sum, rollout_bits(ret_sum), staged, dropped};
        rollout_post(a, vals);
    }
}

static RolloutArgs rollout_args(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, int cur) {
    const RolloutLayout l = rollout_layout(net, rp, ro);
    uint8_t* base = static_cast<uint8_t*>(ro->state);
    const ActorBlock in = actor_block(net, base + l.off[6 + (cur & 1)], ro->n_envs), out = actor_block(net, base + l.off[6 + ((cur & 1) ^ 1)], ro->n_envs);
    RolloutArgs a{};
    a.rp = *rp;
    a.counters = reinterpret_cast<long long*>(base + l.off[0]);
    a.env_f64 = reinterpret_cast<double*>(base + l.off[1]);
    a.env_i32 = reinterpret_cast<int32_t*>(base + l.off[2]);
    a.elapsed = reinterpret_cast<int32_t*>(base + l.off[3]);
    a.ep_ret = reinterpret_cast<double*>(base + l.off[4]);
    a.last = reinterpret_cast<int32_t*>(base + l.off[5]);
    a.obs_in = in.obs; a.act_in = in.actions; a.len_in = in.lens;
    a.obs_out = out.obs; a.act_out = out.actions; a.len_out = out.lens;
    a.stage_obs = reinterpret_cast<float*>(base + l.off[8]);
    a.stage_act = base + l.off[9];
    a.stage_rew = reinterpret_cast<float*>(base + l.off[10]);
    a.stage_done = base + l.off[11];
    a.pend_obs = reinterpret_cast<float*>(base + l.off[12]);
    a.pend_act = base + l.off[13];
    a.pend_rew = reinterpret_cast<float*>(base + l.off[14]);
    a.pend_done = base + l.off[15];
    a.pend_len = reinterpret_cast<int32_t*>(base + l.off[16]);
    a.pend_slots = ro->pending_slots;
    a.forced = ro->forced_actions;
    a.status = static_cast<unsigned long long*>(ro->status_host);
    a.kind = ro->env_kind; a.n_envs = ro->n_envs; a.cap = ro->max_episode_steps; a.pairs = ro->num_pairs; a.pos0 = ro->pos0;
    a.L = net->ctx_len; a.O = net->obs_dim; a.A = net->num_actions;
    a.seed = ro->seed; a.vstep = vstep;
    if (ro->env_kind == DTQN_ROLLOUT_POMDP)
        a.pomdp = pomdp_tables(ro->pomdp_tables, ro->pomdp_states, ro->pomdp_actions, ro->pomdp_obs, ro->pomdp_first_obs_action);
    return a;
}

int rollout_check(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro) {
    if (!net || !rp || !ro || !ro->state || !ro->status_host || ro->n_envs < 1 || ro->pending_slots < 1) return DTQN_ERR_ARG;
    if (net->img_c > 0 || net->bag_size > 0 || rp->obs_u8 != nullptr || !rp->obs || !rp->actions || !rp->rewards || !rp->dones || !rp->ep_len)
        return DTQN_ERR_CONFIG;
    if (rp->obs_dim != net->obs_dim || rp->num_episodes < 1 || ro->pos0 < 0) return DTQN_ERR_ARG;
    if (ro->max_episode_steps < 1 || ro->max_episode_steps > rp->max_steps) return DTQN_ERR_ARG;     // an episode fits its staging and its slot
    if (ro->env_kind == DTQN_ROLLOUT_CARFLAG) {
        if (net->obs_dim != 3 || net->num_actions != 3) return DTQN_ERR_ARG;
    } else if (ro->env_kind == DTQN_ROLLOUT_MEMORY) {
        if (ro->num_pairs < 1 || 1 + 4 * ro->num_pairs > kRolloutEnvInts) return DTQN_ERR_ARG;
        if (net->obs_dim != 2 * ro->num_pairs || net->num_actions != 2 * ro->num_pairs) return DTQN_ERR_ARG;
    } else if (ro->env_kind == DTQN_ROLLOUT_POMDP) {
        if (pomdp_check(net, ro->pomdp_tables, ro->pomdp_states, ro->pomdp_obs, ro->pomdp_first_obs_action) != DTQN_OK) return DTQN_ERR_ARG;
        if (net->num_actions != ro->pomdp_actions) return DTQN_ERR_ARG;
    } else {
        return DTQN_ERR_ARG;
    }
    if (net->num_actions > 255) return DTQN_ERR_ARG;
    return DTQN_OK;
}

int rollout_reset_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, hipStream_t stream) {
    RolloutArgs a = rollout_args(net, rp, ro, vstep, 1);              // a reset writes the `out` block: block 0
    (void)hipGetLastError();   // drop stale errors left by other users of the runtime
    hipLaunchKernelGGL(dtqn_rollout_reset_kernel, dim3(1), dim3(DTQN_THREADS), 0, stream, a);
    return hipGetLastError() == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}

int rollout_commit_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, long long authorize, hipStream_t stream) {
    RolloutArgs a = rollout_args(net, rp, ro, vstep, 0);
    a.authorize = authorize;
    (void)hipGetLastError();   // drop stale errors left by other users of the runtime
    hipLaunchKernelGGL(dtqn_rollout_commit_kernel, dim3(1), dim3(DTQN_THREADS), 0, stream, a);
    return hipGetLastError() == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}

int rollout_step_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, int cur, int n_max, float epsilon,
                        int store, long long authorize, int have_q, hipStream_t stream) {
    RolloutArgs a = rollout_args(net, rp, ro, vstep, cur);
    a.epsilon = epsilon; a.store = store; a.have_q = have_q; a.authorize = authorize;
    a.q_rows = net->tiled ? ro->q_dev : ro->q_last;
    a.q_seq_rows = net->tiled ? n_max : 0;
    if (have_q && a.q_rows == nullptr) return DTQN_ERR_ARG;
    (void)hipGetLastError();   // drop stale errors left by other users of the runtime
    hipLaunchKernelGGL(dtqn_rollout_step_kernel, dim3(1), dim3(DTQN_THREADS), 0, stream, a);
    return hipGetLastError() == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}

}  // namespace dtqn

using namespace dtqn;

extern "C" long long dtqn_rollout_state_bytes(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, int32_t* offsets) {
    if (!net || !rp || !ro || ro->n_envs < 1 || ro->pending_slots < 1 || rp->max_steps < 1 || net->obs_dim < 1) return -1;
    const RolloutLayout l = rollout_layout(net, rp, ro);
    if (l.bytes > 0x7fffffffull) return -1;
    if (offsets != nullptr)
        for (int k = 0; k < DTQN_ROLLOUT_OFFSETS; ++k) offsets[k] = (int32_t)l.off[k];
    return (long long)l.bytes;
}

extern "C" long long dtqn_pomdp_table_bytes(int states, int actions, int observations, long long* offsets) {
    if (states < 1 || actions < 1 || observations < 1) return -1;
    const PomdpLayout l = pomdp_layout(states, actions, observations);
    if (offsets != nullptr)
        for (int k = 0; k < DTQN_POMDP_SECTIONS; ++k) offsets[k] = (long long)l.off[k];
    return (long long)l.bytes;
}

extern "C" int dtqn_rollout_reset(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, void* stream) {
    const int rc = rollout_check(net, rp, ro);
    return rc != DTQN_OK ? rc : rollout_reset_launch(net, rp, ro, vstep, (hipStream_t)stream);
}

extern "C" int dtqn_rollout_commit(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, long long authorize, void* stream) {
    const int rc = rollout_check(net, rp, ro);
    return rc != DTQN_OK ? rc : rollout_commit_launch(net, rp, ro, vstep, authorize, (hipStream_t)stream);
}

extern "C" int dtqn_rollout_get_state(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, void* host, void* stream) {
    if (!host || rollout_check(net, rp, ro) != DTQN_OK) return DTQN_ERR_ARG;
    const RolloutLayout l = rollout_layout(net, rp, ro);
    return hipMemcpyAsync(host, ro->state, l.bytes, hipMemcpyDeviceToHost, (hipStream_t)stream) == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}
extern "C" int dtqn_rollout_set_state(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, const void* host, void* stream) {
    if (!host || rollout_check(net, rp, ro) != DTQN_OK) return DTQN_ERR_ARG;
    const RolloutLayout l = rollout_layout(net, rp, ro);
    return hipMemcpyAsync(ro->state, host, l.bytes, hipMemcpyHostToDevice, (hipStream_t)stream) == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}
