// Device-resident rollout (gfx950): N CarFlag / Memory / tabular POMDP environments stepped behind the batched actor forward.
//
// Replaces, per vector step, the host work of VectorActor.step_all (agents/vector.py): the epsilon-greedy draw, N numpy environment
// steps, N Context.add_transition calls with their re-staging, and the record-by-record replay of finished episodes through
// dtqn_replay_push.  One workgroup: the work is a few hundred bytes per environment, and one workgroup makes the order in which
// finished episodes take their replay slots a loop order instead of a race (no atomic decides placement).
//
// This file holds what is the rollout's alone: epsilon-greedy and forced actions, the staged episodes, the pending ring, the commit
// and its counters.  The environments, the draws, the context slide, the `last` record and the status post are those of
// dtqn_devenv.hpp, shared with the device-resident evaluation (dtqn_deval.hip).
//
// Phases of dtqn_rollout_step_kernel, separated by workgroup barriers (one thread per environment unless noted):
//   A  action (first arg-max of the Q row | counter-based draws | forced), environment step, time limit, the transition -> staging
//   B  every thread: the rolling contexts, block `cur` -> block `cur ^ 1`, slid by one row where the window is full
//   C  every thread: the pending episodes the host has authorised -> replay slot (pos0 + k) mod E, cleansed tail included; then,
//      environments in index order, the episodes that finished in this step -> the pending ring
//   D  finished environments: reset, fresh context (row 0) in block `cur ^ 1`, staging row 0
//   E  cumulative counters -> state and, as {word, tag} granules of one 8-byte store each, -> the pinned status record
#include "dtqn_devenv.hpp"
#include "dtqn_rollout.hpp"

namespace dtqn {

struct RolloutArgs : DevEnvArgs {
    DtqnReplay rp;
    float* stage_obs;                  // the episodes in progress: [N][T+1][O] | [N][T] | [N][T] | [N][T]
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
    const int32_t* forced;
    int have_q, pos0, store;
    uint32_t seed, vstep;
    float epsilon;
};

constexpr uint32_t kDrawExplore = 0, kDrawAction = 1;      // a step's own draws; the reset of an episode it finishes: kDrawReset ..
constexpr uint32_t kDrawReset = 2, kDrawResetAll = 64;     // (dtqn_devenv.hpp lists every draw index)

__device__ __forceinline__ DrawKey rollout_key(const RolloutArgs& a, int i) { return DrawKey{a.seed, a.vstep, (uint32_t)i}; }

// Environment i starts an episode: the fresh context, and its first observation -> staging row 0.
__device__ __forceinline__ void rollout_reset_env(const RolloutArgs& a, int i, uint32_t base) {
    env_start(a, i, rollout_key(a, i), base);
    a.env.write_obs(i, a.stage_obs + (size_t)i * (a.rp.max_steps + 1) * a.env.O);
}

__global__ __launch_bounds__(DTQN_THREADS) void dtqn_rollout_reset_kernel(RolloutArgs a) {
    for (int i = (int)threadIdx.x; i < a.n_envs; i += DTQN_THREADS) {
        rollout_reset_env(a, i, kDrawResetAll);
        for (int k = 0; k < kLastInts; ++k) a.last[(size_t)i * kLastInts + k] = 0;
    }
}

// Pending episodes [committed, upto) -> the replay, by every thread of the workgroup (uniform control flow): store_obs + store x n + the
// slot's cleansed tail (dtqn_replay_apply kind 0) in one pass; episode k since attach takes slot (pos0 + k) mod E.  The HOST chooses
// `upto` from a status record it has seen, so it knows which launch writes the replay (and moves ReplayBuffer.version only then).
__device__ __forceinline__ void rollout_commit_pending(const RolloutArgs& a, long long& committed, long long upto) {
    const int tid = (int)threadIdx.x, O = a.env.O, T = a.rp.max_steps;
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

__device__ __forceinline__ void rollout_post(const RolloutArgs& a, const long long (&vals)[kEnvCounters]) {
    env_post(a, (a.vstep + 1u) & 0x7fffffffu, vals);
}

// The pending episodes up to `authorize` -> the replay, and nothing else (DeviceVectorActor.sync: what finished last is written out).
__global__ __launch_bounds__(DTQN_THREADS) void dtqn_rollout_commit_kernel(RolloutArgs a) {
    long long committed = a.counters[0];
    const long long staged = a.counters[6];
    rollout_commit_pending(a, committed, a.authorize < staged ? a.authorize : staged);
    if (threadIdx.x == 0) {
        const long long vals[kEnvCounters] = {committed, a.counters[1], a.counters[2], a.counters[3], a.counters[4], a.counters[5], staged, a.counters[7]};
        rollout_post(a, vals);
    }
}

__global__ __launch_bounds__(DTQN_THREADS) void dtqn_rollout_step_kernel(RolloutArgs a) {
    const int tid = (int)threadIdx.x, N = a.n_envs, L = a.L, O = a.env.O, A = a.env.A, T = a.rp.max_steps;
    // ---- A: action, environment step, time limit, staging -------------------------------------------------------------------
    for (int i = tid; i < N; i += DTQN_THREADS) {
        const int t = env_elapsed(a, i);
        const DrawKey key = rollout_key(a, i);
        const int forced = a.forced != nullptr ? a.forced[i] : -1;
        const bool random = key.u(kDrawExplore) < (double)a.epsilon || !a.have_q;
        int action;
        if (forced >= 0) action = forced < A ? forced : A - 1;
        else if (random) action = (int)(key.u(kDrawAction) * (double)A);
        else action = first_argmax(env_q_row(a, i, t), A);
        double reward;
        bool done, success;
        a.env.step(i, action, key, reward, done, success);
        const int steps = t + 1;
        const bool truncated = env_time_limit(a, steps, done);
        a.env.write_obs(i, a.stage_obs + ((size_t)i * (T + 1) + steps) * O);
        a.stage_act[(size_t)i * T + t] = (uint8_t)action;
        a.stage_rew[(size_t)i * T + t] = (float)reward;
        a.stage_done[(size_t)i * T + t] = done && !truncated ? 1 : 0;                 // a truncated step is stored as not done (run.py:113)
        env_account(a, i, steps, action, forced < 0 && random ? 1 : 0, done, truncated, success, done ? 1 : 0, reward);
    }
    __syncthreads();
    // ---- B: contexts of the environments that play on, into the other block (finished ones: phase D starts a fresh context) -------
    for (int idx = tid; idx < N * L; idx += DTQN_THREADS) {
        const int i = idx / L, r = idx - i * L;
        if (!a.last[(size_t)i * kLastInts + 2]) env_slide_row(a, i, r, a.stage_obs + ((size_t)i * (T + 1) + a.elapsed[i]) * O);
    }
    // ---- C: authorised pending episodes -> the replay; what finished now -> the pending ring, in environment order; accounting ----
    long long committed = a.counters[0], steps = a.counters[1], successes = a.counters[2], finished = a.counters[3], len_sum = a.counters[4];
    long long staged = a.counters[6], dropped = a.counters[7];
    double ret_sum = f64_of_bits(a.counters[5]);
    steps += N;
    rollout_commit_pending(a, committed, a.authorize < staged ? a.authorize : staged);
    for (int i = 0; i < N; ++i) {                                     // uniform control flow: every thread reads the same flags
        const int32_t* last = a.last + (size_t)i * kLastInts;
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
        if (a.last[(size_t)i * kLastInts + 2]) rollout_reset_env(a, i, kDrawReset);
    // ---- E: counters and the status record ------------------------------------------------------------------------------------
    if (tid == 0) {
        const long long vals[kEnvCounters] = {committed, steps, successes, finished, len_sum, bits_of_f64(ret_sum), staged, dropped};
        rollout_post(a, vals);
    }
}

static RolloutArgs rollout_args(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, int cur) {
    const RolloutLayout l = rollout_layout(net, rp, ro);
    uint8_t* base = static_cast<uint8_t*>(ro->state);
    RolloutArgs a{};
    devenv_fill(a, net, ro, l.off, 5, 6, cur);
    a.rp = *rp;
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
    a.pos0 = ro->pos0;
    a.seed = ro->seed; a.vstep = vstep;
    return a;
}

// The environment check, then what is the rollout's: the replay it writes into, and an episode that fits its staging and its slot.
static int rollout_check_net(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, int bags) {
    if (!net || !rp || !ro || !ro->state || !ro->status_host || ro->n_envs < 1 || ro->pending_slots < 1) return DTQN_ERR_ARG;
    const int rc = devenv_check(net, ro, bags);
    if (rc == DTQN_ERR_CONFIG || rp->obs_u8 != nullptr || !rp->obs || !rp->actions || !rp->rewards || !rp->dones || !rp->ep_len) return DTQN_ERR_CONFIG;
    if (rc != DTQN_OK || rp->obs_dim != net->obs_dim || rp->num_episodes < 1 || ro->pos0 < 0 || ro->max_episode_steps > rp->max_steps) return DTQN_ERR_ARG;
    return DTQN_OK;
}
int rollout_check(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro) { return rollout_check_net(net, rp, ro, 0); }
// The twin that admits a bag network: the bag path's entry points (dtqn_api.cpp) and commit / get_state / set_state, which launch no forward.
int rollout_check_bags(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro) { return rollout_check_net(net, rp, ro, 1); }

int rollout_reset_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, hipStream_t stream) {
    return devenv_launch(dtqn_rollout_reset_kernel, rollout_args(net, rp, ro, vstep, 1), stream);        // a reset writes the `out` block: block 0
}

int rollout_commit_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, long long authorize, hipStream_t stream) {
    RolloutArgs a = rollout_args(net, rp, ro, vstep, 0);
    a.authorize = authorize;
    return devenv_launch(dtqn_rollout_commit_kernel, a, stream);
}

int rollout_step_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, int cur, int n_max, float epsilon,
                        int store, long long authorize, int have_q, hipStream_t stream) {
    RolloutArgs a = rollout_args(net, rp, ro, vstep, cur);
    a.epsilon = epsilon; a.store = store; a.have_q = have_q; a.authorize = authorize;
    devenv_q_rows(a, net, ro, n_max);
    if (have_q && a.q_rows == nullptr) return DTQN_ERR_ARG;
    return devenv_launch(dtqn_rollout_step_kernel, a, stream);
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
    const int rc = rollout_check_bags(net, rp, ro);
    return rc != DTQN_OK ? rc : rollout_commit_launch(net, rp, ro, vstep, authorize, (hipStream_t)stream);
}

extern "C" int dtqn_rollout_get_state(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, void* host, void* stream) {
    if (!host || rollout_check_bags(net, rp, ro) != DTQN_OK) return DTQN_ERR_ARG;
    return devenv_copy_state(host, ro->state, rollout_layout(net, rp, ro).bytes, hipMemcpyDeviceToHost, stream);
}
extern "C" int dtqn_rollout_set_state(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, const void* host, void* stream) {
    if (!host || rollout_check_bags(net, rp, ro) != DTQN_OK) return DTQN_ERR_ARG;
    return devenv_copy_state(ro->state, host, rollout_layout(net, rp, ro).bytes, hipMemcpyHostToDevice, stream);
}
