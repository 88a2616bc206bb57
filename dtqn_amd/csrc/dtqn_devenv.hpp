// Device environments: everything the device-resident rollout (dtqn_rollout.hip) and the device-resident greedy evaluation
// (dtqn_deval.hip) have in common, once.  Bottom up:
//   * the environment arithmetic of CarFlag, Memory and the tabular POMDP (plain pointers in, the uniform draws handed over);
//   * DrawKey: three key words and a draw index -> 32 counter-based bits / u in [0, 1).  The rollout keys it (seed, vector step,
//     environment), the evaluation (mixed seed, step in the episode, episode); the draw indices are one set;
//   * DevEnv: the kernel-side view of the N environments -- reset, step, observation.  The only place that asks which kind it is;
//   * DevEnvArgs and the step bookkeeping on it: clamp of `elapsed`, Q-row address, TimeLimit, the `last` record, the slide of one
//     context row, the fresh context of a new episode, the status post, the f64 bit casts;
//   * host side: devenv_check (the one environment check of a descriptor) and devenv_fill (DevEnvArgs from a state layout).
// A kernel keeps only its own protocol.  Everything on the device is __forceinline__; no thread keeps an indexed private array.
#pragma once
#include <hip/hip_runtime.h>

#include "dtqn_actor.hpp"
#include "dtqn_device.hpp"
#include "dtqn_hip.h"

namespace dtqn {

constexpr int kEnvInts = DTQN_DEVENV_STATE_INTS;   // Memory: current card | hidden values [cards] | shown table [cards], cards <= 16
constexpr int kLastInts = DTQN_DEVENV_LAST_INTS;
constexpr int kEnvCounters = DTQN_ROLLOUT_STATUS_WORDS / 2;        // i64 counters of a state: two {word, tag} granules each in its status record
static_assert(DTQN_DEVAL_STATUS_WORDS == DTQN_ROLLOUT_STATUS_WORDS, "both status records carry kEnvCounters counters");

// ---- environment arithmetic (plain pointers in, the uniform draws handed over by the caller: no key scheme in here) ----------------
constexpr double kMaxPosition = 1.1, kMaxSpeed = 0.07, kPower = 0.0015, kPriest = 0.5, kPriestDelta = 0.2;

// CarFlag.reset (car_flag.py:31-37): the side first (top bit of h_side), then the start position, uniform on [-0.2, 0.2) from the 53
// random bits of (h_hi >> 5, h_lo >> 6).  s: position, velocity, direction, heaven position.
__device__ __forceinline__ void rollout_carflag_reset(double* s, uint32_t h_side, uint32_t h_hi, uint32_t h_lo) {
    const bool right = (h_side >> 31) == 0u;
    const unsigned long long bits = ((unsigned long long)(h_hi >> 5) << 26) | (unsigned long long)(h_lo >> 6);
    const double u = (double)bits * (1.0 / 9007199254740992.0);
    s[0] = -0.2 + 0.4 * u;
    s[1] = 0.0;
    s[2] = 0.0;
    s[3] = right ? 1.0 : -1.0;
}

// Memory.reset (memory_cards.py:29-35): the pairs in order, Fisher-Yates, every card hidden, then the first shown card.
// e: current card | hidden values [cards] | shown table [cards]; u(k) in [0, 1): draw k -- k = cards - 1 .. 1 the shuffle, k = cards the card.
template <class Draw>
__device__ __forceinline__ void rollout_memory_reset(int32_t* e, int pairs, Draw&& u) {
    const int C = 2 * pairs;
    int32_t *hidden = e + 1, *shown = e + 1 + C;
    for (int k = 0; k < C; ++k) { hidden[k] = 1 + k / 2; shown[k] = 0; }
    for (int k = C - 1; k > 0; --k) {
        const int j = (int)(u(k) * (double)(k + 1));
        const int32_t t = hidden[k];
        hidden[k] = hidden[j];
        hidden[j] = t;
    }
    const int cur = (int)(u(C) * (double)C);
    e[0] = cur;
    shown[cur] = hidden[cur];
}

// CarFlag.step (car_flag.py:39-62) in float64, statement by statement.  No contraction: each Python statement rounds once per
// operation.  (force is -1, 0 or 1, so force * POWER is exact and velocity + force * POWER rounds once either way; the pragma keeps
// that true of every other expression here as well.)
__device__ __forceinline__ void rollout_carflag_step(double* s, int action, double& reward, bool& done, bool& success) {
#pragma clang fp contract(off)
    double position = s[0], velocity = s[1];
    const double heaven = s[3], hell = -s[3];
    const double force = (double)(action - 1);
    velocity = velocity + force * kPower;
    velocity = velocity > -kMaxSpeed ? velocity : -kMaxSpeed;            // max(v, -MAX_SPEED), then min(., MAX_SPEED)
    velocity = velocity < kMaxSpeed ? velocity : kMaxSpeed;
    position = position + velocity;
    position = position > -kMaxPosition ? position : -kMaxPosition;
    position = position < kMaxPosition ? position : kMaxPosition;
    if (position == -kMaxPosition && velocity < 0.0) velocity = 0.0;
    done = position >= 1.0 || position <= -1.0;
    reward = 0.0;
    if (heaven > hell) {
        if (position >= heaven) reward = 1.0;
        if (position <= hell) reward = -1.0;
    } else {
        if (position <= heaven) reward = 1.0;
        if (position >= hell) reward = -1.0;
    }
    double direction = 0.0;
    if (kPriest - kPriestDelta <= position && position <= kPriest + kPriestDelta) direction = heaven > hell ? 1.0 : -1.0;
    s[0] = position;
    s[1] = velocity;
    s[2] = direction;
    success = reward > 0.0;
}

// Memory.step (memory_cards.py:37-58).  A card that has left the table still "matches" when its hidden value equals the shown one:
// the comparison is against the hidden values, as in the reference.  The next shown card is the k-th card still on the table, k
// uniform (u_card in [0, 1)): the distribution of the host's rejection loop without its unbounded loop.
__device__ __forceinline__ void rollout_memory_step(int32_t* e, int pairs, int action, double u_card, double& reward, bool& done, bool& success) {
    const int C = 2 * pairs, removed = pairs + 1;
    int32_t *hidden = e + 1, *shown = e + 1 + C;
    const int cur = e[0] < 0 ? 0 : (e[0] < C ? e[0] : C - 1);
    done = false;
    success = false;
    if (action != cur && hidden[action] == shown[cur]) {
        shown[action] = removed;
        shown[cur] = removed;
        reward = 0.0;
        int left = 0;
        for (int k = 0; k < C; ++k) left += shown[k] != removed ? 1 : 0;
        if (left == 0) done = success = true;
    } else {
        shown[cur] = 0;
        reward = -1.0;
    }
    if (!done) {
        int left = 0;
        for (int k = 0; k < C; ++k) left += shown[k] != removed ? 1 : 0;
        int pick = (int)(u_card * (double)left);
        int next = 0;
        for (int k = 0; k < C; ++k)
            if (shown[k] != removed) {
                if (pick == 0) next = k;
                --pick;
            }
        e[0] = next;
        shown[next] = hidden[next];
    }
}

// ---- tabular POMDP (DTQN_ROLLOUT_POMDP): three dense tables and two inverse-CDF draws per step ---------------------------------------
// Byte offsets of the sections of the packed table buffer (DtqnRollout::pomdp_tables, DtqnEval::pomdp_tables), every section 16-byte
// aligned: start_cdf f64[S] | T_cdf f64[A][S][S] | O_cdf f64[A][S][Z] | R f64[A][S][S][Z] | D u8[A][S].  The CDFs are derived once
// on the host (envs/pomdp_file.py): every entry from the last positive probability onward is exactly 1.0.
struct PomdpLayout {
    size_t off[DTQN_POMDP_SECTIONS];
    size_t bytes;
};
inline PomdpLayout pomdp_layout(int states, int actions, int observations) {
    PomdpLayout l;
    const size_t S = (size_t)states, A = (size_t)actions, Z = (size_t)observations;
    const size_t sizes[DTQN_POMDP_SECTIONS] = {8 * S, 8 * A * S * S, 8 * A * S * Z, 8 * A * S * S * Z, A * S};
    size_t at = 0;
    for (int k = 0; k < DTQN_POMDP_SECTIONS; ++k) {
        l.off[k] = at;
        at += (sizes[k] + 15) & ~(size_t)15;
    }
    l.bytes = at;
    return l;
}

struct PomdpTables {
    const double *start_cdf, *t_cdf, *o_cdf, *r;
    const uint8_t* d;
    int S, A, Z, first_obs_action;
};
inline PomdpTables pomdp_tables(const void* packed, int states, int actions, int observations, int first_obs_action) {
    const PomdpLayout l = pomdp_layout(states, actions, observations);
    const uint8_t* base = static_cast<const uint8_t*>(packed);
    PomdpTables t;
    t.start_cdf = reinterpret_cast<const double*>(base + l.off[0]);
    t.t_cdf = reinterpret_cast<const double*>(base + l.off[1]);
    t.o_cdf = reinterpret_cast<const double*>(base + l.off[2]);
    t.r = reinterpret_cast<const double*>(base + l.off[3]);
    t.d = base + l.off[4];
    t.S = states; t.A = actions; t.Z = observations; t.first_obs_action = first_obs_action;
    return t;
}

// The first k with u < cdf[k]: an upper bound with the comparison of np.searchsorted(cdf, u, side="right"), clamped to the row (the
// row ends in exactly 1.0 and u < 1, so the clamp never acts on a table built by the parser).  ceil(log2(n + 1)) dependent loads.
__device__ __forceinline__ int rollout_pomdp_draw(const double* cdf, int n, double u) {
    int lo = 0, len = n;
    while (len > 0) {
        const int half = len >> 1;
        const bool right = !(u < cdf[lo + half]);
        lo = right ? lo + half + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    return lo < n ? lo : n - 1;
}

// TabularPOMDP.reset_with (envs/pomdp.py): s0 from `start`, the first observation from O[first_obs_action][s0].  e: state | observation.
__device__ __forceinline__ void rollout_pomdp_reset(int32_t* e, const PomdpTables& t, double u_state, double u_obs) {
    const int s0 = rollout_pomdp_draw(t.start_cdf, t.S, u_state);
    e[0] = s0;
    e[1] = rollout_pomdp_draw(t.o_cdf + ((size_t)t.first_obs_action * t.S + s0) * t.Z, t.Z, u_obs);
}

// TabularPOMDP.step_with: s' from T[a][s], z from O[a][s'], reward R[a][s][s'][z], done D[a][s].  (A state or an action from outside
// -- set_state, a forced action -- is clamped into the tables.)
__device__ __forceinline__ void rollout_pomdp_step(int32_t* e, const PomdpTables& t, int action, double u_state, double u_obs, double& reward,
                                                   bool& done, bool& success) {
    const int s = e[0] < 0 ? 0 : (e[0] < t.S ? e[0] : t.S - 1);
    const int a = action < 0 ? 0 : (action < t.A ? action : t.A - 1);
    const size_t row = (size_t)a * t.S + s;
    const int s2 = rollout_pomdp_draw(t.t_cdf + row * t.S, t.S, u_state);
    const int z = rollout_pomdp_draw(t.o_cdf + ((size_t)a * t.S + s2) * t.Z, t.Z, u_obs);
    reward = t.r[(row * t.S + s2) * t.Z + z];
    done = t.d[row] != 0;
    success = done && reward > 0.0;
    e[0] = s2;
    e[1] = z;
}

// ---- draws -----------------------------------------------------------------------------------------------------------------------------
// Draw indices.  A reset takes base + 0 ..: CarFlag 3 (side, position hi, lo), the POMDP 2 (state, observation), Memory base + 1 ..
// base + cards (<= 16), and base + kDrawPad for the action of context row 0 (Context.reset fills its action rows with random draws).
// The bases: 2 for the reset of an episode that finished in a rollout step (0 / 1 are its explore and random-action draws), 64 for
// dtqn_rollout_reset (a step with the same vstep may reset too), 0 for the evaluation (an episode's first step has a key of its own).
constexpr uint32_t kDrawCard = 40;         // Memory: the next shown card
constexpr uint32_t kDrawPad = 41;
constexpr uint32_t kDrawPomdpState = 48;   // tabular POMDP: the step's next state and observation
constexpr uint32_t kDrawPomdpObs = 49;

struct DrawKey {
    uint32_t a, b, c;
    __device__ __forceinline__ uint32_t bits(uint32_t k) const { return hash_u32(a, b, c, k); }
    // u in [0, 1) from 32 counter-based bits, in DOUBLE: hash * 2^-32 is exact there; in f32 it can round up to 1.0
    __device__ __forceinline__ double u(uint32_t k) const { return (double)bits(k) * (1.0 / 4294967296.0); }
};

// ---- the N environments as a kernel sees them ------------------------------------------------------------------------------------------
struct DevEnv {
    int kind, pairs, O, A;
    double* env_f64;                   // [N][4]   CarFlag: the state; POMDP: the recorded uniforms ([0], [1] the step's, [2], [3] the reset's)
    int32_t* env_i32;                  // [N][kEnvInts]   Memory: the tables; POMDP: state | observation
    PomdpTables pomdp;                 // DTQN_ROLLOUT_POMDP: the packed tables

    __device__ __forceinline__ void reset(int i, const DrawKey& key, uint32_t base) const {
        double* s = env_f64 + (size_t)i * 4;
        int32_t* e = env_i32 + (size_t)i * kEnvInts;
        if (kind == DTQN_ROLLOUT_CARFLAG) {
            rollout_carflag_reset(s, key.bits(base), key.bits(base + 1), key.bits(base + 2));
        } else if (kind == DTQN_ROLLOUT_POMDP) {
            const double u_state = key.u(base), u_obs = key.u(base + 1);
            rollout_pomdp_reset(e, pomdp, u_state, u_obs);
            s[2] = u_state;
            s[3] = u_obs;
        } else {
            rollout_memory_reset(e, pairs, [&](int k) { return key.u(base + (uint32_t)k); });
        }
    }

    __device__ __forceinline__ void step(int i, int action, const DrawKey& key, double& reward, bool& done, bool& success) const {
        double* s = env_f64 + (size_t)i * 4;
        int32_t* e = env_i32 + (size_t)i * kEnvInts;
        if (kind == DTQN_ROLLOUT_CARFLAG) {
            rollout_carflag_step(s, action, reward, done, success);
        } else if (kind == DTQN_ROLLOUT_POMDP) {
            const double u_state = key.u(kDrawPomdpState), u_obs = key.u(kDrawPomdpObs);
            rollout_pomdp_step(e, pomdp, action, u_state, u_obs, reward, done, success);
            s[0] = u_state;
            s[1] = u_obs;
        } else {
            rollout_memory_step(e, pairs, action, key.u(kDrawCard), reward, done, success);
        }
    }

    // The current observation of environment i -> row[O]; f32 only where an observation is stored.
    __device__ __forceinline__ void write_obs(int i, float* row) const {
        if (kind == DTQN_ROLLOUT_CARFLAG) {
            const double* s = env_f64 + (size_t)i * 4;
            for (int k = 0; k < 3; ++k) row[k] = (float)s[k];
        } else if (kind == DTQN_ROLLOUT_POMDP) {
            row[0] = (float)env_i32[(size_t)i * kEnvInts + 1];
        } else {
            const int32_t* shown = env_i32 + (size_t)i * kEnvInts + 1 + 2 * pairs;
            for (int k = 0; k < O; ++k) row[k] = (float)shown[k];
        }
    }
};

// ---- what both step kernels keep per environment, and the bookkeeping on it ------------------------------------------------------------
struct DevEnvArgs {
    DevEnv env;
    long long* counters;               // [kEnvCounters]
    int32_t* elapsed;                  // [N] steps of the episode in progress = the context's timestep
    double* ep_ret;                    // [N]
    int32_t* last;                     // [N][kLastInts]
    float *obs_in, *obs_out;           // the two actor blocks: a step reads `in` and writes `out`
    uint8_t *act_in, *act_out;
    int32_t* len_out;                  // (the lengths of `in` are implied by `elapsed`)
    const float* q_rows;               // Q of the last live rows: [N][A] (q_seq_rows == 0) or [N][q_seq_rows][A], row len_i - 1
    unsigned long long* status;
    int q_seq_rows;
    int n_envs, cap, L;
};

__device__ __forceinline__ double f64_of_bits(long long b) { double d; __builtin_memcpy(&d, &b, 8); return d; }
__device__ __forceinline__ long long bits_of_f64(double d) { long long b; __builtin_memcpy(&b, &d, 8); return b; }

// Steps so far of environment i, inside the cap whatever set_state wrote (so that the staging and the context are never overrun).
__device__ __forceinline__ int env_elapsed(const DevEnvArgs& a, int i) {
    const int t = a.elapsed[i];
    return t < 0 ? 0 : (t < a.cap ? t : a.cap - 1);
}

// The Q row of environment i after t steps: row len - 1 of its sequence (n_max bounds every live-row count; stay inside q_dev if not).
__device__ __forceinline__ const float* env_q_row(const DevEnvArgs& a, int i, int t) {
    const int A = a.env.A;
    int len = t + 1 < a.L ? t + 1 : a.L;
    if (a.q_seq_rows > 0 && len > a.q_seq_rows) len = a.q_seq_rows;
    return a.q_rows + (a.q_seq_rows > 0 ? ((size_t)i * a.q_seq_rows + (len - 1)) * A : (size_t)i * A);
}

// gym TimeLimit (time_limit.py) after `steps` steps: the cap ends the episode; -> truncated (such a step is stored as not done, run.py:113).
__device__ __forceinline__ bool env_time_limit(const DevEnvArgs& a, int steps, bool& done) {
    const bool truncated = steps >= a.cap && !done;
    if (steps >= a.cap) done = true;
    return truncated;
}

// The bookkeeping of one step: elapsed, return and the `last` record (word 1 and word 6 are the kernel's own).
__device__ __forceinline__ void env_account(const DevEnvArgs& a, int i, int steps, int action, int word1, bool done, bool truncated, bool success,
                                            int word6, double reward) {
    a.elapsed[i] = steps;
    a.ep_ret[i] += reward;
    int32_t* last = a.last + (size_t)i * kLastInts;
    last[0] = action;
    last[1] = word1;
    last[2] = done ? 1 : 0;
    last[3] = done && !truncated ? 1 : 0;
    last[4] = truncated ? 1 : 0;
    last[5] = success ? 1 : 0;
    last[6] = word6;
    last[7] = (int32_t)__float_as_uint((float)reward);
}

// Context.add_transition (utils/context.py:53-70) for row r of environment i, block `in` -> block `out`, slid by one row where the
// window is full; the newest row takes `newest_obs` and the action of the `last` record.  (Sliding in place would read rows another
// thread has already overwritten: the copy is the price, N L (O + 1/4) words.)
__device__ __forceinline__ void env_slide_row(const DevEnvArgs& a, int i, int r, const float* newest_obs) {
    const int L = a.L, O = a.env.O;
    const int ts = a.elapsed[i];                                      // the context's timestep after this transition
    const int newest = ts < L - 1 ? ts : L - 1, shift = ts >= L ? 1 : 0;
    if (r > newest) return;
    float* dst = a.obs_out + ((size_t)i * L + r) * O;
    const float* src = r == newest ? newest_obs : a.obs_in + ((size_t)i * L + r + shift) * O;
    for (int k = 0; k < O; ++k) dst[k] = src[k];
    a.act_out[(size_t)i * L + r] = r == newest ? (uint8_t)a.last[(size_t)i * kLastInts] : a.act_in[(size_t)i * L + r + shift];
    if (r == 0) a.len_out[i] = newest + 1;
}

// Environment i starts an episode: reset, the first observation -> row 0 of the block a step writes, the pad action, len = 1.
__device__ __forceinline__ void env_start(const DevEnvArgs& a, int i, const DrawKey& key, uint32_t base) {
    a.env.reset(i, key, base);
    a.env.write_obs(i, a.obs_out + (size_t)i * a.L * a.env.O);
    a.act_out[(size_t)i * a.L] = (uint8_t)(int)(key.u(base + kDrawPad) * (double)a.env.A);
    a.len_out[i] = 1;
    a.elapsed[i] = 0;
    a.ep_ret[i] = 0.0;
}

// Counters -> state and the status record, every granule {word, tag} one system-scope 8-byte store (agents/dtqn.py _drain_stats); one
// thread.  tag32: never 0, and another one with every launch that posts.
__device__ __forceinline__ void env_post(const DevEnvArgs& a, uint32_t tag32, const long long (&vals)[kEnvCounters]) {
    const unsigned long long tag = (unsigned long long)tag32 << 32;
    for (int k = 0; k < kEnvCounters; ++k) {
        a.counters[k] = vals[k];
        DTQN_SYSTEM_STORE(a.status + 2 * k, tag | ((unsigned long long)vals[k] & 0xffffffffull));
        DTQN_SYSTEM_STORE(a.status + 2 * k + 1, tag | ((unsigned long long)vals[k] >> 32));
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
// DTQN_OK when the environment fields of a descriptor (DtqnRollout, DtqnEval: the same names) fit the network: flat f32 observations of
// the environment's width, its action count, at most 255 actions (a u8 per action); DTQN_ERR_CONFIG for an image or a bag network
// (bags != 0: a bag network passes -- the entry points that serve dtqn_devbag.hip's path ask so).
template <class Desc>
inline int devenv_check(const DtqnNet* net, const Desc* d, int bags = 0) {
    if (net->img_c > 0 || (net->bag_size > 0 && !bags)) return DTQN_ERR_CONFIG;
    if (d->max_episode_steps < 1) return DTQN_ERR_ARG;
    if (d->env_kind == DTQN_ROLLOUT_CARFLAG) {
        if (net->obs_dim != 3 || net->num_actions != 3) return DTQN_ERR_ARG;
    } else if (d->env_kind == DTQN_ROLLOUT_MEMORY) {
        if (d->num_pairs < 1 || 1 + 4 * d->num_pairs > kEnvInts) return DTQN_ERR_ARG;
        if (net->obs_dim != 2 * d->num_pairs || net->num_actions != 2 * d->num_pairs) return DTQN_ERR_ARG;
    } else if (d->env_kind == DTQN_ROLLOUT_POMDP) {          // one token per observation, the table's action count, a first-observation action inside it
        if (d->pomdp_tables == nullptr || d->pomdp_states < 1 || d->pomdp_obs < 1 || net->obs_dim != 1 || net->num_actions < 1) return DTQN_ERR_ARG;
        if (d->pomdp_first_obs_action < 0 || d->pomdp_first_obs_action >= net->num_actions || net->num_actions != d->pomdp_actions) return DTQN_ERR_ARG;
    } else {
        return DTQN_ERR_ARG;
    }
    return net->num_actions > 255 ? DTQN_ERR_ARG : DTQN_OK;
}

// The common part of a kernel's arguments from the state's section offsets: sections 0 .. 4 are counters, env_f64, env_i32, elapsed
// and ep_ret in both states; `last` and the two actor blocks sit where the caller says.  A step reads block `cur` and writes the other.
template <class Desc>
inline void devenv_fill(DevEnvArgs& a, const DtqnNet* net, const Desc* d, const size_t* off, int last_section, int block_section, int cur) {
    uint8_t* base = static_cast<uint8_t*>(d->state);
    const ActorBlock in = actor_block(net, base + off[block_section + (cur & 1)], d->n_envs);
    const ActorBlock out = actor_block(net, base + off[block_section + ((cur & 1) ^ 1)], d->n_envs);
    a.counters = reinterpret_cast<long long*>(base + off[0]);
    a.env.env_f64 = reinterpret_cast<double*>(base + off[1]);
    a.env.env_i32 = reinterpret_cast<int32_t*>(base + off[2]);
    a.elapsed = reinterpret_cast<int32_t*>(base + off[3]);
    a.ep_ret = reinterpret_cast<double*>(base + off[4]);
    a.last = reinterpret_cast<int32_t*>(base + off[last_section]);
    a.obs_in = in.obs; a.act_in = in.actions;
    a.obs_out = out.obs; a.act_out = out.actions; a.len_out = out.lens;
    a.status = static_cast<unsigned long long*>(d->status_host);
    a.env.kind = d->env_kind; a.env.pairs = d->num_pairs; a.env.O = net->obs_dim; a.env.A = net->num_actions;
    a.n_envs = d->n_envs; a.cap = d->max_episode_steps; a.L = net->ctx_len;
    if (d->env_kind == DTQN_ROLLOUT_POMDP)
        a.env.pomdp = pomdp_tables(d->pomdp_tables, d->pomdp_states, d->pomdp_actions, d->pomdp_obs, d->pomdp_first_obs_action);
}

// The Q rows a step kernel reads: q_last [N][A] of a whole-sequence network, q_dev with n_max rows per sequence of a row-block one.
template <class Desc>
inline void devenv_q_rows(DevEnvArgs& a, const DtqnNet* net, const Desc* d, int n_max) {
    a.q_rows = net->tiled ? d->q_dev : d->q_last;
    a.q_seq_rows = net->tiled ? n_max : 0;
}

// One launch of a one-workgroup kernel; the whole state to or from host memory.
template <class Kernel, class Args>
inline int devenv_launch(Kernel kernel, const Args& a, hipStream_t stream) {
    (void)hipGetLastError();   // drop stale errors left by other users of the runtime
    hipLaunchKernelGGL(kernel, dim3(1), dim3(DTQN_THREADS), 0, stream, a);
    return hipGetLastError() == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}
inline int devenv_copy_state(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, void* stream) {
    return hipMemcpyAsync(dst, src, bytes, kind, (hipStream_t)stream) == hipSuccess ? DTQN_OK : DTQN_ERR_LAUNCH;
}

}  // namespace dtqn
