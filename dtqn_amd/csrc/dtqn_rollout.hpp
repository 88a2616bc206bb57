// Device-resident rollout: the layout of its one state allocation and the launches dtqn_api.cpp sequences (dtqn_rollout.hip), and
// the one copy of the environment arithmetic: the rollout and the device-resident evaluation (dtqn_deval.hip) both step with it.
#pragma once
#include <hip/hip_runtime.h>

#include "dtqn_actor.hpp"
#include "dtqn_hip.h"

namespace dtqn {

constexpr int kRolloutEnvInts = 40;        // Memory: current card | hidden values [cards] | shown table [cards], cards <= 16
constexpr int kRolloutLastInts = 8;
constexpr int kRolloutCounters = 8;

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
// DTQN_OK when the table fields of a descriptor fit the network: one token per observation, the table's action count, a first-observation
// action inside it.
inline int pomdp_check(const DtqnNet* net, const void* packed, int states, int observations, int first_obs_action) {
    if (packed == nullptr || states < 1 || observations < 1) return DTQN_ERR_ARG;
    if (net->obs_dim != 1 || net->num_actions < 1 || first_obs_action < 0 || first_obs_action >= net->num_actions) return DTQN_ERR_ARG;
    return DTQN_OK;
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

// Byte offsets of the sections of DtqnRollout::state (include/dtqn_hip.h lists them), every section 16-byte aligned.
struct RolloutLayout {
    size_t off[DTQN_ROLLOUT_OFFSETS];
    size_t bytes;
    size_t block_bytes;
};
inline RolloutLayout rollout_layout(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro) {
    RolloutLayout l;
    const int n_envs = ro->n_envs;
    const size_t N = (size_t)n_envs, T = (size_t)rp->max_steps, O = (size_t)net->obs_dim, K = (size_t)ro->pending_slots;
    l.block_bytes = (actor_block(net, nullptr, n_envs).bytes + 15) & ~(size_t)15;
    const size_t sizes[DTQN_ROLLOUT_OFFSETS] = {8 * kRolloutCounters, 8 * N * 4,       4 * N * kRolloutEnvInts, 4 * N,     8 * N, 4 * N * kRolloutLastInts,
                                                l.block_bytes,        l.block_bytes,   4 * N * (T + 1) * O,     N * T,     4 * N * T, N * T,
                                                4 * K * (T + 1) * O,  K * T,           4 * K * T,               K * T,     4 * K};
    size_t at = 0;
    for (int k = 0; k < DTQN_ROLLOUT_OFFSETS; ++k) {
        l.off[k] = at;
        at += (sizes[k] + 15) & ~(size_t)15;
    }
    l.bytes = at;
    return l;
}

// DTQN_OK when the descriptor, the network and the replay fit the kernels (flat f32 observations of the environment's width, ...)
int rollout_check(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro);
int rollout_reset_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, hipStream_t stream);
// q_rows: where the step kernel finds Q of the last live row -- q_last [N][A] (stride 0) or q_dev with n_max rows per sequence
int rollout_step_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, int cur, int n_max, float epsilon,
                        int store, long long authorize, int have_q, hipStream_t stream);
int rollout_commit_launch(const DtqnNet* net, const DtqnReplay* rp, const DtqnRollout* ro, uint32_t vstep, long long authorize, hipStream_t stream);

}  // namespace dtqn
