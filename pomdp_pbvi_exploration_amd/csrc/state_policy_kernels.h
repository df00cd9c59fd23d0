// State-policy heuristics (pbvi_state_policy, pbvi_rollout_state_policy): the three policies that act through a per-state
// action table pi(s) instead of value rows -- most likely state, action voting, Thompson sampling.  include/pbvi_hip.h has
// the definition; the arithmetic is a sequential fp64 walk per chunk of 256 states and an in-order combine of the chunks, so
// the results agree bit for bit with pomdp.state_policy_numpy.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pbvi {

enum StatePolicyRule { STATE_POLICY_MLS = 0, STATE_POLICY_VOTING = 1, STATE_POLICY_THOMPSON = 2 };

constexpr int STATE_POLICY_CHUNK = 256;       // states per chunk of the definition
constexpr int STATE_POLICY_MAX_A = 256;       // the table is staged as one byte per state
__host__ __device__ inline int64_t state_policy_chunks(int S) { return ((int64_t)S + STATE_POLICY_CHUNK - 1) / STATE_POLICY_CHUNK; }

// One call on the rows of `bel` (engine order; caller row c = perm ? perm[i] : i).  Every result is written in caller order.
template <typename T>
struct StatePolicy {
    const T* bel;                     // [B][ldb], rows 16-byte aligned (ldb * sizeof(T) a multiple of 16), zero beyond S
    int ldb, B, S, A;
    const int32_t* perm;              // [B] or nullptr
    const int32_t* table;             // [S] state_actions, every entry in [0, A)
    int rule;                         // StatePolicyRule
    // STATE_POLICY_THOMPSON: u of caller row c = uniforms ? uniforms[c]
    //                                          : uniform01(splitmix64(seed, first_id + (orig ? orig[c] : c)), 2^33 + t)
    const double* uniforms;           // [B] caller order, or nullptr
    uint64_t seed, first_id;
    const int32_t* orig;              // [B] caller row -> simulation row of a rollout call, or nullptr
    int64_t t;
    double* chunk_sums;               // [B][ceil(S/256)][2] = (P_c, m_c) per engine row: scratch of STATE_POLICY_THOMPSON
    int32_t* action_out;              // [B]
    int32_t* state_out;               // [B]: s* / -1 / the drawn state
    double* votes_out;                // [B][A], written by STATE_POLICY_VOTING (required for it)
};
// k_state_policy<T, RULE>: one block per belief row, no atomics, each row read once per tile of 8 actions (voting) or once.
template <typename T>
hipError_t launch_state_policy(const StatePolicy<T>& sp, hipStream_t st);

}  // namespace pbvi
