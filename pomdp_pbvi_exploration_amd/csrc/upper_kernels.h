// Launchers of the HSVI upper bound (pbvi_upper_bound, pbvi_upper_q): the support-restricted sawtooth over a sparse
// point store, and the bound-greedy action values built on it (internal).
#pragma once
#include "backup_kernels.h"

namespace pbvi {

// The device point store as the kernels read it: P points, rows in CSR (ascending state inside a row).
struct UpperStore {
    const int64_t* ptr;        // [P + 1] first entry of every point
    const int32_t* idx;        // [nnz] state of an entry
    const double* val;         // [nnz] its probability (> 0)
    const int32_t* nnz;        // [P] entries of every point
    const double* v;           // [P] the point's value
    const double* gap;         // [P] v - p.c, computed by the caller
    const double* c;           // [S] corner values
};

constexpr int UB_PPB = 64;     // points one block of k_ub_pairs reduces (16 per wave)
inline int upper_chunks(int64_t n_hit) { return (int)((n_hit + UB_PPB - 1) / UB_PPB); }

// Scratch of one sawtooth evaluation of n rows against n_hit points
struct UpperScratch {
    double* v0;                // [n] sum_s b[s] c[s]
    int32_t* bnnz;             // [n] non-zeros of the row, -1 when it holds a NaN
    double* part_w;            // [n][chunks] smallest w of the chunk's visible points (+inf: none)
    int32_t* part_i;           // [n][chunks] the lowest point attaining it
    int32_t* part_h;           // [n][chunks] lowest hit of the chunk's points (INT32_MAX: none)
};

// The sawtooth of every row of `rows` (n rows, ld apart, widened to fp64) over the store:
//   v0 = sum_s b[s] c[s];  r_i = min_{s: p_i[s] > 0} b[s] / p_i[s];  w_i = v0 + gap_i * r_i (two roundings)
//   U = min(v0, min_{i < n_visible} w_i), point = the first i attaining it (-1: v0 <= every w_i)
//   hit = the first i < n_hit with p_i == b;  value = hit >= 0 ? v[hit] : U;  a row with a NaN: value NaN, point = hit = -1
// Three kernels on `st`, no atomics, every reduction in a fixed order (thread-strided sums, the wave's xor butterfly, the
// block's four waves in order, the chunks in order): a row's results do not depend on n or on its place among the rows.
// Results go to row perm[r] (perm == nullptr: r) of out_value / out_point / out_hit (either of the last two may be nullptr).
template <typename T>
hipError_t launch_upper_sawtooth(const T* rows, int ld, int n, int S, const int32_t* perm, UpperStore store, int64_t n_visible,
                                 int64_t n_hit, UpperScratch ws, double* out_value, int32_t* out_point, int32_t* out_hit,
                                 hipStream_t st);

// The successors of pbvi_upper_q are rows of the Bayes step (backup_kernels.h: a BayesStep with every_ao_from, pushed with the
// fixed-order norm and normalised with out_row == nullptr into [rows][S]): mass [B][A][O] is launch_belief_push's, value
// [B][A][O] the sawtooth of the normalised rows.
// Q[b,a] = sum_s b[s] ER[s,a] + gamma * sum_o mass[b,a,o] * value[b,a,o] (sequential over o; mass == 0 adds 0) for engine rows
// b < B, written with p_obs = mass and succ_value = value to the caller's row perm[b]; action = first maximum of the row of Q
// as written (a NaN never wins, a row of NaNs gives 0).  out_action / out_pobs / out_sval may be nullptr.
template <typename T>
hipError_t launch_upper_q_finish(const T* bel, int ldb, int B, ModelView<T> mv, const int32_t* perm, double gamma,
                                 const double* mass, const double* value, double* out_q, int32_t* out_action, double* out_pobs,
                                 double* out_sval, hipStream_t st);

}  // namespace pbvi
