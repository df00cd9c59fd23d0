// gfx950 HIP kernels of the HSVI upper bound: the support-restricted sawtooth over a sparse (CSR) point store
// (pbvi_upper_bound) and the bound-greedy action values of the descent (pbvi_upper_q).  Reference: BeliefValueMapping.evaluate,
// src/pomdp.py:873-895, with the minimum restricted to the support of the point (the reference's 0/0 is NaN on every
// belief that shares a zero with a point), and the action loop of expand_hsvi, src/pomdp.py:1768-1868.
//
// Everything here is bound by gathers and fp64 divisions, not by the matrix cores: one wave walks the non-zeros of one point
// against one belief row, the point's entries read coalesced (int32 state, fp64 value), the row gathered at those states.
// No atomics anywhere; every reduction has a fixed order, so a row's results do not depend on what else is in the launch.
#include "upper_kernels.h"
#include "successor.h"

#include <cstdint>
#include <limits>

namespace pbvi {

namespace {

// v0 + gap * r with both roundings (never one fused multiply-add): the host restatement rounds twice
__device__ __forceinline__ double ub_two_roundings(double v0, double gap, double r) {
#pragma clang fp contract(off)
    const double t = gap * r;
    return v0 + t;
}

constexpr int32_t UB_NONE = std::numeric_limits<int32_t>::max();

}  // namespace

// One block per row: v0 = sum_s b[s] c[s] (thread t sums s = t, t + 256, ... in order, then the block's fixed order), the
// row's non-zeros, and -1 in their place when the row holds a NaN.
template <typename T>
__global__ void __launch_bounds__(256) k_ub_row(const T* __restrict__ rows, int ld, int S, const double* __restrict__ c,
                                                double* __restrict__ v0, int32_t* __restrict__ bnnz) {
    __shared__ double red[4];
    const T* row = rows + (int64_t)blockIdx.x * ld;
    double acc = 0.0, cnt = 0.0, bad = 0.0;
    for (int s = threadIdx.x; s < S; s += 256) {
        const double x = (double)row[s];
        acc += x * c[s];
        if (x != 0.0) cnt += 1.0;
        if (x != x) bad += 1.0;
    }
    const double tot = block_sum(acc, red);
    const double n = block_sum(cnt, red);                // (counts below 2^53 are exact in fp64)
    const double nbad = block_sum(bad, red);
    if (threadIdx.x == 0) {
        v0[blockIdx.x] = tot;
        bnnz[blockIdx.x] = nbad != 0.0 ? -1 : (int32_t)n;
    }
}

// One wave per (row, point): the lanes walk the point's entries 64 at a time and reduce min(b / p) and all(b == p).  A block
// takes UB_PPB consecutive points of one row, wave w the points w, w + 4, ... in ascending order, so "strictly smaller" keeps
// the lowest index inside a wave; the four waves are then combined by (w, index).
template <typename T>
__global__ void __launch_bounds__(256) k_ub_pairs(const T* __restrict__ rows, int ld, UpperStore st, int n_visible, int n_hit,
                                                  int chunks, const double* __restrict__ v0, const int32_t* __restrict__ bnnz,
                                                  double* __restrict__ part_w, int32_t* __restrict__ part_i,
                                                  int32_t* __restrict__ part_h) {
    __shared__ double sw[4];
    __shared__ int32_t si[4], sh[4];
    const int r = blockIdx.x, chunk = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const T* row = rows + (int64_t)r * ld;
    const double base = v0[r];
    const int rn = bnnz[r];
    const double inf = std::numeric_limits<double>::infinity();
    double best_w = inf;
    int32_t best_i = UB_NONE, first_hit = UB_NONE;
    for (int k = 0; k < UB_PPB / 4; ++k) {
        const int i = chunk * UB_PPB + k * 4 + wid;
        if (i >= n_hit) break;                              // (uniform in the wave)
        const int64_t j0 = st.ptr[i], j1 = st.ptr[i + 1];
        double m = inf;
        int same = 1;
        for (int64_t j = j0 + lane; j < j1; j += 64) {
            const double p = st.val[j];
            const double x = (double)row[st.idx[j]];
            const double q = x / p;                         // IEEE fp64 division
            if (q < m) m = q;
            if (x != p) same = 0;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double om = __shfl_xor(m, off, 64);
            if (om < m) m = om;
            same &= __shfl_xor(same, off, 64);
        }
        if (i < n_visible) {
            const double w = ub_two_roundings(base, st.gap[i], m);
            if (w < best_w) {
                best_w = w;
                best_i = i;
            }
        }
        if (same && first_hit == UB_NONE && st.nnz[i] == rn) first_hit = i;
    }
    if (lane == 0) {
        sw[wid] = best_w;
        si[wid] = best_i;
        sh[wid] = first_hit;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double w = sw[0];
        int32_t i = si[0], h = sh[0];
        for (int q = 1; q < 4; ++q) {
            if (sw[q] < w || (sw[q] == w && si[q] < i)) {
                w = sw[q];
                i = si[q];
            }
            if (sh[q] < h) h = sh[q];
        }
        const int64_t at = (int64_t)r * chunks + chunk;
        part_w[at] = w;
        part_i[at] = i;
        part_h[at] = h;
    }
}

// One thread per row: the chunks' minima in chunk order behind v0 (strictly smaller wins: ties go to v0, then to the lowest
// index), the lowest hit, and the value; written to the caller's row.
__global__ void __launch_bounds__(256) k_ub_finish(int n, int chunks, const int32_t* __restrict__ perm,
                                                   const double* __restrict__ v0, const int32_t* __restrict__ bnnz,
                                                   const double* __restrict__ part_w, const int32_t* __restrict__ part_i,
                                                   const int32_t* __restrict__ part_h, const double* __restrict__ v,
                                                   double* __restrict__ out_value, int32_t* __restrict__ out_point,
                                                   int32_t* __restrict__ out_hit) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const int64_t d = perm ? perm[r] : r;
    double u = v0[r];
    int32_t arg = -1, hit = UB_NONE;
    if (bnnz[r] < 0) {
        u = std::numeric_limits<double>::quiet_NaN();
    } else {
        for (int c = 0; c < chunks; ++c) {
            const int64_t at = (int64_t)r * chunks + c;
            const double w = part_w[at];
            if (w < u) {
                u = w;
                arg = part_i[at];
            }
            if (part_h[at] < hit) hit = part_h[at];
        }
        if (hit != UB_NONE) u = v[hit];
    }
    out_value[d] = u;
    if (out_point) out_point[d] = arg;
    if (out_hit) out_hit[d] = hit == UB_NONE ? -1 : hit;
}

template <typename T>
hipError_t launch_upper_sawtooth(const T* rows, int ld, int n, int S, const int32_t* perm, UpperStore store, int64_t n_visible,
                                 int64_t n_hit, UpperScratch ws, double* out_value, int32_t* out_point, int32_t* out_hit,
                                 hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const int chunks = upper_chunks(n_hit);
    if (S > ld || n_visible < 0 || n_visible > n_hit || n_hit > 0x7fffffff || chunks > 65535 || out_value == nullptr)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ub_row<T>, dim3(n), dim3(256), 0, st, rows, ld, S, store.c, ws.v0, ws.bnnz);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (chunks > 0) {
        hipLaunchKernelGGL(k_ub_pairs<T>, dim3(n, chunks), dim3(256), 0, st, rows, ld, store, (int)n_visible, (int)n_hit, chunks,
                           ws.v0, ws.bnnz, ws.part_w, ws.part_i, ws.part_h);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ub_finish, dim3((n + 255) / 256), dim3(256), 0, st, n, chunks, perm, ws.v0, ws.bnnz, ws.part_w, ws.part_i,
                       ws.part_h, store.v, out_value, out_point, out_hit);
    return hipGetLastError();
}

// ------------------------------------------------------------------------- //
// pbvi_upper_q: the successors come from the Bayes-step launchers (launch_belief_push over every (a, o), launch_belief_norm);
// their values from the sawtooth above; this folds them into Q.
// ------------------------------------------------------------------------- //
// One block per belief (engine row b, caller row d = perm[b]).  Per action the immediate reward b . ER[:, a] in the block's
// fixed order, then thread 0 adds the observations in order and writes the row; it takes the row's first maximum last.
template <typename T>
__global__ void __launch_bounds__(256) k_upper_q_finish(const T* __restrict__ bel, int ldb, ModelView<T> mv,
                                                        const int32_t* __restrict__ perm, double gamma,
                                                        const double* __restrict__ mass, const double* __restrict__ value,
                                                        double* out_q, int32_t* __restrict__ out_action,
                                                        double* __restrict__ out_pobs, double* __restrict__ out_sval) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const int64_t d = perm ? perm[b] : b;
    const T* row = bel + (int64_t)b * ldb;
    for (int a = 0; a < mv.A; ++a) {
        const T* er = mv.er + (int64_t)a * mv.S_pad;
        double acc = 0.0;
        for (int s = threadIdx.x; s < mv.S; s += 256) acc += (double)row[s] * (double)er[s];
        const double rew = block_sum(acc, red);
        if (threadIdx.x == 0) {
            double tail = 0.0;
            for (int o = 0; o < mv.O; ++o) {
                const int64_t k = ((int64_t)b * mv.A + a) * mv.O + o, kd = (d * mv.A + a) * mv.O + o;
                const double Z = mass[k], val = value[k];
                if (Z != 0.0) tail += Z * val;              // an impossible observation adds 0 (its successor is NaN)
                if (out_pobs) out_pobs[kd] = Z;
                if (out_sval) out_sval[kd] = val;
            }
            out_q[d * mv.A + a] = rew + gamma * tail;
        }
    }
    if (threadIdx.x == 0 && out_action != nullptr) {        // (thread 0 wrote the row itself)
        const double* q = out_q + d * mv.A;
        int best = 0;
        double bv = q[0];
        if (bv != bv) bv = -std::numeric_limits<double>::infinity();
        for (int a = 1; a < mv.A; ++a)
            if (q[a] > bv) {
                bv = q[a];
                best = a;
            }
        out_action[d] = best;
    }
}

template <typename T>
hipError_t launch_upper_q_finish(const T* bel, int ldb, int B, ModelView<T> mv, const int32_t* perm, double gamma,
                                 const double* mass, const double* value, double* out_q, int32_t* out_action, double* out_pobs,
                                 double* out_sval, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (mv.S > ldb || out_q == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_upper_q_finish<T>, dim3(B), dim3(256), 0, st, bel, ldb, mv, perm, gamma, mass, value, out_q, out_action,
                       out_pobs, out_sval);
    return hipGetLastError();
}

#define PBVI_UPPER_INST(T)                                                                                                   \
    template hipError_t launch_upper_sawtooth<T>(const T*, int, int, int, const int32_t*, UpperStore, int64_t, int64_t,      \
                                                 UpperScratch, double*, int32_t*, int32_t*, hipStream_t);                    \
    template hipError_t launch_upper_q_finish<T>(const T*, int, int, ModelView<T>, const int32_t*, double, const double*,    \
                                                 const double*, double*, int32_t*, double*, double*, hipStream_t);
PBVI_UPPER_INST(float)
PBVI_UPPER_INST(double)

}  // namespace pbvi
