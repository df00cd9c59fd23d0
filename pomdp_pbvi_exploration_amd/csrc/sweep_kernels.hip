// The sweep kernels of the handle-free value-iteration entries (sweep_kernels.h): MDP value iteration, the Fast Informed
// Bound and finite-state controller evaluation.  The three differ in what a thread owns; they share how a sweep behind a
// converged one leaves and how a block reports its largest change.
#include "sweep_kernels.h"

namespace pbvi {

namespace {

// Sweep `it` has nothing to do when sweep it-1 already met the change limit.
__device__ __forceinline__ bool sweep_after_converged(const double* __restrict__ changes, double limit, int it) {
    return it > 0 && changes[it - 1] < limit;
}

// changes[it] = max(changes[it], max of `diff` over the block of 256 threads): block max, then one atomic per block
// (non-negative doubles order like their bit patterns).  Every thread of the block calls it.
__device__ __forceinline__ void block_change_max(double diff, double* __restrict__ changes, int it) {
    __shared__ double red[4];
    for (int off = 32; off > 0; off >>= 1) diff = fmax(diff, __shfl_xor(diff, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = diff;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        atomicMax(reinterpret_cast<unsigned long long*>(&changes[it]), (unsigned long long)__double_as_longlong(m));
    }
}

// --------------------------------------------------------------------------- //
// MDP value iteration (VI_Solver.solve, src/mdp.py:1485-1510).  One thread per state, tables re-tiled [A][R][S] so
// every load is coalesced; HBM/latency-bound (A*R gathers per state per sweep).  Products and sums are kept
// un-fused (fp contract off) so R = 1 reproduces NumPy's  ER + gamma * (P * v)  bit for bit.
// Sweep `it` leaves at once when sweep it-1 already met the change limit, so the host can enqueue sweeps in
// batches without syncing; the rows / values of the converged sweep stay in place.
// --------------------------------------------------------------------------- //
__global__ void k_vi_sweep(int S, int A, int R, const int32_t* __restrict__ rs, const double* __restrict__ prob,
                           const double* __restrict__ er, double gamma, double limit, int it,
                           const double* __restrict__ v_in, double* __restrict__ v_out, double* __restrict__ rows,
                           double* __restrict__ changes) {
#pragma clang fp contract(off)   // no FMA fusion: every product and sum rounds like NumPy's separate ufuncs
    if (sweep_after_converged(changes, limit, it)) return;
    const int s = blockIdx.x * 256 + threadIdx.x;
    double diff = 0.0;
    if (s < S) {
        double best = 0.0;
        for (int a = 0; a < A; ++a) {
            double acc = 0.0;
            for (int r = 0; r < R; ++r) {
                const int64_t k = ((int64_t)a * R + r) * S + s;
                const double t = prob[k] * v_in[rs[k]];
                acc = r == 0 ? t : acc + t;
            }
            const double scaled = gamma * acc;
            const double row = er[(int64_t)a * S + s] + scaled;
            rows[(int64_t)a * S + s] = row;
            best = (a == 0 || row > best) ? row : best;
        }
        v_out[s] = best;
        diff = fabs(best - v_in[s]);
    }
    block_change_max(diff, changes, it);
}

// --------------------------------------------------------------------------- //
// Fast Informed Bound (Hauskrecht 2000): the MDP sweep with the observation kept inside the maximisation,
//   Q'(s,a) = ER[s,a] + gamma * sum_o max_a' sum_r RTO[s,a,o,r] * Q(rs[s,a,r], a')
// One thread per (s, a), s fastest across lanes; tables re-tiled rs [A][R][S], rto [A][O][R][S], er [A][S] so every
// table load is coalesced.  The two Q buffers are state-major [S][A]: the action values of one successor are one
// contiguous segment, gathered R times per (o, tile) (the repeats hit cache).  a' runs in register tiles of TW
// accumulators with the running maximum carried across tiles; the tail tile is bounded, never padded (0 * -inf).
// PAIRS: A is even, so every segment starts 16-byte aligned and no tile ends inside a pair: double2 loads.
// The order of every product and sum is the one pomdp.fib_numpy states, un-fused, so both agree bit for bit on
// finite inputs.
// --------------------------------------------------------------------------- //
template <int TW, bool PAIRS>
__global__ __launch_bounds__(256) void k_fib_sweep(int S, int A, int O, int R, int s_blocks, const int32_t* __restrict__ rs,
                                                   const double* __restrict__ rto, const double* __restrict__ er,
                                                   double gamma, double limit, int it, const double* __restrict__ q_in,
                                                   double* __restrict__ q_out, double* __restrict__ changes) {
#pragma clang fp contract(off)   // no FMA fusion: every product and sum rounds like NumPy's separate ufuncs
    if (sweep_after_converged(changes, limit, it)) return;
    const int a = blockIdx.x / s_blocks;
    const int s = (blockIdx.x - a * s_blocks) * 256 + threadIdx.x;
    double diff = 0.0;
    if (s < S) {
        const int32_t* rs_a = rs + (int64_t)a * R * S + s;
        double tot = 0.0;
        for (int o = 0; o < O; ++o) {
            const double* rto_ao = rto + ((int64_t)a * O + o) * R * S + s;
            double m = 0.0;                                     // (set by the first accumulator, never compared before)
            for (int a0 = 0; a0 < A; a0 += TW) {
                const int n = min(TW, A - a0);
                double acc[TW];
                for (int r = 0; r < R; ++r) {
                    const double p = rto_ao[(int64_t)r * S];
                    const double* q = q_in + (int64_t)rs_a[(int64_t)r * S] * A + a0;
                    double v[TW];
                    if constexpr (PAIRS) {
#pragma unroll
                        for (int j = 0; j < TW; j += 2)
                            if (j < n) {
                                const double2 t = *reinterpret_cast<const double2*>(q + j);
                                v[j] = t.x;
                                v[j + 1] = t.y;
                            }
                    } else {
#pragma unroll
                        for (int j = 0; j < TW; ++j)
                            if (j < n) v[j] = q[j];
                    }
#pragma unroll
                    for (int j = 0; j < TW; ++j)
                        if (j < n) {
                            const double t = p * v[j];
                            acc[j] = r == 0 ? t : acc[j] + t;
                        }
                }
#pragma unroll
                for (int j = 0; j < TW; ++j)
                    if (j < n) m = (a0 + j == 0 || acc[j] > m) ? acc[j] : m;
            }
            tot = o == 0 ? m : tot + m;
        }
        const double scaled = gamma * tot;
        const double q_new = er[(int64_t)a * S + s] + scaled;
        q_out[(int64_t)s * A + a] = q_new;
        diff = fabs(q_new - q_in[(int64_t)s * A + a]);
    }
    block_change_max(diff, changes, it);
}

// --------------------------------------------------------------------------- //
// Finite-state controller evaluation.  One thread per (node tile, state), s fastest across lanes.  The tables are re-tiled
// rs [A][R][S], rto [A][O][R][S], er [A][S], so every table load is coalesced; V is node-major [N][S], so the R gathers
// V[succ][rs] of one (node, o) fall inside one row of 8 * S bytes (cache traffic).  A block belongs to one tile: its action
// and its O successors per node are block-uniform loads, read once per block.  NT nodes of one action share every RTO / rs
// load; a short tile is a predicate on the node count, never padding.  Per node the order of every product and sum is the
// definition's, un-fused.
// --------------------------------------------------------------------------- //
template <int NT>
__global__ __launch_bounds__(256) void k_controller_sweep(int S, int O, int R, int s_blocks, const int32_t* __restrict__ rs,
                                                          const double* __restrict__ rto, const double* __restrict__ er,
                                                          const int32_t* __restrict__ node_action,
                                                          const int32_t* __restrict__ node_succ,
                                                          const int32_t* __restrict__ tile_first, double gamma, double limit,
                                                          int it, const double* __restrict__ v_in, double* __restrict__ v_out,
                                                          double* __restrict__ changes) {
#pragma clang fp contract(off)   // no FMA fusion: every product and sum rounds like NumPy's separate ufuncs
    if (sweep_after_converged(changes, limit, it)) return;
    const int t = blockIdx.x / s_blocks;
    const int s = (blockIdx.x - t * s_blocks) * 256 + threadIdx.x;
    const int n0 = NT == 1 ? t : tile_first[t];                 // (block-uniform, as are cnt, a and every successor)
    const int cnt = NT == 1 ? 1 : tile_first[t + 1] - n0;
    double diff = 0.0;
    if (s < S) {
        const int a = node_action[n0];
        const int32_t* rs_a = rs + (int64_t)a * R * S + s;
        double tot[NT];
        for (int o = 0; o < O; ++o) {
            const double* rto_ao = rto + ((int64_t)a * O + o) * R * S + s;
            const double* row[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (j < cnt) row[j] = v_in + (int64_t)node_succ[(int64_t)(n0 + j) * O + o] * S;
            double acc[NT];
            for (int r = 0; r < R; ++r) {
                const double p = rto_ao[(int64_t)r * S];
                const int32_t to = rs_a[(int64_t)r * S];
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    if (j < cnt) {
                        const double x = p * row[j][to];
                        acc[j] = r == 0 ? x : acc[j] + x;
                    }
            }
#pragma unroll
            for (int j = 0; j < NT; ++j)
                if (j < cnt) tot[j] = o == 0 ? acc[j] : tot[j] + acc[j];
        }
        const double reward = er[(int64_t)a * S + s];
#pragma unroll
        for (int j = 0; j < NT; ++j)
            if (j < cnt) {
                const double scaled = gamma * tot[j];
                const double v_new = reward + scaled;
                const int64_t k = (int64_t)(n0 + j) * S + s;
                v_out[k] = v_new;
                diff = fmax(diff, fabs(v_new - v_in[k]));
            }
    }
    block_change_max(diff, changes, it);
}

}  // namespace

hipError_t launch_vi_sweep(const ViSweep& vs, hipStream_t st) {
    hipLaunchKernelGGL(k_vi_sweep, dim3((vs.S + 255) / 256), dim3(256), 0, st, vs.S, vs.A, vs.R, vs.rs, vs.rto, vs.er, vs.gamma,
                       vs.limit, vs.it, vs.v_in, vs.v_out, vs.rows, vs.changes);
    return hipGetLastError();
}

hipError_t launch_fib_sweep(const FibSweep& fs, hipStream_t st) {
    auto sweep = fs.A <= 4 ? (fs.A % 2 == 0 ? k_fib_sweep<4, true> : k_fib_sweep<4, false>)
                           : (fs.A % 2 == 0 ? k_fib_sweep<8, true> : k_fib_sweep<8, false>);
    const int s_blocks = (fs.S + 255) / 256;                 // (s_blocks * A <= S * A <= int32)
    hipLaunchKernelGGL(sweep, dim3((unsigned)(s_blocks * fs.A)), dim3(256), 0, st, fs.S, fs.A, fs.O, fs.R, s_blocks, fs.rs,
                       fs.rto, fs.er, fs.gamma, fs.limit, fs.it, fs.q_in, fs.q_out, fs.changes);
    return hipGetLastError();
}

hipError_t launch_controller_sweep(const ControllerSweep& cs, hipStream_t st) {
    const int s_blocks = (cs.S + 255) / 256;
    auto sweep = cs.node_tile == 1 ? k_controller_sweep<1> : k_controller_sweep<CONTROLLER_NODE_TILE>;
    hipLaunchKernelGGL(sweep, dim3((unsigned)(s_blocks * cs.tiles)), dim3(256), 0, st, cs.S, cs.O, cs.R, s_blocks, cs.rs, cs.rto,
                       cs.er, cs.node_action, cs.node_succ, cs.tile_first, cs.gamma, cs.limit, cs.it, cs.v_in, cs.v_out,
                       cs.changes);
    return hipGetLastError();
}

}  // namespace pbvi
