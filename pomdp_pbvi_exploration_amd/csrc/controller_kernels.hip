// Finite-state controller evaluation: the sweep kernel of pbvi_controller_value_iteration (controller_kernels.h).
//
// One thread per (node tile, state), s fastest across lanes.  The tables are re-tiled rs [A][R][S], rto [A][O][R][S],
// er [A][S], so every table load is coalesced; V is node-major [N][S], so the R gathers V[succ][rs] of one (node, o) fall
// inside one row of 8 * S bytes (cache traffic).  A block belongs to one tile: its action and its O successors per node are
// block-uniform loads, read once per block.  NT nodes of one action share every RTO / rs load; a short tile is a predicate on
// the node count, never padding.  Per node the order of every product and sum is the definition's, un-fused.  Early exit
// and change reduction as in k_vi_sweep and k_fib_sweep (engine.hip).
#include "controller_kernels.h"

namespace pbvi {

namespace {

template <int NT>
__global__ __launch_bounds__(256) void k_controller_sweep(int S, int O, int R, int s_blocks, const int32_t* __restrict__ rs,
                                                          const double* __restrict__ rto, const double* __restrict__ er,
                                                          const int32_t* __restrict__ node_action,
                                                          const int32_t* __restrict__ node_succ,
                                                          const int32_t* __restrict__ tile_first, double gamma, double limit,
                                                          int it, const double* __restrict__ v_in, double* __restrict__ v_out,
                                                          double* __restrict__ changes) {
#pragma clang fp contract(off)   // no FMA fusion: every product and sum rounds like NumPy's separate ufuncs
    if (it > 0 && changes[it - 1] < limit) return;
    __shared__ double red[4];
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
    // block max, then one atomic per block (non-negative doubles order like their bit patterns)
    for (int off = 32; off > 0; off >>= 1) diff = fmax(diff, __shfl_xor(diff, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = diff;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        atomicMax(reinterpret_cast<unsigned long long*>(&changes[it]), (unsigned long long)__double_as_longlong(mx));
    }
}

}  // namespace

hipError_t launch_controller_sweep(const ControllerSweep& cs, hipStream_t st) {
    const int s_blocks = (cs.S + 255) / 256;
    auto sweep = cs.node_tile == 1 ? k_controller_sweep<1> : k_controller_sweep<CONTROLLER_NODE_TILE>;
    hipLaunchKernelGGL(sweep, dim3((unsigned)(s_blocks * cs.tiles)), dim3(256), 0, st, cs.S, cs.O, cs.R, s_blocks, cs.rs, cs.rto,
                       cs.er, cs.node_action, cs.node_succ, cs.tile_first, cs.gamma, cs.limit, cs.it, cs.v_in, cs.v_out,
                       cs.changes);
    return hipGetLastError();
}

}  // namespace pbvi
