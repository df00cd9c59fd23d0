// The un-normalised Bayes successor, pulled over the inverse transition lists (device code; included by the .hip files):
//   u[s'] = sum over the inverse list of (a, s') of (double) b[s] * (double) RTO[s,a,o,r]
// in list order -- ascending (s, r), np.bincount's accumulation order -- so every kernel that needs u adds the same doubles
// in the same order.  The two functions below are the only readers of the lists (engine.hip::build_inverse_lists:
// in_ptr, [A][S+1], and in_src, [A][S*R], entries e = s * R + r): a change of their layout is made here.  Beside them, the
// block reductions every fixed-order sum of the kernels ends in.
#pragma once
#include "backup_kernels.h"

namespace pbvi {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Sum over the block (blockDim.x = 256) in a fixed order; every thread gets the result.  sh: >= 4 doubles.
__device__ __forceinline__ double block_sum(double v, double* sh) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) sh[wid] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// u + x * w.  ROUND_PRODUCT: the product is rounded, then added (NumPy's doubles: the walk promises bincount's); otherwise
// the compiler may contract the two (it does: v_fmac_f64 -- exact for fp32 operands, whose products fit a double).
template <bool ROUND_PRODUCT>
__device__ __forceinline__ double successor_add(double u, double x, double w) {
    if constexpr (ROUND_PRODUCT) {
#pragma clang fp contract(off)
        const double p = x * w;
        return u + p;
    } else {
        return u + x * w;
    }
}

// Single row: u[sp] for one (a, o) and one landing state sp < S.  rto_all: the table in ModelView's layout [A][O][R][S_pad], of
// the engine's type or an fp64 copy; base(s): the belief value of state s as a double.
template <bool ROUND_PRODUCT, typename TT, typename Base>
__device__ __forceinline__ double successor_pull(const int32_t* in_ptr, const int32_t* in_src, const TT* rto_all, int S,
                                                 int S_pad, int O, int R, int a, int o, int sp, Base base) {
    in_ptr += (int64_t)a * (S + 1);
    in_src += (int64_t)a * S * R;
    const TT* rto = rto_all + (int64_t)(a * O + o) * R * S_pad;
    double u = 0.0;
    for (int j = in_ptr[sp]; j < in_ptr[sp + 1]; ++j) {
        const int e = in_src[j];                             // e = s * R + r
        const int s = e / R, r = e - s * R;
        u = successor_add<ROUND_PRODUCT>(u, base(s), (double)rto[(int64_t)r * S_pad + s]);
    }
    return u;
}

// Tile: u of one landing state for TILE_NB beliefs x TILE_NO observations per thread.  The list of (a, s') and the weights of
// its entries do not depend on the belief, so they are read once for the four; an entry at which all four beliefs are zero
// is skipped (it adds exact zeros).  Blocks of the tile kernels walk TILE_NT chunks of 256 landing states.
constexpr int TILE_NB = 4;   // beliefs per thread
constexpr int TILE_NT = 8;   // 256-state chunks per block
constexpr int TILE_NO = 4;   // observations per pass

// acc[k][q] = u of belief b0 + k (k < nb) under (a, o0 + q) (q < no) over entries [j0, j1) of in_src, here the lists of action a.
template <typename T>
__device__ __forceinline__ void successor_tile(const T* bel, int ldb, int b0, int nb, ModelView<T> mv,
                                               const int32_t* in_src, int j0, int j1, int a, int o0, int no,
                                               double (&acc)[TILE_NB][TILE_NO]) {
#pragma unroll
    for (int k = 0; k < TILE_NB; ++k)
#pragma unroll
        for (int q = 0; q < TILE_NO; ++q) acc[k][q] = 0.0;
    for (int j = j0; j < j1; ++j) {
        const int e = in_src[j];                             // e = s * R + r
        const int s = mv.R == 1 ? e : e / mv.R, r = e - s * mv.R;
        double bs[TILE_NB];
        bool any = false;
#pragma unroll
        for (int k = 0; k < TILE_NB; ++k) {
            bs[k] = k < nb ? (double)bel[(int64_t)(b0 + k) * ldb + s] : 0.0;
            any = any || bs[k] != 0.0;
        }
        if (any) {
#pragma unroll
            for (int q = 0; q < TILE_NO; ++q)
                if (q < no) {
                    const double w = (double)mv.rto[((int64_t)(a * mv.O + o0 + q) * mv.R + r) * mv.S_pad + s];
#pragma unroll
                    for (int k = 0; k < TILE_NB; ++k) acc[k][q] += bs[k] * w;
                }
        }
    }
}

}  // namespace pbvi
