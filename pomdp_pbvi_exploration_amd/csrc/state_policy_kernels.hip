// gfx950 HIP kernel of the state-policy heuristics (pbvi_state_policy, pbvi_rollout_state_policy): most likely state, action
// voting and Thompson sampling over a per-state action table.  include/pbvi_hip.h fixes the arithmetic: every sum is a
// sequential fp64 walk over a chunk of 256 states, and the chunks are combined in order.  The kernel keeps that order and
// still reads the row with coalesced 16-byte loads:
//   * one block of 128 threads per belief row; thread j walks chunk 128 g + j of chunk group g, so 128 walks run side by
//     side (two waves per row: at B = 1000 every SIMD then holds waves of two rows, and one walks while the other stages);
//   * a step stages 128 contiguous bytes of each of the group's 128 chunks (32 fp32 / 16 fp64 states) into an LDS tile, 8
//     lanes per chunk and load; the tile's rows are padded by one element, so the walk's column reads spread over the banks;
//   * the loads of step n + 1 are issued into registers before the walk of step n, which hides them behind it;
//   * at the end of a group the 128 per-chunk results are combined by one thread in chunk order.
// Voting keeps 8 action accumulators in registers per thread and takes one pass over the row per tile of 8 actions (the
// table is staged beside the tile as one byte per state).  Thompson stores (P_c, m_c) per chunk in global scratch, finds the
// chunk with all threads and walks that one chunk again from LDS.  MLS needs no order: 256 threads per row, plain 16-byte
// loads, a (value, state) butterfly per wave and the four waves' results through LDS.
// No atomics; a row's results do not depend on the other rows of the launch.
#include "state_policy_kernels.h"

#include <cstdint>
#include <limits>

namespace pbvi {

namespace {

constexpr int SP_LANES = 128;                 // walkers per row: two waves, so that a SIMD holds two rows' waves at B = 1000
constexpr int SP_MLS_LANES = 256;             // most likely state: four waves per row, for bytes in flight
constexpr int SP_WAVE = 64;
constexpr int SP_AT = 8;                      // actions per register tile of the voting walk
constexpr int SP_NONE = std::numeric_limits<int>::max();

__device__ __forceinline__ uint64_t sp_mix(uint64_t seed, uint64_t idx) {     // synth.splitmix64 (as k_rollout_draw's)
    const uint64_t x = seed + (idx + 1ull) * 0x9E3779B97F4A7C15ull;
    uint64_t z = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double sp_uniform01(uint64_t key, uint64_t counter) {   // synth.uniform01: 53 bits * 2^-53
    return (double)(sp_mix(key, counter) >> 11) * (1.0 / 9007199254740992.0);
}

template <typename T>
struct SpVec;
template <>
struct SpVec<float> {
    using V = float4;
    using I = int4;
};
template <>
struct SpVec<double> {
    using V = double2;
    using I = int2;
};

__device__ __forceinline__ float sp_get(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ __forceinline__ double sp_get(const double2& v, int e) { return e == 0 ? v.x : v.y; }
__device__ __forceinline__ int sp_get(const int4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ __forceinline__ int sp_get(const int2& v, int e) { return e == 0 ? v.x : v.y; }

__device__ __forceinline__ double sp_no_nan(double x) { return x != x ? -std::numeric_limits<double>::infinity() : x; }

}  // namespace

// min / max of (first, last) over the block: a butterfly per wave, then the waves' results through LDS
template <int LANES>
__device__ __forceinline__ void sp_block_min_max(int& lo, int& hi, int lane) {
    __shared__ int wave_lo[LANES / SP_WAVE], wave_hi[LANES / SP_WAVE];
#pragma unroll
    for (int off = 1; off < SP_WAVE; off <<= 1) {
        const int ol = __shfl_xor(lo, off), oh = __shfl_xor(hi, off);
        lo = ol < lo ? ol : lo;
        hi = oh > hi ? oh : hi;
    }
    if ((lane & (SP_WAVE - 1)) == 0) {
        wave_lo[lane / SP_WAVE] = lo;
        wave_hi[lane / SP_WAVE] = hi;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < LANES / SP_WAVE; ++w) {
        lo = wave_lo[w] < lo ? wave_lo[w] : lo;
        hi = wave_hi[w] > hi ? wave_hi[w] : hi;
    }
}

template <typename T, int RULE>
__global__ void __launch_bounds__(RULE == STATE_POLICY_MLS ? SP_MLS_LANES : SP_LANES) k_state_policy(StatePolicy<T> sp) {
#pragma clang fp contract(off)
    using Vec = typename SpVec<T>::V;
    using IVec = typename SpVec<T>::I;
    constexpr int VEC = 16 / (int)sizeof(T);               // elements per 16-byte load
    constexpr int SUB = 128 / (int)sizeof(T);              // states of a chunk staged per step (128 bytes)
    constexpr int QS = STATE_POLICY_CHUNK / SUB;           // steps per chunk group
    constexpr int LPC = SUB / VEC;                         // lanes per chunk and load: 8
    constexpr int NIT = SUB / VEC;                         // loads per lane and step: 8, each covering SP_LANES / LPC = 16 chunks
    constexpr bool VOTING = RULE == STATE_POLICY_VOTING;
    const int i = blockIdx.x, lane = threadIdx.x;
    const int S = sp.S, ldb = sp.ldb;
    const int c = sp.perm ? sp.perm[i] : i;
    const T* __restrict__ row = sp.bel + (int64_t)i * ldb;

    if constexpr (RULE == STATE_POLICY_MLS) {
        // the maximum does not depend on the order: per lane in ascending state order, then a butterfly that prefers the lower state
        double best = -std::numeric_limits<double>::infinity();
        int bidx = SP_NONE;
        const int nvec = ldb / VEC;
#pragma unroll 4
        for (int v = lane; v < nvec; v += SP_MLS_LANES) {
            const Vec x = *reinterpret_cast<const Vec*>(row + (int64_t)v * VEC);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int idx = v * VEC + e;
                const double val = sp_no_nan((double)sp_get(x, e));
                if (idx < S && (val > best || bidx == SP_NONE)) {
                    best = val;
                    bidx = idx;
                }
            }
        }
        __shared__ double wave_best[SP_MLS_LANES / SP_WAVE];
        __shared__ int wave_idx[SP_MLS_LANES / SP_WAVE];
#pragma unroll
        for (int off = 1; off < SP_WAVE; off <<= 1) {
            const double ob = __shfl_xor(best, off);
            const int oi = __shfl_xor(bidx, off);
            if (ob > best || (ob == best && oi < bidx)) {
                best = ob;
                bidx = oi;
            }
        }
        if ((lane & (SP_WAVE - 1)) == 0) {
            wave_best[lane / SP_WAVE] = best;
            wave_idx[lane / SP_WAVE] = bidx;
        }
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int w = 1; w < SP_MLS_LANES / SP_WAVE; ++w) {
                if (wave_best[w] > best || (wave_best[w] == best && wave_idx[w] < bidx)) {
                    best = wave_best[w];
                    bidx = wave_idx[w];
                }
            }
            const int s = bidx == SP_NONE ? 0 : bidx;
            sp.state_out[c] = s;
            sp.action_out[c] = sp.table[s];
        }
        return;
    } else {
        __shared__ T tile[SP_LANES][SUB + 1];
        __shared__ uint8_t acts[VOTING ? SP_LANES : 1][SUB + 4];
        __shared__ double part[SP_LANES][SP_AT + 1];       // voting: W_c[a0 .. a0 + 8) of chunk j; Thompson: (m_c, P_c)
        __shared__ double wtot[VOTING ? STATE_POLICY_MAX_A : 1];
        const int C = (int)state_policy_chunks(S);
        const int ngroups = (C + SP_LANES - 1) / SP_LANES, nsteps = ngroups * QS;
        const int jl = lane / LPC, kl = (lane % LPC) * VEC;   // this lane's chunk within a load, and its first state there
        Vec rb[NIT];
        IVec ra[VOTING ? NIT : 1];

        // first state of load `it` of step `step` for this lane
        auto first_state = [&](int step, int it) {
            const int g = step / QS, q = step - g * QS;
            return ((int64_t)g * SP_LANES + it * (SP_LANES / LPC) + jl) * STATE_POLICY_CHUNK + q * SUB + kl;
        };
        auto load = [&](int step) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int64_t idx = first_state(step, it);
                Vec v{};
                if (idx < ldb) v = *reinterpret_cast<const Vec*>(row + idx);
                rb[it] = v;
                if constexpr (VOTING) {
                    IVec a{};
                    if (idx + VEC <= S) {
                        a = *reinterpret_cast<const IVec*>(sp.table + idx);
                    } else {
                        if (idx < S) a.x = sp.table[idx];
                        if (idx + 1 < S) a.y = sp.table[idx + 1];
                        if constexpr (VEC == 4) {
                            if (idx + 2 < S) a.z = sp.table[idx + 2];
                        }
                    }
                    ra[it] = a;
                }
            }
        };
        auto stage = [&](int step) {
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int64_t idx = first_state(step, it);
                const int j = it * (SP_LANES / LPC) + jl;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    tile[j][kl + e] = idx + e < S ? sp_get(rb[it], e) : (T)0;
                    if constexpr (VOTING) acts[j][kl + e] = (uint8_t)sp_get(ra[it], e);
                }
            }
        };

        if constexpr (VOTING) {
            for (int a0 = 0; a0 < sp.A; a0 += SP_AT) {
                double W = 0.0;                                 // lane r < 8: the votes of action a0 + r
                double acc[SP_AT];
#pragma unroll
                for (int r = 0; r < SP_AT; ++r) acc[r] = 0.0;
                load(0);
                for (int step = 0; step < nsteps; ++step) {
                    stage(step);
                    __syncthreads();
                    if (step + 1 < nsteps) load(step + 1);
#pragma unroll 8
                    for (int k = 0; k < SUB; ++k) {
                        const double v = (double)tile[lane][k];
                        const int a = (int)acts[lane][k] - a0;
#pragma unroll
                        for (int r = 0; r < SP_AT; ++r) acc[r] += a == r ? v : 0.0;   // (+0.0 leaves the bits of a sum >= +0.0)
                    }
                    if (step % QS == QS - 1) {                  // the group's chunks are complete: W += W_c in chunk order
#pragma unroll
                        for (int r = 0; r < SP_AT; ++r) {
                            part[lane][r] = acc[r];
                            acc[r] = 0.0;
                        }
                        __syncthreads();
                        if (lane < SP_AT) {
                            const int g = step / QS;
                            const int nvalid = C - g * SP_LANES < SP_LANES ? C - g * SP_LANES : SP_LANES;
                            for (int j = 0; j < nvalid; ++j) W += part[j][lane];
                        }
                    }
                    __syncthreads();
                }
                if (lane < SP_AT && a0 + lane < sp.A) {
                    wtot[a0 + lane] = W;
                    sp.votes_out[(int64_t)c * sp.A + a0 + lane] = W;
                }
            }
            __syncthreads();
            if (lane == 0) {
                double best = sp_no_nan(wtot[0]);
                int ba = 0;
                for (int a = 1; a < sp.A; ++a) {
                    const double v = sp_no_nan(wtot[a]);
                    if (v > best) {
                        best = v;
                        ba = a;
                    }
                }
                sp.action_out[c] = ba;
                sp.state_out[c] = -1;
            }
        } else {
            __shared__ double total_sh;
            double* __restrict__ sums = sp.chunk_sums + (int64_t)i * C * 2;
            double P = 0.0, m = 0.0;
            load(0);
            for (int step = 0; step < nsteps; ++step) {
                stage(step);
                __syncthreads();
                if (step + 1 < nsteps) load(step + 1);
#pragma unroll 8
                for (int k = 0; k < SUB; ++k) m += (double)tile[lane][k];
                if (step % QS == QS - 1) {
                    const int g = step / QS;
                    const int nvalid = C - g * SP_LANES < SP_LANES ? C - g * SP_LANES : SP_LANES;
                    part[lane][0] = m;
                    m = 0.0;
                    __syncthreads();
                    if (lane == 0) {
                        for (int j = 0; j < nvalid; ++j) {
                            P += part[j][0];
                            part[j][1] = P;
                        }
                    }
                    __syncthreads();
                    if (lane < nvalid) {
                        sums[((int64_t)g * SP_LANES + lane) * 2] = part[lane][1];
                        sums[((int64_t)g * SP_LANES + lane) * 2 + 1] = part[lane][0];
                    }
                }
                __syncthreads();
            }
            if (lane == 0) total_sh = P;
            __syncthreads();                                    // (also: the block's stores to `sums` are visible to its lanes)
            double u;
            if (sp.uniforms) {
                u = sp.uniforms[c];
            } else {
                const uint64_t og = sp.orig ? (uint64_t)sp.orig[c] : (uint64_t)c;
                u = sp_uniform01(sp_mix(sp.seed, sp.first_id + og), (1ull << 33) + (uint64_t)sp.t);
            }
            const double target = u * total_sh;
            int first = SP_NONE, lastpos = -1;
            for (int cc = lane; cc < C; cc += SP_LANES) {
                if (first == SP_NONE && target < sums[(int64_t)cc * 2]) first = cc;
                if (sums[(int64_t)cc * 2 + 1] > 0.0) lastpos = cc;
            }
            sp_block_min_max<SP_LANES>(first, lastpos, lane);
            const int cstar = first != SP_NONE ? first : (lastpos >= 0 ? lastpos : 0);
            const double r = target - (cstar > 0 ? sums[(int64_t)(cstar - 1) * 2] : 0.0);
            T* flat = &tile[0][0];
#pragma unroll
            for (int e = 0; e < STATE_POLICY_CHUNK / SP_LANES; ++e) {
                const int64_t idx = (int64_t)cstar * STATE_POLICY_CHUNK + e * SP_LANES + lane;
                flat[e * SP_LANES + lane] = idx < S ? row[idx] : (T)0;
            }
            __syncthreads();
            if (lane == 0) {
                double q = 0.0;
                int firstj = -1, lastj = -1;
                for (int j = 0; j < STATE_POLICY_CHUNK; ++j) {
                    const double v = (double)flat[j];
                    q += v;
                    if (firstj < 0 && r < q) firstj = j;
                    if (v > 0.0) lastj = j;
                }
                const int jj = firstj >= 0 ? firstj : (lastj >= 0 ? lastj : 0);
                int64_t s = (int64_t)cstar * STATE_POLICY_CHUNK + jj;
                if (s >= S) s = S - 1;                          // (unreachable for a row with mass: the drawn state has b > 0)
                sp.state_out[c] = (int)s;
                sp.action_out[c] = sp.table[s];
            }
        }
    }
}

template <typename T>
hipError_t launch_state_policy(const StatePolicy<T>& sp, hipStream_t st) {
    if (sp.B <= 0) return hipSuccess;
    if (!sp.bel || !sp.table || !sp.action_out || !sp.state_out || sp.S < 1 || sp.A < 1 || sp.A > STATE_POLICY_MAX_A ||
        sp.ldb < sp.S || ((size_t)sp.ldb * sizeof(T)) % 16 != 0 || (reinterpret_cast<uintptr_t>(sp.bel) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(sp.table) & 15) != 0)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)sp.B), block(sp.rule == STATE_POLICY_MLS ? SP_MLS_LANES : SP_LANES);
    switch (sp.rule) {
        case STATE_POLICY_MLS:
            hipLaunchKernelGGL((k_state_policy<T, STATE_POLICY_MLS>), grid, block, 0, st, sp);
            break;
        case STATE_POLICY_VOTING:
            if (!sp.votes_out) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_state_policy<T, STATE_POLICY_VOTING>), grid, block, 0, st, sp);
            break;
        case STATE_POLICY_THOMPSON:
            if (!sp.chunk_sums || sp.t < 0 || sp.t >= (1ll << 31)) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_state_policy<T, STATE_POLICY_THOMPSON>), grid, block, 0, st, sp);
            break;
        default:
            return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template hipError_t launch_state_policy<float>(const StatePolicy<float>&, hipStream_t);
template hipError_t launch_state_policy<double>(const StatePolicy<double>&, hipStream_t);

}  // namespace pbvi
