// Score / projection GEMM for the PBVI backup on gfx950 (CDNA4).
//
//   C[z][m][n] = sum over (a chunk of) the pair's K-tile list of A[m][k] * B[n][k]
//
// In the backup A = belief block [B][S], B = Gamma [(a,o,v)][S] (reference:
// xp.tensordot(belief_array, gamma_a_o_t, (1,3)), src/pomdp.py:1495).  Both operands are
// K-contiguous, exactly the layouts the reference keeps them in, so no transpose copy is ever made
// (NumPy's tensordot makes one internally).
//
// Tile engine: v_mfma_f32_32x32x2_f32 (exact f32 fma chains, 64 FLOP/clk/SIMD = the 157 TFLOP/s fp32
// matrix peak).  256x256x32 tiles, 8 waves (2 per SIMD) laid out 2(M) x 4(N), each wave a 128x64
// sub-tile = 4x2 MFMA blocks = 128 accumulator VGPRs.  Operands go HBM/L2 -> LDS by LDS-DMA
// (global_load_lds_dwordx4) into a double buffer; the 128-byte LDS rows are XOR-swizzled on the SOURCE
// address so the ds_read_b128 fragment reads are bank-conflict free.  K is permuted inside each 8-wide
// group (lane half h takes k = 8g+4h+j for MFMA step j) so one ds_read_b128 feeds four MFMAs; the
// permutation is applied to both operands, so the sum is unchanged.
//
// Zero-tile skipping (exact): for every (m-tile, n-tile) pair only the K tiles where both operands have
// a non-zero are listed and multiplied; a skipped tile could only have added +0 products.
//
// Two schedulers over the same tile engine:
//  * k_gemm_nt_f32_mfma   -- one block per (pair, chunk of the list), optionally batched.  Used with a
//    single chunk per pair for the dense projection (slab 0 is the finished product).
//  * k_gemm_nt_f32_streamk -- persistent, one block per CU, each owning an equal contiguous share of the
//    concatenated tile lists (stream-K): per-pair list lengths differ by 1000x under zero-tile skipping,
//    so equal shares of listed tile-steps is what balances the chip.  A pair split over several blocks
//    leaves one partial slab per block; the consumer sums them in a fixed order (deterministic).
#include "pbvi_common.h"
#include "split_bf16.h"

#include <cstdlib>
#include <type_traits>
#include <map>
#include <mutex>

namespace pbvi {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TILE_FLOATS = 256 * GEMM_BK;          // one operand tile: 256 rows x 32 k = 32 KiB
constexpr int KL_IRR_BIT = 30;                      // tile-list entries: K tile index | (needs gathers << 30), see k_build_klists
constexpr int KL_MASK = (1 << KL_IRR_BIT) - 1;
constexpr int GEMM_LDS_BYTES = 4 * TILE_FLOATS * 4;  // 2 buffers x (A tile + B tile) = 128 KiB

__device__ __forceinline__ void glds16(const float* g, float* l) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

// Per-thread constants of the tile engine.
struct TileThread {
    int lane, wid, i, h, wr, wc;
    int srow[4], scol[4];      // staging: row and (swizzled) first column of this thread's 4 chunks
    int a_row[4], b_row[2];    // fragment rows
    __device__ __forceinline__ void init() {
        const int tid = threadIdx.x;
        lane = tid & 63;
        wid = __builtin_amdgcn_readfirstlane(tid >> 6);   // scalar: the LDS-DMA base (M0) of every stage load becomes an s_add
        i = lane & 31;
        h = lane >> 5;
        wr = wid >> 2;
        wc = wid & 3;
        // 2048 16-byte chunks per operand tile, 4 per thread.  LDS image is lane-linear (chunk c at byte
        // 16c); physical chunk p of row r holds logical chunk p ^ ((r>>1)&7).
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int c = it * 512 + tid;
            const int row = c >> 3, pc = c & 7;
            srow[it] = row;
            scol[it] = (pc ^ ((row >> 1) & 7)) * 4;
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) a_row[mi] = wr * 128 + mi * 32 + i;
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) b_row[ni] = wc * 64 + ni * 32 + i;
    }
};

__device__ __forceinline__ void tile_stage(const TileThread& t, float* lds, int buf, const float* Ablk, int lda,
                                           const float* Bblk, int ldb, int kt) {
    float* la = lds + buf * 2 * TILE_FLOATS;
    float* lb = la + TILE_FLOATS;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int wave_chunk = it * 512 + t.wid * 64;        // wave-uniform LDS base (M0)
        glds16(Ablk + (int64_t)t.srow[it] * lda + kt * GEMM_BK + t.scol[it], la + wave_chunk * 4);
        glds16(Bblk + (int64_t)t.srow[it] * ldb + kt * GEMM_BK + t.scol[it], lb + wave_chunk * 4);
    }
}

// MFMA group g of the four 8-wide K groups of a staged tile pair (one ds_read_b128 feeds four MFMAs)
__device__ __forceinline__ void tile_compute_group(const TileThread& t, const float* lds, int buf, f32x16 (&acc)[4][2], int g) {
    const float* la = lds + buf * 2 * TILE_FLOATS;
    const float* lb = la + TILE_FLOATS;
    f32x4 af[4], bf[2];
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int pc = (2 * g + t.h) ^ ((t.a_row[mi] >> 1) & 7);
        af[mi] = *(const f32x4*)(la + t.a_row[mi] * GEMM_BK + pc * 4);
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int pc = (2 * g + t.h) ^ ((t.b_row[ni] >> 1) & 7);
        bf[ni] = *(const f32x4*)(lb + t.b_row[ni] * GEMM_BK + pc * 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mi][j], bf[ni][j], acc[mi][ni], 0, 0, 0);
}

__device__ __forceinline__ void tile_compute(const TileThread& t, const float* lds, int buf, f32x16 (&acc)[4][2]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) tile_compute_group(t, lds, buf, acc, g);
}

// Multiply list entries [i0, i1) of one pair into acc (double-buffered LDS-DMA pipeline).
__device__ __forceinline__ void tile_run(const TileThread& t, float* lds, const float* Ablk, int lda, const float* Bblk,
                                         int ldb, const int* __restrict__ kl, int i0, int i1, f32x16 (&acc)[4][2]) {
    tile_stage(t, lds, 0, Ablk, lda, Bblk, ldb, kl[i0] & KL_MASK);
    int k_next = (i0 + 1 < i1) ? (kl[i0 + 1] & KL_MASK) : 0;   // list entries are read one step ahead of their use
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int buf = 0;
    for (int it = i0; it < i1; ++it) {
        int k_after = 0;
        if (it + 1 < i1) {
            tile_stage(t, lds, buf ^ 1, Ablk, lda, Bblk, ldb, k_next);
            if (it + 2 < i1) k_after = kl[it + 2] & KL_MASK;
        }
        tile_compute(t, lds, buf, acc);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        buf ^= 1;
        k_next = k_after;
    }
}

__device__ __forceinline__ void tile_zero(f32x16 (&acc)[4][2]) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;
}

// lane holds column (lane&31); register e holds row (e&3) + 8*(e>>2) + 4*(lane>>5)
__device__ __forceinline__ void tile_store(const TileThread& t, float* Cz, int ldc, int tm, int tn,
                                           const f32x16 (&acc)[4][2]) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int col = tn * 256 + t.wc * 64 + ni * 32 + t.i;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = tm * 256 + t.wr * 128 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * t.h;
                Cz[(int64_t)row * ldc + col] = acc[mi][ni][e];
            }
        }
}

// --------------------------------------------------------------------------- //
// scheduler 1: one block per (pair, chunk), batched
// --------------------------------------------------------------------------- //
__global__ __launch_bounds__(512) void k_gemm_nt_f32_mfma(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, float* __restrict__ C,
    int ldc, int64_t slab_stride, int tiles_m, int tiles_n, int k_tiles, int chunk_len, int max_chunks,
    const int* __restrict__ klist, const int* __restrict__ kcount, int64_t batch_stride_b, int64_t batch_stride_c) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // Work-item map.  Blocks b and b+8 share an XCD (round-robin dispatch).  A group = the tiles_m
    // M-tiles of one (n-tile, chunk): they read the same B tile rows, so a group stays on ONE XCD (one L2
    // fill), while groups are dealt round-robin over the 8 XCDs with the chunk index slowest.
    const int bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;
    const int tm = slot % tiles_m;
    const int q = (slot / tiles_m) * 8 + xcd;           // group id
    const int tn = q % tiles_n;
    const int z = q / tiles_n;
    if (z >= max_chunks) return;                        // grid is padded to a multiple of 8 groups
    const int batch = blockIdx.y;
    B += batch * batch_stride_b;
    C += batch * batch_stride_c;
    const int pair = (batch * tiles_n + tn) * tiles_m + tm;
    const int cnt = kcount[pair];
    const int i0 = z * chunk_len;
    const int i1 = (i0 + chunk_len < cnt) ? i0 + chunk_len : cnt;
    if (i0 >= i1) return;                               // this chunk does not exist
    TileThread t;
    t.init();
    f32x16 acc[4][2];
    tile_zero(acc);
    tile_run(t, lds, A + (int64_t)tm * 256 * lda, lda, B + (int64_t)tn * 256 * ldb, ldb,
             klist + (int64_t)pair * k_tiles, i0, i1, acc);
    tile_store(t, C + (int64_t)z * slab_stride, ldc, tm, tn, acc);
}

// --------------------------------------------------------------------------- //
// scheduler 2: stream-K, persistent
// --------------------------------------------------------------------------- //
// Shares are equal in COST, not in tile-steps: every non-empty pair carries `ovh` extra units in front of its list
// (zeroing the accumulators, the exposed latency of its first operand tiles, the 256 KiB slab store), so a block
// whose share crosses many one-tile lists (a rarely-seen observation) is not the last one to finish.  Unit u of a
// pair maps to list entry max(0, u - ovh); a block whose part of a pair lies wholly inside the overhead units
// multiplies nothing and stores nothing.
// plan[0] = q (cost units per block, an upper bound of the tile-steps of any chain), plan[1] = T (total cost units)
__global__ void k_streamk_plan(const int* __restrict__ kcount, int pairs, int nblocks, int k_tiles, int max_split,
                               int ovh, int* __restrict__ prefix, int* __restrict__ start_pair,
                               int* __restrict__ first_block, int* __restrict__ nchunks, int* __restrict__ plan) {
    __shared__ int part[256];
    __shared__ int q_sh;
    const int tid = threadIdx.x;
    const int per = (pairs + 255) / 256;
    const int p0 = (tid * per < pairs) ? tid * per : pairs;
    const int p1 = (p0 + per < pairs) ? p0 + per : pairs;
    int sum = 0;
    for (int p = p0; p < p1; ++p) {
        const int cnt = kcount[p];
        sum += cnt > 0 ? cnt + ovh : 0;
    }
    part[tid] = sum;
    for (int i = tid; i < nblocks; i += 256) start_pair[i] = -1;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int i = 0; i < 256; ++i) {
            const int v = part[i];
            part[i] = run;
            run += v;
        }
        int q = (run + nblocks - 1) / nblocks;
        const int qmin = (k_tiles + ovh + max_split - 1) / max_split;   // a pair spans at most max_split+1 blocks
        if (q < qmin) q = qmin;
        if (q < 1) q = 1;
        q_sh = q;
        plan[0] = q;
        plan[1] = run;
        prefix[pairs] = run;
    }
    __syncthreads();
    const int q = q_sh;
    int run = part[tid];
    for (int p = p0; p < p1; ++p) {
        const int cnt = kcount[p];
        prefix[p] = run;
        if (cnt > 0) {
            const int cost = cnt + ovh;
            const int fb = run / q, lb = (run + cost - 1) / q;
            const int fw = (run + ovh) / q;                                // first block that reaches a list entry
            first_block[p] = fw;
            nchunks[p] = lb - fw + 1;
            for (int i = fb; i <= lb; ++i)
                if ((int64_t)i * q >= run) start_pair[i] = p;          // block i's share begins inside pair p
            run += cost;
        } else {
            first_block[p] = 0;
            nchunks[p] = 0;
        }
    }
}

// Named arguments of the stream-K kernels: the tile lists with the plan k_streamk_plan made of them, and where the slabs go.
struct StreamKView {
    const int *klist, *kcount, *prefix, *start_pair, *first_block, *plan;
    int tiles_m, pairs, k_tiles, ovh;
};
struct SlabOut {
    float* C;
    int ldc;
    int64_t slab_stride;
};

// The share walk of every stream-K kernel.  Block ids are made XCD-contiguous first: consecutive shares (which walk the
// same n-tile's pairs) sit on one XCD.  Share L covers cost units [L q, (L + 1) q) of the concatenated lists (units and
// `ovh`: see k_streamk_plan); part(t, p, tm, tn, lo, hi, acc) multiplies entries [lo, hi) of pair p's list into the zeroed
// accumulators.  The first chunk of a pair is stored into the full slab; a continuation into this block's own tile behind
// it (GemmPlan::c_floats).  Arguments by value: by reference two kernels gain an SGPR spill (profiles/streamk_walk.md).
template <typename Part>
__device__ __forceinline__ void streamk_walk(const StreamKView v, const SlabOut out, Part part) {
    const int nb = gridDim.x;
    int L;
    {
        const int bid = blockIdx.x, xcd = bid & 7, qq = nb >> 3, r = nb & 7;
        const int base = (xcd < r) ? xcd * (qq + 1) : r * (qq + 1) + (xcd - r) * qq;
        L = base + (bid >> 3);
    }
    const int q = v.plan[0], T = v.plan[1];
    int64_t pos = (int64_t)L * q;
    if (pos >= T) return;
    const int64_t end = (pos + q < T) ? pos + q : T;
    int p = v.start_pair[L];
    if (p < 0) return;                                   // cannot happen when pos < T; defensive
    TileThread t;
    t.init();
    while (pos < end && p < v.pairs) {
        const int cnt = v.kcount[p];
        if (cnt == 0) {                                  // block-uniform
            ++p;
            continue;
        }
        const int u_lo = (int)(pos - v.prefix[p]);       // cost units of this pair inside the share
        const int64_t room = end - pos;
        const int u_hi = (u_lo + room < cnt + v.ovh) ? (int)(u_lo + room) : cnt + v.ovh;
        const int lo = u_lo > v.ovh ? u_lo - v.ovh : 0;
        const int hi = u_hi > v.ovh ? u_hi - v.ovh : 0;
        if (hi > lo) {
            const int tm = p % v.tiles_m, tn = p / v.tiles_m;
            f32x16 acc[4][2];
            tile_zero(acc);
            part(t, p, tm, tn, lo, hi, acc);
            const bool cont = L != v.first_block[p];
            tile_store(t, cont ? out.C + out.slab_stride + (int64_t)L * (256 * 256) : out.C, cont ? 256 : out.ldc, cont ? 0 : tm,
                       cont ? 0 : tn, acc);
        }
        pos += u_hi - u_lo;
        ++p;
    }
}

// Every stream-K kernel takes these arguments (one signature: the kernel table below).  Flat, not the two structs: only a
// __restrict__ kernel argument makes the uniform reads of the lists and the plan scalar loads (profiles/streamk_walk.md).
// This kernel reads every B tile and ignores its FusedB.
__global__ __launch_bounds__(512) void k_gemm_nt_f32_streamk(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, FusedB, float* __restrict__ C, int ldc,
    int64_t slab_stride, int tiles_m, int pairs, int k_tiles, const int* __restrict__ klist, const int* __restrict__ kcount,
    const int* __restrict__ prefix, const int* __restrict__ start_pair, const int* __restrict__ first_block,
    const int* __restrict__ plan, int ovh) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const StreamKView v{klist, kcount, prefix, start_pair, first_block, plan, tiles_m, pairs, k_tiles, ovh};
    streamk_walk(v, SlabOut{C, ldc, slab_stride}, [&](const TileThread& t, int p, int tm, int tn, int lo, int hi, auto& acc) {
        tile_run(t, lds, A + (int64_t)tm * 256 * lda, lda, B + (int64_t)tn * 256 * ldb, ldb, klist + (int64_t)p * k_tiles,
                 lo, hi, acc);
    });
}

// --------------------------------------------------------------------------- //
// scheduler 2b: stream-K with the Gamma projection FUSED into the B-operand staging (one reachable state per (s, a))
// --------------------------------------------------------------------------- //
// Gamma[(g, v)][s] = gamma * rto[g][s] * alpha[v][rs[a][s]]   (g = a*O + o; src/pomdp.py:1485-1491 with R = 1)
// is not written to HBM for n-tiles that lie inside one (action, observation) group: the block that multiplies the
// tile generates it on the way into LDS -- per thread and K step one 16-byte load each of the successor indices and
// of RTO (a thread's four 16-byte chunks of the tile sit in rows 64 apart at the same 4 states), four 16-byte alpha
// loads (a grid move maps 4 consecutive states to 4 consecutive successors; otherwise four gathers each), 16
// multiplies, four ds_write_b128 into the same swizzled image the LDS-DMA path produces.  The belief operand still
// arrives by LDS-DMA.  Same products, same rounding (rto*alpha, then *gamma, contraction off) and same summation
// order as projecting first, so the scores are bit-identical to the unfused pipeline -- without its 0.8 GB of Gamma
// writes and the 0.3 ms kernel that makes them.  Tiles flagged in `mat` (those that straddle two groups, and the tail
// tile with the magnitude / reward rows) are projected as before and take the LDS-DMA path from B.
typedef int i32x4 __attribute__((ext_vector_type(4)));

// Loads of the generated operand are issued as inline assembly and waited for with explicit s_waitcnt: vector
// memory operations return in issue order, so "vmcnt(n)" means "all but the last n issued have arrived".  Left to the
// compiler, every use of a loaded value was preceded by vmcnt(0) -- which also waits for the belief tile's LDS-DMA
// loads issued a moment earlier, in the middle of the MFMA stream.
__device__ __forceinline__ void ld16(f32x4& dst, const float* p) {
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void ld16i(i32x4& dst, const int32_t* p) {
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}
__device__ __forceinline__ void ld4(float& dst, const float* p) {
    asm volatile("global_load_dword %0, %1, off" : "=v"(dst) : "v"(p) : "memory");
}

__device__ __forceinline__ f32x4 fused_value(float gamma, f32x4 w, f32x4 av) {
#pragma clang fp contract(off)
    const f32x4 pr = w * av;                 // one rounding, then the scale: exactly k_project's arithmetic
    return gamma * pr;
}

// Multiply list entries [i0, i1) of one pair whose B tile (rows of ONE group) is generated (see above).
// rsrow / rtorow: the group's successor and RTO rows; arow0: alpha row of the tile's first row + this thread's row;
// A list entry with bit KL_IRR_BIT set: that K tile holds a 4-state chunk whose successors are not 4 consecutive states
// (gathers instead of one 16-byte load; block-uniform).
__device__ __forceinline__ void tile_run_fused(const TileThread& t, float* lds, const float* Ablk, int lda,
                                               const int32_t* __restrict__ rsrow, const float* __restrict__ rtorow,
                                               const float* __restrict__ arow0, int64_t a_step /* 64 rows of alpha */,
                                               float gamma, const int* __restrict__ kl,
                                               int i0, int i1, f32x16 (&acc)[4][2]) {
    const int tid = threadIdx.x;
    auto stage_a = [&](int buf, int entry) {
        const int kt = entry & KL_MASK;
        float* la = lds + buf * 2 * TILE_FLOATS;
#pragma unroll
        for (int it = 0; it < 4; ++it)
            glds16(Ablk + (int64_t)t.srow[it] * lda + kt * GEMM_BK + t.scol[it], la + (it * 512 + t.wid * 64) * 4);
    };
    // scol is the same for a thread's four chunks (their rows differ by 64): one table load pair serves all four.
    // Schedule of a K step -- the MFMA groups g0..g3 of the CURRENT tile carry the latencies of the NEXT tile's operands:
    //   tables, belief DMA | g0 | wait tables; alpha loads | g1 | g2 | wait all; scale + 4 ds_write_b128 | g3 | barrier
    i32x4 idx;
    f32x4 w, av[4];
    auto tables = [&](int entry) {
        const int s = (entry & KL_MASK) * GEMM_BK + t.scol[0];
        ld16i(idx, rsrow + s);
        ld16(w, rtorow + s);
    };
    auto alphas = [&](int entry) {
        if (entry >> KL_IRR_BIT) {                        // block-uniform: the list entry carries the flag (k_build_klists)
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const float* arow = arow0 + it * a_step;
                float e0, e1, e2, e3;
                ld4(e0, arow + idx[0]);
                ld4(e1, arow + idx[1]);
                ld4(e2, arow + idx[2]);
                ld4(e3, arow + idx[3]);
                // (assembled before the wait: register moves of values still in flight would be wrong, so the vector is
                // built by the same asm that waits)
                asm volatile("s_waitcnt vmcnt(0)\n\tv_mov_b32 %0, %4\n\tv_mov_b32 %1, %5\n\tv_mov_b32 %2, %6\n\tv_mov_b32 %3, %7"
                             : "=&v"(av[it].x), "=&v"(av[it].y), "=&v"(av[it].z), "=&v"(av[it].w)
                             : "v"(e0), "v"(e1), "v"(e2), "v"(e3)
                             : "memory");
            }
        } else {
#pragma unroll
            for (int it = 0; it < 4; ++it) ld16(av[it], arow0 + it * a_step + idx[0]);
        }
    };
    auto store_b = [&](int buf) {
        float* lb = lds + buf * 2 * TILE_FLOATS + TILE_FLOATS;
#pragma unroll
        for (int it = 0; it < 4; ++it) *(f32x4*)(lb + (it * 512 + tid) * 4) = fused_value(gamma, w, av[it]);
    };
    // first tile of the segment: nothing to overlap with
    tables(kl[i0]);
    stage_a(0, kl[i0]);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(idx), "+v"(w)::"memory");
    alphas(kl[i0]);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(av[0]), "+v"(av[1]), "+v"(av[2]), "+v"(av[3])::"memory");
    store_b(0);
    int k_next = (i0 + 1 < i1) ? kl[i0 + 1] : 0;         // list entries are read one step ahead of their use
    __syncthreads();
    int buf = 0;
    for (int it = i0; it < i1; ++it) {
        int k_after = 0;
        const bool more = it + 1 < i1;                    // block-uniform
        if (more) {
            tables(k_next);                               // the 2 small loads first, then the 4 DMA loads of the belief tile
            stage_a(buf ^ 1, k_next);
            if (it + 2 < i1) k_after = kl[it + 2];
        }
        tile_compute_group(t, lds, buf, acc, 0);
        if (more) {
            asm volatile("s_waitcnt vmcnt(4)" : "+v"(idx), "+v"(w)::"memory");      // the tables are here; the DMA may not be
            alphas(k_next);
        }
        tile_compute_group(t, lds, buf, acc, 1);
        tile_compute_group(t, lds, buf, acc, 2);
        if (more) {
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(av[0]), "+v"(av[1]), "+v"(av[2]), "+v"(av[3])::"memory");
            store_b(buf ^ 1);
        }
        tile_compute_group(t, lds, buf, acc, 3);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        buf ^= 1;
        k_next = k_after;
    }
}

__global__ __launch_bounds__(512) void k_gemm_nt_f32_streamk_fused(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, FusedB fb, float* __restrict__ C, int ldc,
    int64_t slab_stride, int tiles_m, int pairs, int k_tiles, const int* __restrict__ klist, const int* __restrict__ kcount,
    const int* __restrict__ prefix, const int* __restrict__ start_pair, const int* __restrict__ first_block,
    const int* __restrict__ plan, int ovh) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const StreamKView v{klist, kcount, prefix, start_pair, first_block, plan, tiles_m, pairs, k_tiles, ovh};
    streamk_walk(v, SlabOut{C, ldc, slab_stride}, [&](const TileThread& t, int p, int tm, int tn, int lo, int hi, auto& acc) {
        if (fb.mat[tn]) {                                // block-uniform: projected rows, the LDS-DMA path
            const int bt = fb.ctile != nullptr ? fb.ctile[tn] : tn;          // (compact layout: only these tiles exist)
            tile_run(t, lds, A + (int64_t)tm * 256 * lda, lda, B + (int64_t)bt * 256 * ldb, ldb,
                     klist + (int64_t)p * k_tiles, lo, hi, acc);
        } else {
            const int r0 = tn * 256;
            const int g = r0 / fb.V, v0 = r0 - g * fb.V;                     // scalar: all 256 rows belong to group g
            tile_run_fused(t, lds, A + (int64_t)tm * 256 * lda, lda, fb.rs + (int64_t)(g / fb.O) * fb.S_pad,
                           fb.rto + (int64_t)g * fb.S_pad, fb.alpha + (int64_t)(v0 + t.srow[0]) * fb.lda,
                           (int64_t)64 * fb.lda, fb.gamma, klist + (int64_t)p * k_tiles, lo, hi, acc);
        }
    });
}

// --------------------------------------------------------------------------- //
// scheduler 2c: stream-K with the Gamma projection fused for 2..7 reachable states per (s, a)
// --------------------------------------------------------------------------- //
// Gamma[(g, v)][s] = gamma * sum_r rto[g][r][s] * alpha[v][rs[a][r][s]]   (src/pomdp.py:1485-1491, the padded-ELL SpMM)
// With R successors a generated B tile needs R gathered alpha chunks per 16-byte output chunk: 20 16-byte loads per
// thread and K step at R = 5 against the 128 MFMAs (8192 SIMD cycles) a wave issues in that step.  What does not fit
// is registers (the tile engine leaves ~24 for the staging), so a K step is cut into 2R UNITS -- (half h of the
// thread's four rows) x (successor slot r) -- of two alpha loads each, issued at the 16 boundaries between the
// 8-MFMA sub-groups of the step and consumed two boundaries later: two units (4 loads, 16 VGPRs) in flight, one
// 2-row accumulator (8 VGPRs), the same footprint as the R = 1 kernel's staging.  The successor indices and RTO
// weights of the K tile are not held in registers at all: wave 0 copies them (R x 128 B each) into LDS by LDS-DMA
// one K step ahead, and every thread reads its 16 bytes of them right where it uses them.
// Arithmetic is k_project's, operation for operation (acc = 0; acc = acc + rto*alpha per r, contraction off; then
// gamma * acc), so the scores are bit-identical to the unfused pipeline.
// K tiles in which some 4-state chunk has non-consecutive successors for some r (grid edges; flagged per action in
// bit KL_IRR_BIT of the list entry) are NOT generated: k_project writes those Gamma tiles (8-16 % of them on the
// olfactory grids) and the step stages B by LDS-DMA like the unfused kernel.  Both kinds of step share one loop.
constexpr int FUSED_R_MAX = 7;                       // 2R + 2 <= 16 issue points per K step
constexpr int TAB_WORDS = 8 * GEMM_BK;               // one table image: [r < 8][32 states]
constexpr int GEMM_LDS_BYTES_R = GEMM_LDS_BYTES + 2 * 2 * TAB_WORDS * 4;   // + 2 buffers x (indices, weights) = 4 KiB

struct Frag {
    f32x4 af[4], bf[2];
};
__device__ __forceinline__ void frag_load(const TileThread& t, const float* lds, int buf, int g, Frag& f) {
    const float* la = lds + buf * 2 * TILE_FLOATS;
    const float* lb = la + TILE_FLOATS;
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int pc = (2 * g + t.h) ^ ((t.a_row[mi] >> 1) & 7);
        f.af[mi] = *(const f32x4*)(la + t.a_row[mi] * GEMM_BK + pc * 4);
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int pc = (2 * g + t.h) ^ ((t.b_row[ni] >> 1) & 7);
        f.bf[ni] = *(const f32x4*)(lb + t.b_row[ni] * GEMM_BK + pc * 4);
    }
}
__device__ __forceinline__ void frag_mfma(const Frag& f, int j, f32x16 (&acc)[4][2]) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.af[mi][j], f.bf[ni][j], acc[mi][ni], 0, 0, 0);
}

__device__ __forceinline__ f32x4 proj_add(f32x4 acc, f32x4 w, f32x4 av) {
#pragma clang fp contract(off)
    const f32x4 pr = w * av;                 // k_project: acc = acc + w * av, one rounding per operation
    return acc + pr;
}
__device__ __forceinline__ f32x4 proj_scale(float gamma, f32x4 acc) {
#pragma clang fp contract(off)
    return gamma * acc;
}

// Multiply list entries [i0, i1) of one pair whose B rows belong to ONE group (see above).  rs_a / rto_g: the R
// successor / weight rows of the group's action / of the group, S_pad apart; arow0: alpha row of the tile's first
// row + this thread's row; Bblk: the projected Gamma rows (read for the flagged K tiles only).
template <int R>
__device__ __forceinline__ void tile_run_fused_r(const TileThread& t, float* lds, const float* Ablk, int lda,
                                                 const float* Bblk, int ldb, const int32_t* __restrict__ rs_a,
                                                 const float* __restrict__ rto_g, int S_pad,
                                                 const float* __restrict__ arow0, int64_t a_step /* 64 rows of alpha */,
                                                 float gamma, const int* __restrict__ kl, int i0, int i1,
                                                 f32x16 (&acc)[4][2]) {
    const int tid = threadIdx.x;
    int32_t* tabi = (int32_t*)(lds + 4 * TILE_FLOATS);      // [2][8][32] successor indices of the K tile
    float* tabw = (float*)(tabi + 2 * TAB_WORDS);           // [2][8][32] RTO weights
    constexpr int nunits = 2 * R;
    static_assert(R >= 2 && R <= FUSED_R_MAX, "2R + 2 issue points must fit the 16 of a K step");
    const int scol0 = t.scol[0];                            // the thread's 4 states inside the K tile (same for its 4 rows)
    auto stage_a = [&](int buf, int entry) {
        const int kt = entry & KL_MASK;
        float* la = lds + buf * 2 * TILE_FLOATS;
#pragma unroll
        for (int it = 0; it < 4; ++it)
            glds16(Ablk + (int64_t)t.srow[it] * lda + kt * GEMM_BK + t.scol[it], la + (it * 512 + t.wid * 64) * 4);
    };
    auto stage_b = [&](int buf, int entry) {
        const int kt = entry & KL_MASK;
        float* lb = lds + buf * 2 * TILE_FLOATS + TILE_FLOATS;
#pragma unroll
        for (int it = 0; it < 4; ++it)
            glds16(Bblk + (int64_t)t.srow[it] * ldb + kt * GEMM_BK + t.scol[it], lb + (it * 512 + t.wid * 64) * 4);
    };
    auto stage_tab = [&](int tb, int entry) {               // wave 0: lane (r, c) copies chunk c of row r
        if (t.wid == 0 && t.lane < 8 * R) {
            const int64_t off = (int64_t)(t.lane >> 3) * S_pad + (entry & KL_MASK) * GEMM_BK + (t.lane & 7) * 4;
            glds16((const float*)(rs_a + off), (float*)(tabi + tb * TAB_WORDS));
            glds16(rto_g + off, tabw + tb * TAB_WORDS);
        }
    };
    f32x4 av[2][2];                                          // two units in flight
    f32x4 pacc[2];
    auto unit_issue = [&](int u, int slot, int tb) {
        const int hh = u >= R ? 1 : 0, r = u - hh * R;     // compile-time at the unrolled issue points
        const i32x4 idx = *(const i32x4*)(tabi + tb * TAB_WORDS + r * GEMM_BK + scol0);
        const float* p0 = arow0 + (int64_t)(2 * hh) * a_step + idx[0];
        ld16(av[slot][0], p0);
        ld16(av[slot][1], p0 + a_step);
    };
    auto unit_consume = [&](int u, int slot, int tb, int dst_buf, bool last_in_queue) {
        const int hh = u >= R ? 1 : 0, r = u - hh * R;
        const f32x4 w = *(const f32x4*)(tabw + tb * TAB_WORDS + r * GEMM_BK + scol0);
        if (last_in_queue)
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(av[slot][0]), "+v"(av[slot][1])::"memory");
        else                                                  // the next unit's two loads may still be in flight
            asm volatile("s_waitcnt vmcnt(2)" : "+v"(av[slot][0]), "+v"(av[slot][1])::"memory");
        if (r == 0) {
            pacc[0] = f32x4{0.f, 0.f, 0.f, 0.f};
            pacc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        pacc[0] = proj_add(pacc[0], w, av[slot][0]);
        pacc[1] = proj_add(pacc[1], w, av[slot][1]);
        if (r == R - 1) {
            float* lb = lds + dst_buf * 2 * TILE_FLOATS + TILE_FLOATS;
            *(f32x4*)(lb + ((2 * hh) * 512 + tid) * 4) = proj_scale(gamma, pacc[0]);
            *(f32x4*)(lb + ((2 * hh + 1) * 512 + tid) * 4) = proj_scale(gamma, pacc[1]);
        }
    };
    // first tile of the segment: nothing to overlap with
    {
        const int e0 = kl[i0];
        stage_a(0, e0);
        if (e0 >> KL_IRR_BIT) {
            stage_b(0, e0);
        } else {
            stage_tab(0, e0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            for (int u = 0; u < nunits; ++u) {
                unit_issue(u, 0, 0);
                unit_consume(u, 0, 0, 0, true);
            }
        }
    }
    int e_next = (i0 + 1 < i1) ? kl[i0 + 1] : 0;            // list entries are read ahead of their use
    if (i0 + 1 < i1 && !(e_next >> KL_IRR_BIT)) stage_tab(1, e_next);
    int e_after = (i0 + 2 < i1) ? kl[i0 + 2] : 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int buf = 0;
    for (int it = i0; it < i1; ++it) {
        const bool more = it + 1 < i1;                       // block-uniform, as everything that branches below
        const bool gen = more && !(e_next >> KL_IRR_BIT);
        int e_after2 = 0;
        if (more) {
            stage_a(buf ^ 1, e_next);
            if (!gen) stage_b(buf ^ 1, e_next);
            if (it + 2 < i1 && !(e_after >> KL_IRR_BIT)) stage_tab(buf, e_after);   // tile it+2's tables; tile it's are done with
            if (it + 3 < i1) e_after2 = kl[it + 3];
        }
        Frag f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            frag_load(t, lds, buf, g, f);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = 4 * g + j;                     // issue point p: unit p goes out, unit p-2 comes in
                if (gen) {
                    if (p >= 2 && p - 2 < nunits) unit_consume(p - 2, p & 1, buf ^ 1, buf ^ 1, p - 2 == nunits - 1);
                    if (p < nunits) unit_issue(p, p & 1, buf ^ 1);
                }
                frag_mfma(f, j, acc);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        buf ^= 1;
        e_next = e_after;
        e_after = e_after2;
    }
}

template <int R>
__global__ __launch_bounds__(512) void k_gemm_nt_f32_streamk_fused_r(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, FusedB fb, float* __restrict__ C, int ldc,
    int64_t slab_stride, int tiles_m, int pairs, int k_tiles, const int* __restrict__ klist, const int* __restrict__ kcount,
    const int* __restrict__ prefix, const int* __restrict__ start_pair, const int* __restrict__ first_block,
    const int* __restrict__ plan, int ovh) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const StreamKView v{klist, kcount, prefix, start_pair, first_block, plan, tiles_m, pairs, k_tiles, ovh};
    streamk_walk(v, SlabOut{C, ldc, slab_stride}, [&](const TileThread& t, int p, int tm, int tn, int lo, int hi, auto& acc) {
        if (fb.mat[tn]) {                                // block-uniform: projected rows, the LDS-DMA path
            tile_run(t, lds, A + (int64_t)tm * 256 * lda, lda, B + (int64_t)tn * 256 * ldb, ldb,
                     klist + (int64_t)p * k_tiles, lo, hi, acc);
        } else {
            const int r0 = tn * 256;
            const int g = r0 / fb.V, v0 = r0 - g * fb.V;                     // scalar: all 256 rows belong to group g
            tile_run_fused_r<R>(t, lds, A + (int64_t)tm * 256 * lda, lda, B + (int64_t)tn * 256 * ldb, ldb,
                                fb.rs + (int64_t)(g / fb.O) * R * fb.S_pad, fb.rto + (int64_t)g * R * fb.S_pad, fb.S_pad,
                                fb.alpha + (int64_t)(v0 + t.srow[0]) * fb.lda, (int64_t)64 * fb.lda, fb.gamma,
                                klist + (int64_t)p * k_tiles, lo, hi, acc);
        }
    });
}

// --------------------------------------------------------------------------- //
// scheduler 2d: stream-K on bf16 MFMAs with a three-term operand split (fp32 data, fp32 accumulation)
// --------------------------------------------------------------------------- //
// Every operand element x is split as hi = RNE_bf16(x), lo = RNE_bf16(x - hi) (x - hi is exact in fp32), and a product
// b*g is taken as bh*gh + bh*gl + bl*gh: three v_mfma_f32_32x32x16_bf16 per 32x32x16 block, 3/16 of the MFMA cycles of
// the fp32 instruction.  Per product |b*g - (bh*gh + bh*gl + bl*gh)| <= (3u^2 + 2u^3)|b||g|, u = 2^-8; the engine widens
// the tie window by that (numerics).  A finite |x| above the largest finite bf16 (where RNE would give inf)
// takes hi = +-max bf16 instead, which keeps the same bound within 1 %.
// A 256-row x 32-k stage of (hi, lo) is 32 KiB, the size of an fp32 stage, so the double buffer and the source-side XOR
// swizzle carry over -- LDS row r holds 8 chunks
// of 8 bf16: hi k 0-7, 8-15, 16-23, 24-31, then lo in the same order, chunk c at physical chunk c ^ ((r>>1)&7).  Lane
// (i, h) of the k-half kk reads hi chunk 2kk+h and lo chunk 4+2kk+h of its rows: k = 16kk + 8h + j, the MFMA's own order.
// The belief operand arrives pre-split: the engine keeps a split plane of the block (split_bf16.h), written once per block
// with the same split code, and it is staged by LDS-DMA.  The B operand is generated (scheduler 2b's arithmetic, then
// split) or read from fp32 rows in HBM and split in registers; the two routes write the same LDS image, so they issue the
// same MFMAs on the same bits.  Plan, lists, slabs: unchanged.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// 8 consecutive k of one row (x0: k 0-3, x1: k 4-7) -> hi and lo chunks of that row's LDS image
__device__ __forceinline__ void split_store(float* lop, int row, int kg, const f32x4& x0, const f32x4& x1) {
    i32x4 hi, lo;
    uint32_t h, l;
    split_pair(x0[0], x0[1], h, l); hi[0] = (int)h; lo[0] = (int)l;
    split_pair(x0[2], x0[3], h, l); hi[1] = (int)h; lo[1] = (int)l;
    split_pair(x1[0], x1[1], h, l); hi[2] = (int)h; lo[2] = (int)l;
    split_pair(x1[2], x1[3], h, l); hi[3] = (int)h; lo[3] = (int)l;
    const int sw = (row >> 1) & 7;
    *(i32x4*)(lop + row * GEMM_BK + (kg ^ sw) * 4) = hi;
    *(i32x4*)(lop + row * GEMM_BK + ((4 + kg) ^ sw) * 4) = lo;
}

// K-step schedules of tile_run_split (pbvi_debug_split_schedule).  The parent one reads each group's fragments right
// before its MFMAs and is the default; the pipelined one reads them a group ahead behind counted waits.  Bit-identical
// slabs.  Measurements of both: profiles/split_lds_pipeline.md.
constexpr int SPLIT_SCHED_PARENT = 0, SPLIT_SCHED_PIPELINED = 1;

// Fragments of one k-half of the staged tile pair: the hi and lo chunks of the wave's 4 A rows and 2 B rows
struct SplitFrag {
    i32x4 ah[4], al[4], bh[2], bl[2];
};
// Term `term` of k-half kk over the wave's 8 blocks, after reading the fragments it is the first to need (term 0: ah, bh;
// 1: bl; 2: al -- at most 32 fragment VGPRs live instead of 48).  Per element the order is fixed: + bh*gh, + bh*gl,
// + bl*gh, then the next k-half (term-major over the 8 blocks: no dependent pairs back to back).
__device__ __forceinline__ void split_group(const TileThread& t, const float* lds, int buf, int kk, int term, SplitFrag& f,
                                            f32x16 (&acc)[4][2]) {
    const float* la = lds + buf * 2 * TILE_FLOATS;
    const float* lb = la + TILE_FLOATS;
    const int hc = 2 * kk + t.h;                          // logical chunk of the hi part; lo: 4 + hc
    if (term != 1) {
#pragma unroll
        for (int mi = 0; mi < 4; ++mi) {
            const int r = t.a_row[mi], sw = (r >> 1) & 7;
            if (term == 0) f.ah[mi] = *(const i32x4*)(la + r * GEMM_BK + (hc ^ sw) * 4);
            else f.al[mi] = *(const i32x4*)(la + r * GEMM_BK + ((4 + hc) ^ sw) * 4);
        }
    }
    if (term != 2) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int r = t.b_row[ni], sw = (r >> 1) & 7;
            if (term == 0) f.bh[ni] = *(const i32x4*)(lb + r * GEMM_BK + (hc ^ sw) * 4);
            else f.bl[ni] = *(const i32x4*)(lb + r * GEMM_BK + ((4 + hc) ^ sw) * 4);
        }
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const i32x4 a = term == 2 ? f.al[mi] : f.ah[mi];
            const i32x4 b = term == 1 ? f.bl[ni] : f.bh[ni];
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                                  acc[mi][ni], 0, 0, 0);
        }
}

// The pipelined schedule's fragment slots: two A slots (4 rows) and two B slots (2 rows); which part sits in which slot
// is fixed at compile time (see tile_run_split).
struct SplitSlots {
    i32x4 a[2][4], b[2][2];
};
// The fragment reads of the pipelined schedule are inline assembly, so that the waits in front of the MFMA groups can
// count them: the compiler drains lgkmcnt to 0 at every use of an LDS read while an LDS-DMA load is in flight, which in
// this loop is always.  LDS operations retire in order; split_wait_*(N, ..) lets the N youngest stay in flight and takes the
// registers it releases as operands, so nothing reads or copies them earlier.  (A scalar load that shares the counter
// and returns out of order can only make such a wait stricter.)
__device__ __forceinline__ void lds_read16(i32x4& dst, uint32_t addr, int offset) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(offset) : "memory");
}
__device__ __forceinline__ uint32_t lds_addr(const float* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)p;
}
// The hi (lo = false) or lo chunks of k-half kk of the wave's A rows / B rows: the same LDS words split_group reads.
// All six rows of a lane share i = lane & 31 and with it the swizzle, so an address is a wave-uniform part (buffer,
// operand, the wave's first row) plus one of four lane parts that serve both operands, plus an immediate per row.
__device__ __forceinline__ uint32_t split_lane_part(const TileThread& t, int kk, bool lo) {
    const int c = (lo ? 4 : 0) + 2 * kk + t.h, sw = (t.i >> 1) & 7;
    return (uint32_t)(t.i * GEMM_BK + (c ^ sw) * 4) * 4u;
}
__device__ __forceinline__ void split_read_a(const TileThread& t, const float* lds, int buf, int kk, bool lo, i32x4 (&a)[4]) {
    const uint32_t addr = lds_addr(lds + buf * 2 * TILE_FLOATS + t.wr * 128 * GEMM_BK) + split_lane_part(t, kk, lo);
    lds_read16(a[0], addr, 0);
    lds_read16(a[1], addr, 32 * GEMM_BK * 4);
    lds_read16(a[2], addr, 64 * GEMM_BK * 4);
    lds_read16(a[3], addr, 96 * GEMM_BK * 4);
}
__device__ __forceinline__ void split_read_b(const TileThread& t, const float* lds, int buf, int kk, bool lo, i32x4 (&b)[2]) {
    const uint32_t addr = lds_addr(lds + buf * 2 * TILE_FLOATS + TILE_FLOATS + t.wc * 64 * GEMM_BK) + split_lane_part(t, kk, lo);
    lds_read16(b[0], addr, 0);
    lds_read16(b[1], addr, 32 * GEMM_BK * 4);
}
// Wait until at most N LDS operations are in flight, for an A slot, a B slot or both
#define PBVI_SPLIT_WAIT(N) "s_waitcnt lgkmcnt(" #N ")"
#define PBVI_SPLIT_A(a) "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3])
#define PBVI_SPLIT_B(b) "+v"(b[0]), "+v"(b[1])
// (the MFMAs touch no memory, so only a scheduling barrier keeps them behind the wait)
#define split_wait_ab(N, a, b)                                                            \
    do {                                                                                  \
        asm volatile(PBVI_SPLIT_WAIT(N) : PBVI_SPLIT_A(a), PBVI_SPLIT_B(b)::"memory");    \
        __builtin_amdgcn_sched_barrier(0);                                                \
    } while (0)
#define split_wait_a(N, a)                                              \
    do {                                                                \
        asm volatile(PBVI_SPLIT_WAIT(N) : PBVI_SPLIT_A(a)::"memory");   \
        __builtin_amdgcn_sched_barrier(0);                              \
    } while (0)
#define split_wait_b(N, b)                                              \
    do {                                                                \
        asm volatile(PBVI_SPLIT_WAIT(N) : PBVI_SPLIT_B(b)::"memory");   \
        __builtin_amdgcn_sched_barrier(0);                              \
    } while (0)
// One term over the wave's 8 blocks, in split_group's block order
__device__ __forceinline__ void split_mfma8(const i32x4 (&a)[4], const i32x4 (&b)[2], f32x16 (&acc)[4][2]) {
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[mi]), __builtin_bit_cast(bf16x8, b[ni]),
                                                                  acc[mi][ni], 0, 0, 0);
}

// Multiply list entries [i0, i1) of one pair.  Aplane: the belief rows' split plane (split_bf16.h), staged by LDS-DMA
// exactly like an fp32 operand (tile_stage's source swizzle), so the A image needs no register pass.  gen: the B tile is
// generated (rsrow / rtorow: the group's successor and RTO rows; arow0: alpha row of this thread's first staging row;
// a_step: 128 rows of alpha); else it is read from the fp32 rows at Bblk.  B staging: thread tid takes k-group
// kg = tid & 3 (8 states) of rows it * 128 + (tid >> 2), it = 0, 1, loads them to registers, splits them and writes both
// halves of that row's LDS image.  Loads are inline assembly counted by explicit s_waitcnt (see ld16).  A K step is six
// MFMA groups of 8 (k-half x term) that carry the latencies of the NEXT tile's operands, as in tile_run_fused; the
// successor indices are loaded one step earlier still, so no dependent load chain sits inside a step (a step is only
// ~3000 SIMD cycles, about two memory round trips):
//   gen:  alphas + weights (tile k+1), indices (k+2), A DMA (k+1) | kk0 t0 | kk0 t1 | kk0 t2 | kk1 t0 | wait alphas;
//         B rows 0-127 | kk1 t1 | B rows 128-255 | kk1 t2 | barrier
//   else: B rows, A DMA | kk0 t0 | kk0 t1 | kk0 t2 | kk1 t0 | wait B rows; B rows 0-127 | kk1 t1 | B rows 128-255 | kk1 t2 |
//         barrier
// STAG (parent schedule only): waves 0-3 run the step above, waves 4-7 the same terms with the staging first:
//   B rows 0-255 of tile k+1 (registers landed a step earlier), A DMA (k+1), register loads of tile k+2 (indices: k+3) |
//   kk0 t0 | kk0 t1 | kk0 t2 | kk1 t0 | kk1 t1 | kk1 t2 | wait all | barrier
template <int SCHED, bool STAG>
__device__ __forceinline__ void tile_run_split(const TileThread& t, float* lds, const float* Aplane, int lda, const float* Bblk,
                                               int ldb, bool gen, const int32_t* __restrict__ rsrow,
                                               const float* __restrict__ rtorow, const float* __restrict__ arow0,
                                               int64_t a_step, float gamma, const int* __restrict__ kl, int i0, int i1,
                                               f32x16 (&acc)[4][2]) {
    int tid = threadIdx.x;
    // (staggered kernel: the per-thread staging addresses are worked out per segment, not kept for the whole kernel --
    // its loops leave no VGPR for them, and they would go to scratch)
    if constexpr (STAG) asm volatile("" : "+v"(tid));
    const int kg = tid & 3, r0 = tid >> 2;
    f32x4 xb[2][2];
    i32x4 idx[2];
    f32x4 w[2];
    // A staging: one 32-bit lane offset from a block-uniform base (the engine keeps 256 rows of the plane under 4 GiB), so
    // the loop keeps one VGPR of addresses instead of four 64-bit pointers
    const uint32_t a_off = (uint32_t)(t.srow[0] * lda + t.scol[0]) * 4u;     // srow[it] = srow[0] + 64 it, same scol
    auto stage_a = [&](int buf, int entry) {
        const char* base = (const char*)(Aplane + (int64_t)(entry & KL_MASK) * GEMM_BK);
        float* la = lds + buf * 2 * TILE_FLOATS;
#pragma unroll
        for (int it = 0; it < 4; ++it)
            glds16((const float*)(base + (int64_t)it * 64 * lda * 4 + a_off), la + (it * 512 + t.wid * 64) * 4);
    };
    auto load_rows = [&](int entry) {
        const int k = (entry & KL_MASK) * GEMM_BK + kg * 8;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const float* p = Bblk + (int64_t)(it * 128 + r0) * ldb + k;
            ld16(xb[it][0], p);
            ld16(xb[it][1], p + 4);
        }
    };
    auto indices = [&](int entry) {                     // successor indices: two K steps ahead of the tile's store
        const int s = (entry & KL_MASK) * GEMM_BK + kg * 8;
        ld16i(idx[0], rsrow + s);
        ld16i(idx[1], rsrow + s + 4);
    };
    auto weights = [&](int entry) {                     // RTO weights: with the alpha loads, one step ahead
        const int s = (entry & KL_MASK) * GEMM_BK + kg * 8;
        ld16(w[0], rtorow + s);
        ld16(w[1], rtorow + s + 4);
    };
    auto alphas = [&](int entry) {
        if (entry >> KL_IRR_BIT) {                        // block-uniform: some 4-state chunk of the K tile needs gathers
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const float* arow = arow0 + it * a_step;
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    float e0, e1, e2, e3;
                    ld4(e0, arow + idx[q][0]);
                    ld4(e1, arow + idx[q][1]);
                    ld4(e2, arow + idx[q][2]);
                    ld4(e3, arow + idx[q][3]);
                    asm volatile("s_waitcnt vmcnt(0)\n\tv_mov_b32 %0, %4\n\tv_mov_b32 %1, %5\n\tv_mov_b32 %2, %6\n\tv_mov_b32 %3, %7"
                                 : "=&v"(xb[it][q].x), "=&v"(xb[it][q].y), "=&v"(xb[it][q].z), "=&v"(xb[it][q].w)
                                 : "v"(e0), "v"(e1), "v"(e2), "v"(e3)
                                 : "memory");
                }
            }
        } else {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                ld16(xb[it][0], arow0 + it * a_step + idx[0][0]);
                ld16(xb[it][1], arow0 + it * a_step + idx[1][0]);
            }
        }
    };
    auto store_b = [&](int buf, int it) {                 // rows it * 128 + r0
        float* lb = lds + buf * 2 * TILE_FLOATS + TILE_FLOATS;
        if (gen)
            split_store(lb, it * 128 + r0, kg, fused_value(gamma, w[0], xb[it][0]), fused_value(gamma, w[1], xb[it][1]));
        else
            split_store(lb, it * 128 + r0, kg, xb[it][0], xb[it][1]);
    };
    // The next tile's B operand has arrived: split and store its rows 0-127.  The waits take the loaded registers as
    // operands, so nothing copies them before they arrive; a wait must not depend on a run-time condition (two asm
    // statements would get operand copies placed ahead of the wait).
    auto wait_and_store_b0 = [&](int buf) {
        if (gen)                                          // alphas + weights in; the indices and the DMA may not be
            asm volatile("s_waitcnt vmcnt(6)" : "+v"(xb[0][0]), "+v"(xb[0][1]), "+v"(xb[1][0]), "+v"(xb[1][1]), "+v"(w[0]),
                         "+v"(w[1])::"memory");
        else                                              // the B rows in; the DMA may not be
            asm volatile("s_waitcnt vmcnt(4)" : "+v"(xb[0][0]), "+v"(xb[0][1]), "+v"(xb[1][0]), "+v"(xb[1][1])::"memory");
        store_b(buf, 0);
    };
    // first tile of the segment: nothing to overlap with
    {
        const int e0 = kl[i0];
        if (gen) {
            indices(e0);
            weights(e0);
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(idx[0]), "+v"(idx[1])::"memory");
            alphas(e0);
            indices(i0 + 1 < i1 ? kl[i0 + 1] : 0);        // (unconditional: see the waits in the loop)
        } else {
            load_rows(e0);
        }
        stage_a(0, e0);
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(xb[0][0]), "+v"(xb[0][1]), "+v"(xb[1][0]), "+v"(xb[1][1]), "+v"(w[0]), "+v"(w[1]),
                     "+v"(idx[0]), "+v"(idx[1])::"memory");
        store_b(0, 0);
        store_b(0, 1);
    }
    // list entries are read ahead of their use
    int k_next = (i0 + 1 < i1) ? kl[i0 + 1] : 0;
    int k_after = (i0 + 2 < i1) ? kl[i0 + 2] : 0;
    int buf = 0;
    if (STAG && t.wid >= 4) {                             // (by half, not by parity: profiles/split_stagger.md)
        // The late half of a staggered block.  Between two barriers every LDS read goes to buf and every write to buf ^ 1,
        // so a wave may order its own interval freely: this half stages first and multiplies last, and its SIMD partner
        // (wave wid - 4) does the reverse.  In interval `it` it scales, splits and stores tile it+1 from registers that
        // landed during interval it-1, issues tile it+1's A DMA and the register loads of tile it+2 (indices: it+3), and
        // then runs the six groups on buf.  The end wait names every staging register, so only landed values cross the
        // barrier.  The steps are peeled by what is left of the list (no run-time condition between a load and its wait):
        // (true, true) while it+2 < i1, (true, false) for it+2 == i1, (false, false) for the last tile.
        int k_after2 = (i0 + 3 < i1) ? kl[i0 + 3] : 0;
        if (i0 + 1 < i1) {                                // tile i0+1's B operand, and the indices of tile i0+2
            if (gen) {
                alphas(k_next);
                weights(k_next);
                indices(k_after);
            } else {
                load_rows(k_next);
            }
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(xb[0][0]), "+v"(xb[0][1]), "+v"(xb[1][0]), "+v"(xb[1][1]), "+v"(w[0]),
                         "+v"(w[1]), "+v"(idx[0]), "+v"(idx[1])::"memory");
        }
        __syncthreads();
        int it = i0;
        auto late_step = [&](auto store, auto load) {
            const int k_after3 = (it + 4 < i1) ? kl[it + 4] : 0;
            if constexpr (decltype(store)::value) {
                store_b(buf ^ 1, 0);
                store_b(buf ^ 1, 1);
                stage_a(buf ^ 1, k_next);
            }
            if constexpr (decltype(load)::value) {
                if (gen) {
                    alphas(k_after);
                    weights(k_after);
                    indices(k_after2);                    // K tile 0 past the list's end: unused, but always 2 loads
                } else {
                    load_rows(k_after);
                }
            }
            __builtin_amdgcn_sched_barrier(0);            // staging first: no fragment read moves up into it
            SplitFrag f;
            split_group(t, lds, buf, 0, 0, f, acc);
            split_group(t, lds, buf, 0, 1, f, acc);
            split_group(t, lds, buf, 0, 2, f, acc);
            split_group(t, lds, buf, 1, 0, f, acc);
            split_group(t, lds, buf, 1, 1, f, acc);
            split_group(t, lds, buf, 1, 2, f, acc);
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(xb[0][0]), "+v"(xb[0][1]), "+v"(xb[1][0]), "+v"(xb[1][1]), "+v"(w[0]),
                         "+v"(w[1]), "+v"(idx[0]), "+v"(idx[1])::"memory");
            __syncthreads();
            buf ^= 1;
            k_next = k_after;
            k_after = k_after2;
            k_after2 = k_after3;
            ++it;
        };
        while (it + 2 < i1) late_step(std::true_type{}, std::true_type{});
        if (it + 1 < i1) late_step(std::true_type{}, std::false_type{});
        late_step(std::false_type{}, std::false_type{});
        return;
    }
    __syncthreads();
    for (int it = i0; it < i1; ++it) {
        int k_after2 = 0;
        const bool more = it + 1 < i1;                    // block-uniform
        // Issue order (vector memory returns in order, so the waits below count): gen -- the next tile's alpha loads
        // (their indices arrived during the previous step) and weights, the indices of the tile after it, then the 4 A
        // DMA loads; else the 4 B row loads, then the 4 A DMA loads.
        if (more) {
            if (gen) {
                alphas(k_next);
                weights(k_next);
                indices(k_after);                         // K tile 0 past the list's end: unused, but always 2 loads
            } else {
                load_rows(k_next);
            }
            stage_a(buf ^ 1, k_next);
            if (it + 3 < i1) k_after2 = kl[it + 3];
        }
        if constexpr (SCHED == SPLIT_SCHED_PIPELINED) {
            // Fragment reads run one MFMA group ahead of their use, and the wait in front of a group is counted: it
            // retires that group's reads and leaves the next group's in flight under the matrix pipe.  Four slots: hi A in
            // a[0], lo A in a[1]; the B slots swap roles every k-half.  A slot is read again once the last group that uses
            // it has issued.  Terms, blocks and operand bits are split_group's, so the sums are bit-identical.
            SplitSlots f;
            split_read_a(t, lds, buf, 0, false, f.a[0]);
            split_read_b(t, lds, buf, 0, false, f.b[0]);
            split_read_b(t, lds, buf, 0, true, f.b[1]);
            split_wait_ab(2, f.a[0], f.b[0]);
            split_mfma8(f.a[0], f.b[0], acc);                 // k-half 0: bh gh
            __builtin_amdgcn_sched_barrier(0);
            split_read_a(t, lds, buf, 0, true, f.a[1]);
            split_wait_b(4, f.b[1]);
            split_mfma8(f.a[0], f.b[1], acc);                 //           bh gl
            __builtin_amdgcn_sched_barrier(0);
            split_read_a(t, lds, buf, 1, false, f.a[0]);
            split_read_b(t, lds, buf, 1, false, f.b[1]);
            split_wait_a(6, f.a[1]);
            split_mfma8(f.a[1], f.b[0], acc);                 //           bl gh
            __builtin_amdgcn_sched_barrier(0);
            split_read_b(t, lds, buf, 1, true, f.b[0]);
            split_wait_ab(2, f.a[0], f.b[1]);
            split_mfma8(f.a[0], f.b[1], acc);                 // k-half 1: bh gh
            __builtin_amdgcn_sched_barrier(0);
            split_read_a(t, lds, buf, 1, true, f.a[1]);
            split_wait_b(4, f.b[0]);
            if (more) wait_and_store_b0(buf ^ 1);
            split_mfma8(f.a[0], f.b[0], acc);                 //           bh gl
            __builtin_amdgcn_sched_barrier(0);
            split_wait_a(0, f.a[1]);                          // the last reads, and the B stores if any: they count too
            if (more) store_b(buf ^ 1, 1);
            split_mfma8(f.a[1], f.b[1], acc);                 //           bl gh
        } else {
            SplitFrag f;
            split_group(t, lds, buf, 0, 0, f, acc);
            split_group(t, lds, buf, 0, 1, f, acc);
            split_group(t, lds, buf, 0, 2, f, acc);
            split_group(t, lds, buf, 1, 0, f, acc);
            if (more) wait_and_store_b0(buf ^ 1);
            split_group(t, lds, buf, 1, 1, f, acc);
            if (more) store_b(buf ^ 1, 1);
            split_group(t, lds, buf, 1, 2, f, acc);
        }
        asm volatile("s_waitcnt vmcnt(0)" : "+v"(idx[0]), "+v"(idx[1])::"memory");
        __syncthreads();
        buf ^= 1;
        k_next = k_after;
        k_after = k_after2;
    }
}

// A: the belief block's split plane.  fb.mat == nullptr: every B tile is read from fp32 rows (the projected route); else
// scheduler 2b's tiles (R = 1).
template <int SCHED, bool STAG>
__device__ __forceinline__ void gemm_split_streamk_body(const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
                                                        FusedB fb, SlabOut out, StreamKView v) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    streamk_walk(v, out, [&](const TileThread& t, int p, int tm, int tn, int lo, int hi, auto& acc) {
        const float* Ablk = A + (int64_t)tm * 256 * lda;
        if (fb.mat == nullptr || fb.mat[tn]) {           // block-uniform: fp32 rows from B
            const int bt = (fb.mat != nullptr && fb.ctile != nullptr) ? fb.ctile[tn] : tn;
            tile_run_split<SCHED, STAG>(t, lds, Ablk, lda, B + (int64_t)bt * 256 * ldb, ldb, false, nullptr, nullptr, nullptr, 0,
                                  0.f, v.klist + (int64_t)p * v.k_tiles, lo, hi, acc);
        } else {
            const int r0 = tn * 256;
            const int g = r0 / fb.V, v0 = r0 - g * fb.V;
            tile_run_split<SCHED, STAG>(t, lds, Ablk, lda, nullptr, 0, true, fb.rs + (int64_t)(g / fb.O) * fb.S_pad,
                                  fb.rto + (int64_t)g * fb.S_pad, fb.alpha + (int64_t)(v0 + (threadIdx.x >> 2)) * fb.lda,
                                  (int64_t)128 * fb.lda, fb.gamma, v.klist + (int64_t)p * v.k_tiles, lo, hi, acc);
        }
    });
}

__global__ __launch_bounds__(512) void k_gemm_split_streamk(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, FusedB fb, float* __restrict__ C, int ldc,
    int64_t slab_stride, int tiles_m, int pairs, int k_tiles, const int* __restrict__ klist, const int* __restrict__ kcount,
    const int* __restrict__ prefix, const int* __restrict__ start_pair, const int* __restrict__ first_block,
    const int* __restrict__ plan, int ovh) {
    gemm_split_streamk_body<SPLIT_SCHED_PARENT, false>(A, lda, B, ldb, fb, SlabOut{C, ldc, slab_stride},
        StreamKView{klist, kcount, prefix, start_pair, first_block, plan, tiles_m, pairs, k_tiles, ovh});
}
// The pipelined K-step schedule on the same plan, lists and slabs (pbvi_debug_split_schedule)
__global__ __launch_bounds__(512) void k_gemm_split_streamk_pipelined(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, FusedB fb, float* __restrict__ C, int ldc,
    int64_t slab_stride, int tiles_m, int pairs, int k_tiles, const int* __restrict__ klist, const int* __restrict__ kcount,
    const int* __restrict__ prefix, const int* __restrict__ start_pair, const int* __restrict__ first_block,
    const int* __restrict__ plan, int ovh) {
    gemm_split_streamk_body<SPLIT_SCHED_PIPELINED, false>(A, lda, B, ldb, fb, SlabOut{C, ldc, slab_stride},
        StreamKView{klist, kcount, prefix, start_pair, first_block, plan, tiles_m, pairs, k_tiles, ovh});
}

// The parent schedule with the block's two wave halves staggered by role (pbvi_debug_split_stagger): waves 0-3 run the
// parent step, waves 4-7 stage first and multiply last.  Same plan, lists, LDS image and slabs.
__global__ __launch_bounds__(512) void k_gemm_split_streamk_staggered(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb, FusedB fb, float* __restrict__ C, int ldc,
    int64_t slab_stride, int tiles_m, int pairs, int k_tiles, const int* __restrict__ klist, const int* __restrict__ kcount,
    const int* __restrict__ prefix, const int* __restrict__ start_pair, const int* __restrict__ first_block,
    const int* __restrict__ plan, int ovh) {
    gemm_split_streamk_body<SPLIT_SCHED_PARENT, true>(A, lda, B, ldb, fb, SlabOut{C, ldc, slab_stride},
        StreamKView{klist, kcount, prefix, start_pair, first_block, plan, tiles_m, pairs, k_tiles, ovh});
}

// One wave: does the split path keep subnormal lo parts and subnormal products?  out[0] = 1 if
//   x = (1 + 2^-7) 2^-120 + 2^-132 (a bf16-subnormal lo) times 1 comes back as x, and 2^-100 * 2^-30 as 2^-130.
__global__ void k_split_probe(float* out) {
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float x = 0x1.02p-120f + 0x1p-132f;
    if (h == 0) {
        a[0] = x;                                        // A[r][0]
        a[1] = 0x1p-100f;                                // A[r][1]
        if (r == 0) b[0] = 1.f;                          // B[0][0]
        if (r == 1) b[1] = 0x1p-30f;                     // B[1][1]
    }
    i32x4 ah, al, bh, bl;
    uint32_t hh, ll;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        split_pair(a[2 * p], a[2 * p + 1], hh, ll); ah[p] = (int)hh; al[p] = (int)ll;
        split_pair(b[2 * p], b[2 * p + 1], hh, ll); bh[p] = (int)hh; bl[p] = (int)ll;
    }
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bh), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ah), __builtin_bit_cast(bf16x8, bl), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, al), __builtin_bit_cast(bf16x8, bh), acc, 0, 0, 0);
    // C[0][c] sits in register 0 of lane c (h = 0)
    if (lane < 2) out[lane] = acc[0];
    if (lane == 0) out[2] = x;
}

// Probed once per device (engine creation), on a stream of its own; the result is cached under a lock.
int gemm_split_supported(int device) {
    static std::mutex mu;
    static std::map<int, int> known;
    std::lock_guard<std::mutex> lock(mu);
    auto it = known.find(device);
    if (it != known.end()) return it->second;
    int ok = 0;
    float* d = nullptr;
    hipStream_t st = nullptr;
    float h[3] = {0.f, 0.f, 0.f};
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipMalloc((void**)&d, sizeof(h)) == hipSuccess) {
        hipLaunchKernelGGL(k_split_probe, dim3(1), dim3(64), 0, st, d);
        if (hipGetLastError() == hipSuccess && hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, st) == hipSuccess &&
            hipStreamSynchronize(st) == hipSuccess)
            ok = (h[0] == h[2] && h[1] == 0x1p-130f) ? 1 : 0;
    }
    (void)hipGetLastError();
    if (d != nullptr) (void)hipFree(d);
    if (st != nullptr) (void)hipStreamDestroy(st);
    known[device] = ok;
    return ok;
}

// --------------------------------------------------------------------------- //
// Zero-tile bookkeeping
// --------------------------------------------------------------------------- //
// nz[tile][kt] = 1 iff the 256-row x 32-column block of X has a non-zero entry.
__global__ void k_tile_nonzero(const float* __restrict__ X, int ld, int k_tiles, uint8_t* __restrict__ nz) {
    const int tile = blockIdx.y;
    const int row = tile * 256 + threadIdx.x;
    const f32x4* p = (const f32x4*)(X + (int64_t)row * ld);
    for (int j = 0; j < 8; ++j) {
        const int kt = blockIdx.x * 8 + j;
        if (kt >= k_tiles) break;                       // block-uniform
        int f = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const f32x4 v = p[kt * 8 + c];
            f |= (v[0] != 0.f) | (v[1] != 0.f) | (v[2] != 0.f) | (v[3] != 0.f);
        }
        const int any = __syncthreads_or(f);
        if (threadIdx.x == 0) nz[(int64_t)tile * k_tiles + kt] = any ? 1 : 0;
    }
}

// One block per (m-tile, n-tile[, batch]) pair: compact the K tiles where both operands are non-zero.
// B's zero structure: G > 0 -> per row group, rows [g*v_group, (g+1)*v_group) share nzB[g][kt] (Gamma rows of
// one (action, observation)); rows >= G*v_group (magnitude and reward rows) may touch any group or the extra
// support row nzB[G] (so nzB is [G+1][k_tiles]); G == 0 -> per n-tile flags nzB[batch][tn][kt]; nzB == nullptr
// -> dense.
// irr != nullptr (fused projection): an entry of a tile that lies inside one row group carries, in bit KL_IRR_BIT, whether
// its K tile needs gathers for that group's action (irr[a][kt], a = group / groups_per_action); consumers mask it off.
__global__ void k_build_klists(const uint8_t* __restrict__ nzA, const uint8_t* __restrict__ nzB, int G,
                               int v_group, int n_rows, int tiles_m, int k_tiles, int chunk_len, int force_dense,
                               int* __restrict__ klist, int* __restrict__ kcount, int* __restrict__ nchunks,
                               const int32_t* __restrict__ irr, int groups_per_action) {
    __shared__ int wcount[4];
    __shared__ int total;
    const int tiles_n = gridDim.x / tiles_m;
    const int batch = blockIdx.y;
    const int tm = blockIdx.x % tiles_m, tn = blockIdx.x / tiles_m;
    const int pair = (batch * tiles_n + tn) * tiles_m + tm;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int r0 = tn * 256;
    int r1 = r0 + 255;
    if (r1 >= n_rows) r1 = n_rows - 1;
    int g0 = 0, g1 = -1;                                // group range touched by this n-tile
    if (nzB != nullptr && G > 0 && r0 < n_rows) {
        if (r1 >= G * v_group) {                        // tail tile: magnitude + reward rows; nzB has a G-th row
            g0 = 0;                                     // for the reward rows' support
            g1 = G;
        } else {
            g0 = r0 / v_group;
            g1 = r1 / v_group;
        }
    }
    if (tid == 0) total = 0;
    __syncthreads();
    for (int base = 0; base < k_tiles; base += 256) {
        const int kt = base + tid;
        int f = 0;
        if (force_dense) {
            f = kt < k_tiles;
        } else if (kt < k_tiles && r0 < n_rows && nzA[(int64_t)tm * k_tiles + kt]) {
            if (nzB == nullptr) {
                f = 1;
            } else if (G == 0) {
                f = nzB[((int64_t)batch * tiles_n + tn) * k_tiles + kt];
            } else {
                for (int g = g0; g <= g1; ++g) f |= nzB[(int64_t)g * k_tiles + kt];
            }
        }
        const unsigned long long mask = __ballot(f);
        if (lane == 0) wcount[wid] = __popcll(mask);
        __syncthreads();
        int off = total;
        for (int w = 0; w < wid; ++w) off += wcount[w];
        if (f) {
            int entry = kt;
            if (irr != nullptr && g0 == g1 && g1 < G && irr[(int64_t)(g0 / groups_per_action) * k_tiles + kt]) entry |= 1 << KL_IRR_BIT;
            klist[(int64_t)pair * k_tiles + off + __popcll(mask & ((1ull << lane) - 1ull))] = entry;
        }
        __syncthreads();
        if (tid == 0) total += wcount[0] + wcount[1] + wcount[2] + wcount[3];
        __syncthreads();
    }
    if (tid == 0) {
        kcount[pair] = total;
        nchunks[pair] = (total + chunk_len - 1) / chunk_len;    // stream-K overwrites this in k_streamk_plan
    }
}

// The process-wide environment knobs of the fp32 GEMM, read once
struct GemmEnv {
    int dense;        // PBVI_GEMM_DENSE=1: every K tile of every pair listed, zero or not (also pbvi_debug_gemm_dense): what
                      // BASELINE's "dense backup" configuration is measured with.  Results are unchanged (zero tiles add +0).
    int chunk;        // PBVI_GEMM_CHUNK=n: K chunk of the non-persistent scheduler, in tiles
    int no_streamk;   // PBVI_GEMM_NO_STREAMK=1: the non-persistent scheduler for score GEMMs too
    int ovh;          // PBVI_STREAMK_OVH=n: per-pair fixed cost of the stream-K plan, in tile-steps
    int no_stagger;   // PBVI_NO_SPLIT_STAGGER=1: the split score GEMM's lockstep kernel (debugging and A/B only)
};
static int env_int(const char* name, int dflt) { return getenv(name) ? atoi(getenv(name)) : dflt; }
static const GemmEnv& gemm_env() {
    static const GemmEnv env{env_int("PBVI_GEMM_DENSE", 0) != 0, env_int("PBVI_GEMM_CHUNK", 0), env_int("PBVI_GEMM_NO_STREAMK", 0),
                             env_int("PBVI_STREAMK_OVH", 1), env_int("PBVI_NO_SPLIT_STAGGER", 0) != 0};
    return env;
}

static int g_force_dense = -1;                     // set_gemm_force_dense overrides the environment
int gemm_force_dense() { return g_force_dense < 0 ? gemm_env().dense : g_force_dense; }
int set_gemm_force_dense(int enable) {
    const int prev = gemm_force_dense();
    g_force_dense = enable ? 1 : 0;
    return prev;
}

// Which K-step schedule the split score GEMM runs (pbvi_debug_split_schedule): process-wide, for the test that holds
// the two schedules' slabs bit-equal.  Not a tuning knob.
static int g_split_schedule = SPLIT_SCHED_PARENT;
int set_gemm_split_schedule(int schedule) {
    const int prev = g_split_schedule;
    if (schedule == SPLIT_SCHED_PARENT || schedule == SPLIT_SCHED_PIPELINED) g_split_schedule = schedule;
    return prev;
}

// Whether the parent schedule runs with its wave halves staggered (pbvi_debug_split_stagger): a second, independent
// switch, process-wide.  Bit-identical slabs (tests/test_split_stagger.py); measurements: profiles/split_stagger.md.
static int g_split_stagger = -1;                   // set_gemm_split_stagger overrides the environment
static int gemm_split_stagger() { return g_split_stagger < 0 ? !gemm_env().no_stagger : g_split_stagger; }
int set_gemm_split_stagger(int on) {
    const int prev = gemm_split_stagger();
    g_split_stagger = on ? 1 : 0;
    return prev;
}

int choose_chunk_len(int tiles_mn, int k_tiles) {
    if (const int v = gemm_env().chunk; v > 0) return v < k_tiles ? v : k_tiles;
    const int64_t total = (int64_t)tiles_mn * k_tiles;
    int64_t len = total / (256 * 8);
    if (len < 8) len = 8;
    if (len > 96) len = 96;
    if (len > k_tiles) len = k_tiles;
    return (int)len;
}

static int device_cu_count() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            cus = prop.multiProcessorCount;
        if (cus <= 0) cus = 256;
    }
    return cus;
}

hipError_t launch_tile_nonzero_f32(const float* X, int ld, int rows_pad, int k_tiles, uint8_t* nz, hipStream_t stream) {
    dim3 grid((k_tiles + 7) / 8, rows_pad / 256);
    hipLaunchKernelGGL(k_tile_nonzero, grid, dim3(256), 0, stream, X, ld, k_tiles, nz);
    return hipGetLastError();
}

// The stream-K kernels: which one runs for (split, schedule, stagger, fused, R), and the dynamic LDS it needs.  ANY
// matches every value; the first matching row counts.  The stagger exists for the parent schedule only: with the
// pipelined schedule selected the lockstep pipelined kernel runs whatever the stagger switch says.  set_lds_attr walks
// the same rows, so a kernel added here is also configured.
using StreamKKernel = void (*)(const float*, int, const float*, int, FusedB, float*, int, int64_t, int, int, int, const int*,
                               const int*, const int*, const int*, const int*, const int*, int);
struct StreamKKernelRow {
    int split, schedule, stagger, fused, R;
    StreamKKernel kernel;
    int lds_bytes;
};
constexpr int ANY = -1;
static const StreamKKernelRow STREAMK_KERNELS[] = {
    {1, SPLIT_SCHED_PARENT, 1, ANY, ANY, k_gemm_split_streamk_staggered, GEMM_LDS_BYTES},
    {1, SPLIT_SCHED_PARENT, 0, ANY, ANY, k_gemm_split_streamk, GEMM_LDS_BYTES},
    {1, SPLIT_SCHED_PIPELINED, ANY, ANY, ANY, k_gemm_split_streamk_pipelined, GEMM_LDS_BYTES},
    {0, ANY, ANY, 0, ANY, k_gemm_nt_f32_streamk, GEMM_LDS_BYTES},
    {0, ANY, ANY, 1, 1, k_gemm_nt_f32_streamk_fused, GEMM_LDS_BYTES},
    {0, ANY, ANY, 1, 2, k_gemm_nt_f32_streamk_fused_r<2>, GEMM_LDS_BYTES_R},
    {0, ANY, ANY, 1, 3, k_gemm_nt_f32_streamk_fused_r<3>, GEMM_LDS_BYTES_R},
    {0, ANY, ANY, 1, 4, k_gemm_nt_f32_streamk_fused_r<4>, GEMM_LDS_BYTES_R},
    {0, ANY, ANY, 1, 5, k_gemm_nt_f32_streamk_fused_r<5>, GEMM_LDS_BYTES_R},
    {0, ANY, ANY, 1, 6, k_gemm_nt_f32_streamk_fused_r<6>, GEMM_LDS_BYTES_R},
    {0, ANY, ANY, 1, 7, k_gemm_nt_f32_streamk_fused_r<7>, GEMM_LDS_BYTES_R},
};
// nullptr: no such kernel (a fused R outside 1..FUSED_R_MAX)
static const StreamKKernelRow* streamk_kernel(int split, int schedule, int stagger, int fused, int R) {
    auto fits = [](int want, int have) { return want == ANY || want == have; };
    for (const StreamKKernelRow& row : STREAMK_KERNELS)
        if (fits(row.split, split) && fits(row.schedule, schedule) && fits(row.stagger, stagger) &&
            fits(row.fused, fused) && fits(row.R, R)) return &row;
    return nullptr;
}

static hipError_t set_lds_attr() {
    static bool done = false;
    if (done) return hipSuccess;
    hipError_t e = hipFuncSetAttribute((const void*)k_gemm_nt_f32_mfma, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       GEMM_LDS_BYTES);
    for (const StreamKKernelRow& row : STREAMK_KERNELS)
        if (e == hipSuccess) e = hipFuncSetAttribute((const void*)row.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, row.lds_bytes);
    done = e == hipSuccess;
    return e;
}

// The tile lists (and, for stream-K, the plan) depend on the zero maps only, not on the operands' values.
static hipError_t build_klists(const GemmArgs& a, int batch, const FusedB* fused, hipStream_t ls) {
    if (batch < 1 || batch > 65535) return hipErrorInvalidValue;
    const GemmPlan& pl = a.plan;
    hipLaunchKernelGGL(k_build_klists, dim3(pl.tiles_m * pl.tiles_n, batch), dim3(256), 0, ls, a.nzA, a.nzB, a.G, a.v_group,
                       a.n_rows, pl.tiles_m, pl.k_tiles, pl.chunk_len, gemm_force_dense(), a.klist, a.kcount, a.nchunks,
                       fused != nullptr ? fused->irr : nullptr, fused != nullptr ? fused->O : 1);
    return hipGetLastError();
}

// scheduler 1 over built lists
static hipError_t launch_mfma(const GemmArgs& a, int batch, int64_t batch_stride_b, int64_t batch_stride_c) {
    const GemmPlan& pl = a.plan;
    const int64_t groups = ((int64_t)pl.tiles_n * pl.max_chunks + 7) / 8 * 8;
    const int64_t total = groups * pl.tiles_m;
    if (total <= 0 || total > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gemm_nt_f32_mfma, dim3((unsigned)total, batch), dim3(512), GEMM_LDS_BYTES, a.stream, a.A, a.lda, a.B,
                       a.ldb, a.C, pl.ldc, pl.slab_stride, pl.tiles_m, pl.tiles_n, pl.k_tiles, pl.chunk_len, pl.max_chunks,
                       a.klist, a.kcount, batch_stride_b, batch_stride_c);
    return hipGetLastError();
}

hipError_t launch_score_gemm_f32(const ScoreGemmArgs& a) {
    hipError_t e = set_lds_attr();
    if (e != hipSuccess) return e;
    const GemmPlan& pl = a.plan;
    const int fused_R = a.fused != nullptr ? a.fused->R : 1;
    if (pl.streamk ? a.streamk_ws == nullptr : (a.fused != nullptr || a.split)) return hipErrorInvalidValue;
    if (a.split && fused_R != 1) return hipErrorInvalidValue;
    // With a list stream the lists and the plan are built beside whatever `stream` is still doing (the Gamma projection)
    // and the GEMM waits for them.
    hipStream_t ls = (a.list_stream != nullptr && a.list_event != nullptr) ? a.list_stream : a.stream;
    if ((e = build_klists(a, 1, a.fused, ls)) != hipSuccess) return e;
    const int pairs = pl.tiles_m * pl.tiles_n, ovh = gemm_env().ovh;
    const StreamKWorkspace ws = streamk_workspace(pl, a.streamk_ws);
    if (pl.streamk) {
        hipLaunchKernelGGL(k_streamk_plan, dim3(1), dim3(256), 0, ls, a.kcount, pairs, pl.nblocks, pl.k_tiles, pl.max_chunks - 1,
                           ovh, ws.prefix, ws.start_pair, ws.first_block, a.nchunks, ws.plan);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (ls != a.stream) {
        if ((e = hipEventRecord(a.list_event, ls)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(a.stream, a.list_event, 0)) != hipSuccess) return e;
    }
    if (!pl.streamk) return launch_mfma(a, 1, 0, 0);
    const StreamKKernelRow* row = streamk_kernel(a.split ? 1 : 0, g_split_schedule, gemm_split_stagger(), a.fused != nullptr, fused_R);
    if (row == nullptr) return hipErrorInvalidValue;
    const FusedB fb = a.fused != nullptr ? *a.fused : FusedB{};   // (no fused: fb.mat == nullptr, every B tile from fp32 rows)
    hipLaunchKernelGGL(row->kernel, dim3(pl.nblocks), dim3(512), row->lds_bytes, a.stream, a.A, a.lda, a.B, a.ldb, fb, a.C, pl.ldc,
                       pl.slab_stride, pl.tiles_m, pairs, pl.k_tiles, a.klist, a.kcount, ws.prefix, ws.start_pair, ws.first_block,
                       ws.plan, ovh);
    return hipGetLastError();
}

hipError_t launch_batched_gemm_f32(const BatchedGemmArgs& a) {
    hipError_t e = set_lds_attr();
    if (e != hipSuccess) return e;
    if (a.plan.streamk) return hipErrorInvalidValue;
    if ((e = build_klists(a, a.batch, nullptr, a.stream)) != hipSuccess) return e;
    if (a.ev_before != nullptr && (e = hipEventRecord(a.ev_before, a.stream)) != hipSuccess) return e;
    if ((e = launch_mfma(a, a.batch, a.batch_stride_b, a.batch_stride_c)) != hipSuccess) return e;
    if (a.ev_after != nullptr && (e = hipEventRecord(a.ev_after, a.stream)) != hipSuccess) return e;
    return hipSuccess;
}

GemmPlan make_gemm_plan(int M_pad, int N_pad, int K_pad, bool single_chunk) {
    GemmPlan pl;
    pl.tiles_m = M_pad / GEMM_BM;
    pl.tiles_n = N_pad / GEMM_BN;
    pl.k_tiles = K_pad / GEMM_BK;
    pl.ldc = N_pad;
    pl.slab_stride = (int64_t)M_pad * N_pad;
    pl.streamk = !single_chunk && !gemm_env().no_streamk;
    pl.nblocks = device_cu_count();
    if (single_chunk) {
        pl.chunk_len = pl.k_tiles;
        pl.max_chunks = 1;
    } else if (pl.streamk) {
        // a pair's list (<= k_tiles steps) is split over at most max_split+1 consecutive blocks
        const int max_split = 8;
        pl.chunk_len = pl.k_tiles;          // only used for the (overwritten) provisional nchunks
        pl.max_chunks = max_split + 1;
        pl.c_floats = pl.slab_stride + (int64_t)pl.nblocks * (256 * 256);
        return pl;
    } else {
        pl.chunk_len = choose_chunk_len(pl.tiles_m * pl.tiles_n, pl.k_tiles);
        pl.max_chunks = (pl.k_tiles + pl.chunk_len - 1) / pl.chunk_len;
    }
    pl.c_floats = (int64_t)pl.max_chunks * pl.slab_stride;
    return pl;
}

// --------------------------------------------------------------------------- //
// Plain tiled GEMM for any T / any shape (f64 engines, small models).
// --------------------------------------------------------------------------- //
template <typename T>
__global__ void k_gemm_nt_simple(const T* __restrict__ A, int lda, const T* __restrict__ B, int ldb,
                                 T* __restrict__ C, int ldc, int M, int N, int K) {
    __shared__ T As[16][17];
    __shared__ T Bs[16][17];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int m = blockIdx.y * 16 + ty, n = blockIdx.x * 16 + tx;
    T acc = 0;
    for (int k0 = 0; k0 < K; k0 += 16) {
        const int ka = k0 + tx;
        const int ma = blockIdx.y * 16 + ty, nb = blockIdx.x * 16 + ty;
        As[ty][tx] = (ma < M && ka < K) ? A[(int64_t)ma * lda + ka] : T(0);
        Bs[ty][tx] = (nb < N && ka < K) ? B[(int64_t)nb * ldb + ka] : T(0);
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc += As[ty][kk] * Bs[tx][kk];
        __syncthreads();
    }
    if (m < M && n < N) C[(int64_t)m * ldc + n] = acc;
}

template <typename T>
hipError_t launch_gemm_nt_simple(const T* A, int lda, const T* B, int ldb, T* C, int ldc, int M, int N,
                                 int K, hipStream_t stream) {
    if (M <= 0 || N <= 0) return hipSuccess;
    dim3 grid((N + 15) / 16, (M + 15) / 16), block(16, 16);
    hipLaunchKernelGGL(k_gemm_nt_simple<T>, grid, block, 0, stream, A, lda, B, ldb, C, ldc, M, N, K);
    return hipGetLastError();
}

template hipError_t launch_gemm_nt_simple<float>(const float*, int, const float*, int, float*, int, int, int, int, hipStream_t);
template hipError_t launch_gemm_nt_simple<double>(const double*, int, const double*, int, double*, int, int, int, int, hipStream_t);

}  // namespace pbvi
