// The three-term bf16 operand split of the fp32 score GEMM (gemm.hip, scheduler 2d): x -> hi = RNE_bf16(sat(x)),
// lo = RNE_bf16(x - hi).  One definition for the GEMM's own register staging and for the engine's pre-split belief
// plane (engine.hip), so the two cannot produce different bits.
//
// Split plane layout: the same rows and 32-bit words as the fp32 operand ([rows][S_pad]); for row r and K tile kt the
// 32 words kt*32 .. kt*32+31 hold the 32 hi bf16 values (k 0-31, two per word, the lower k in bits 0-15), then the 32 lo
// values.  That is the split LDS image of the row before the XOR swizzle, so the fp32 operand's LDS-DMA staging
// (tile_stage) loads it into exactly the image the register staging writes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbvi {

__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));    // a -> bits 0-15, b -> bits 16-31, RNE
    return r;
}
__device__ __forceinline__ float bf16_sat(float x) {
    const float m = 0x1.fep127f;                                        // largest finite bf16
    return fabsf(x) > m ? copysignf(m, x) : x;                          // (a NaN stays a NaN)
}
__device__ __forceinline__ void split_pair(float x0, float x1, uint32_t& hi, uint32_t& lo) {
#pragma clang fp contract(off)
    hi = cvt_pk_bf16(bf16_sat(x0), bf16_sat(x1));
    const float h0 = __uint_as_float(hi << 16), h1 = __uint_as_float(hi & 0xffff0000u);
    lo = cvt_pk_bf16(x0 - h0, x1 - h1);
}

// 4 consecutive k (4j .. 4j+3 of a K tile) -> the 2 hi words (split plane words 2j, 2j+1 of the tile) and the 2 lo words
// (16 + 2j, 17 + 2j)
__device__ __forceinline__ void split_quad(float x0, float x1, float x2, float x3, uint2& hi, uint2& lo) {
    split_pair(x0, x1, hi.x, lo.x);
    split_pair(x2, x3, hi.y, lo.y);
}

}  // namespace pbvi
