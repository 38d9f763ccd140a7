// bev_conv.hip.h -- the split-fp16 operand pieces shared by bev_conv.hip and head_conv.hip: the fragment types, the tile
// constants, the hi / lo split of eight floats and the magnitude-as-integer used by the exponent words.
#pragma once
#include "common.hip.h"

typedef float bc_f32x4 __attribute__((ext_vector_type(4)));
typedef float bc_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 bc_h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 bc_h16x2 __attribute__((ext_vector_type(2)));

#define BC_WAVES 8
#define BC_WAVE_PIXELS MSSVT_BEV_CONV_WAVE_PIXELS
#define BC_BLOCK_PIXELS MSSVT_BEV_CONV_BLOCK_PIXELS
#define BC_THREADS (BC_WAVES * MSSVT_WAVE)
#define BC_SCALE 2048.0f
#define BC_INV (1.0f / 2048.0f)
#define BC_HDR_BYTES 64  // blob: [w_in, w_un, 14 reserved floats][scale Cout][shift Cout][weight blocks]
#define BC_MFMA(acc, av, bv) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16((av), (bv), acc, 0, 0, 0)
static_assert(BC_WAVE_PIXELS == 32 && BC_BLOCK_PIXELS == BC_WAVES * BC_WAVE_PIXELS, "tile constants of the header");

#define BC_KC(CIN) ((CIN) < 128 ? (CIN) : 128)  // input channels per staged weight block
#define BC_NS(COUT) ((COUT) < 128 ? (COUT) : 128)  // output channels per workgroup (slice)

// 8 floats (scaled by the exact power of two s) -> hi and lo halves, both rounded to nearest even
__device__ __forceinline__ void bc_split8(const float4 v0, const float4 v1, float s, bc_h16x8 &hi, bc_h16x8 &lo) {
    const float x[8] = {v0.x * s, v0.y * s, v0.z * s, v0.w * s, v1.x * s, v1.y * s, v1.z * s, v1.w * s};
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        const bc_h16x2 a = __builtin_convertvector((bc_f32x2{x[i], x[i + 1]}), bc_h16x2);
        // x 2^11 - hi 2^11: exact (the residual of a 24-bit value against its 11-bit rounding has at most 13 bits)
        const bc_f32x2 r = {__builtin_fmaf((float)a[0], -BC_SCALE, x[i] * BC_SCALE),
                            __builtin_fmaf((float)a[1], -BC_SCALE, x[i + 1] * BC_SCALE)};
        const bc_h16x2 c = __builtin_convertvector(r, bc_h16x2);
        hi[i] = a[0]; hi[i + 1] = a[1];
        lo[i] = c[0]; lo[i + 1] = c[1];
    }
}

// |v| as an integer: ordered like the magnitudes, every NaN above infinity (fmaxf would drop a NaN)
__device__ __forceinline__ int bc_abs_bits(float v) { return __builtin_bit_cast(int, v) & 0x7FFFFFFF; }
