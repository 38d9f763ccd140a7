// split_f16.hip.h -- the split-fp16 operand arithmetic behind every fast matrix product of the library.
//
// An fp32 operand v is carried as two fp16 halves, hi = fp16(v) and lo = fp16((v - hi) 2^11): 22 of v's 24 mantissa bits.
// A product sum is three v_mfma_f32_16x16x32_f16 (hi hi, hi lo, lo hi; lo lo is dropped: at most 2^-22 of the product)
// accumulated in fp32,
//     sum a b = sum a_hi b_hi + 2^-11 (sum a_hi b_lo + sum a_lo b_hi),
// with the 2^-11 (SPLIT_INV) folded back in the epilogue: the fp32 matrix instruction's error against float64 at 3/16 of
// its cycles.  What a kernel does with the halves -- layouts, pipelining, epilogues -- stays in the kernel's file.
//
// fp16 is narrow.  The inference kernels (block_attn.hip, ffn.hip, compress_ws.hip, compress_fused.hip) rely on the caller
// for the operands' range (fused.py); the training-path kernels (linear_rows_h.hip, pfn_fused.hip, pfn_sorted.hip,
// split_conv.hip.h) normalise every row / weight matrix by an exact power of two first (pow2_norm) and undo it in the
// epilogue, so the halves always see values in (-2, 2) -- (-4, 4) for a maximum in [2^127, FLT_MAX].
#pragma once
#include "common.hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));  // what __builtin_amdgcn_cvt_pkrtz returns

#define SPLIT_SCALE 2048.0f
#define SPLIT_INV (1.0f / 2048.0f)
#define MFMA_H(acc, av, bv) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16((av), (bv), acc, 0, 0, 0)
#define MFMA_H16(acc, av, bv) acc = __builtin_amdgcn_mfma_f32_16x16x16f16((av), (bv), acc, 0, 0, 0)
#define MFMA4(acc, av, bv) acc = __builtin_amdgcn_mfma_f32_16x16x4f32((av), (bv), acc, 0, 0, 0)

// ---- the splits ----------------------------------------------------------------------------------------------------------
// In all of them (v - hi) 2^11 is computed as fma(hi, -2^11, v 2^11): every step is exact, so the bits are those of the
// subtraction form, and the fp16 -> fp32 conversion of hi rides inside the instruction (v_fma_mix_f32).
//
// 4 values, both halves rounded TOWARD ZERO, the 2^11 multiply PACKED (one v_pk_mul_f32 per pair).  split4_rtz_scalar below
// returns the same bits from other instructions: the two forms are bit-identical and their instruction selection is not,
// and each kernel is tuned around the one it has -- do not merge them without measuring.
__device__ __forceinline__ void split4_rtz(const f32x2 v01, const f32x2 v23, h16x4 &hi, h16x4 &lo) {
    const fp16x2 a = __builtin_amdgcn_cvt_pkrtz(v01[0], v01[1]), b = __builtin_amdgcn_cvt_pkrtz(v23[0], v23[1]);
    const f32x2 s01 = v01 * f32x2{SPLIT_SCALE, SPLIT_SCALE}, s23 = v23 * f32x2{SPLIT_SCALE, SPLIT_SCALE};
    const fp16x2 c = __builtin_amdgcn_cvt_pkrtz(__builtin_fmaf((float)a[0], -SPLIT_SCALE, s01[0]), __builtin_fmaf((float)a[1], -SPLIT_SCALE, s01[1])),
                 d = __builtin_amdgcn_cvt_pkrtz(__builtin_fmaf((float)b[0], -SPLIT_SCALE, s23[0]), __builtin_fmaf((float)b[1], -SPLIT_SCALE, s23[1]));
    hi = h16x4{(_Float16)a[0], (_Float16)a[1], (_Float16)b[0], (_Float16)b[1]};
    lo = h16x4{(_Float16)c[0], (_Float16)c[1], (_Float16)d[0], (_Float16)d[1]};
}
__device__ __forceinline__ void split4_rtz(const f32x4 v, h16x4 &hi, h16x4 &lo) {
    split4_rtz(f32x2{v[0], v[1]}, f32x2{v[2], v[3]}, hi, lo);
}
__device__ __forceinline__ void split4_rtz(const float v0, const float v1, const float v2, const float v3, h16x4 &hi, h16x4 &lo) {
    split4_rtz(f32x2{v0, v1}, f32x2{v2, v3}, hi, lo);
}
// 4 values, both halves rounded TOWARD ZERO, the 2^11 multiply as four SCALAR multiplies (see split4_rtz)
__device__ __forceinline__ void split4_rtz_scalar(const float v0, const float v1, const float v2, const float v3, h16x4 &hi, h16x4 &lo) {
    const fp16x2 a = __builtin_amdgcn_cvt_pkrtz(v0, v1), b = __builtin_amdgcn_cvt_pkrtz(v2, v3);
    const fp16x2 c = __builtin_amdgcn_cvt_pkrtz(__builtin_fmaf((float)a[0], -SPLIT_SCALE, v0 * SPLIT_SCALE), __builtin_fmaf((float)a[1], -SPLIT_SCALE, v1 * SPLIT_SCALE));
    const fp16x2 d = __builtin_amdgcn_cvt_pkrtz(__builtin_fmaf((float)b[0], -SPLIT_SCALE, v2 * SPLIT_SCALE), __builtin_fmaf((float)b[1], -SPLIT_SCALE, v3 * SPLIT_SCALE));
    hi = h16x4{(_Float16)a[0], (_Float16)a[1], (_Float16)b[0], (_Float16)b[1]};
    lo = h16x4{(_Float16)c[0], (_Float16)c[1], (_Float16)d[0], (_Float16)d[1]};
}
__device__ __forceinline__ h16x8 split_cat(const h16x4 a, const h16x4 b) { return h16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }
// 8 values as two quads through split4_rtz (packed form)
__device__ __forceinline__ void split8_rtz(const f32x4 v0, const f32x4 v1, h16x8 &hi, h16x8 &lo) {
    h16x4 h0, l0, h1, l1;
    split4_rtz(v0, h0, l0);
    split4_rtz(v1, h1, l1);
    hi = split_cat(h0, h1);
    lo = split_cat(l0, l1);
}

// 8 values scaled by s (an exact power of two: pow2_norm), both halves rounded TOWARD ZERO
__device__ __forceinline__ void split8_scaled_rtz(const float4 v0, const float4 v1, float s, h16x8 &hi, h16x8 &lo) {
    const float x[8] = {v0.x * s, v0.y * s, v0.z * s, v0.w * s, v1.x * s, v1.y * s, v1.z * s, v1.w * s};
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        const fp16x2 a = __builtin_amdgcn_cvt_pkrtz(x[i], x[i + 1]);
        const fp16x2 c = __builtin_amdgcn_cvt_pkrtz(__builtin_fmaf((float)a[0], -SPLIT_SCALE, x[i] * SPLIT_SCALE),
                                                    __builtin_fmaf((float)a[1], -SPLIT_SCALE, x[i + 1] * SPLIT_SCALE));
        hi[i] = (_Float16)a[0]; hi[i + 1] = (_Float16)a[1];
        lo[i] = (_Float16)c[0]; lo[i + 1] = (_Float16)c[1];
    }
}
// 8 values scaled by s, both halves rounded to NEAREST even (the convolutions, split_conv.hip.h): each operand is then off
// by at most 2^-23 of itself
__device__ __forceinline__ void split8_scaled_rne(const float4 v0, const float4 v1, float s, h16x8 &hi, h16x8 &lo) {
    const float x[8] = {v0.x * s, v0.y * s, v0.z * s, v0.w * s, v1.x * s, v1.y * s, v1.z * s, v1.w * s};
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        const h16x2 a = __builtin_convertvector((f32x2{x[i], x[i + 1]}), h16x2);
        // x 2^11 - hi 2^11: exact (the residual of a 24-bit value against its 11-bit rounding has at most 13 bits)
        const f32x2 r = {__builtin_fmaf((float)a[0], -SPLIT_SCALE, x[i] * SPLIT_SCALE),
                         __builtin_fmaf((float)a[1], -SPLIT_SCALE, x[i + 1] * SPLIT_SCALE)};
        const h16x2 c = __builtin_convertvector(r, h16x2);
        hi[i] = a[0]; hi[i + 1] = a[1];
        lo[i] = c[0]; lo[i + 1] = c[1];
    }
}

// ---- exact power-of-two normalisation ------------------------------------------------------------------------------------
// The exponent rule: from the bits of the largest magnitude, the word eb = E << 23 of its biased exponent E; false for zero
// / denormal and inf / nan maxima, which pass through unscaled.  Otherwise the words 0x7F000000 - eb and eb are the floats
// 2^(127 - E) and 2^(E - 127): scaling by them is exact, so it is undone exactly.
__device__ __forceinline__ bool pow2_norm_exponent(int max_abs_bits, int &eb) {
    eb = max_abs_bits & 0x7F800000;
    return eb != 0 && eb < 0x7F000000;
}
// pow2_norm covers E = 254 (maxima in [2^127, FLT_MAX]) too: 2^(127 - 254) is no normal float, so that row takes 2^-126 /
// 2^126 and lies in [2, 4), still far inside fp16 (unscaled, its halves would saturate at 65504: a finite, wrong sum).
// For E = 1 .. 253 the words are the ones above, bit for bit.
__device__ __forceinline__ void pow2_norm(float max_abs, float &s_in, float &un) {
    const int eb = __builtin_bit_cast(int, max_abs) & 0x7F800000;
    const bool norm = eb != 0 && eb <= 0x7F000000;
    const int sb = max(0x7F000000 - eb, 0x00800000);
    s_in = norm ? __builtin_bit_cast(float, sb) : 1.0f;
    un = norm ? __builtin_bit_cast(float, 0x7F000000 - sb) : 1.0f;
}
__device__ __forceinline__ float abs_max8(const float4 a, const float4 b) {
    return fmaxf(fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))),
                 fmaxf(fmaxf(fabsf(b.x), fabsf(b.y)), fmaxf(fabsf(b.z), fabsf(b.w))));
}

// ---- the weight image of a row product Y = X B^T ---------------------------------------------------------------------------
// B (N, K) staged once per workgroup of WAVES waves as ready MFMA fragments, hi and lo images in LDS as [k step][column
// tile][lane] x 16 bytes (one conflict-free ds_read_b128 per fragment): fragment (P, t, lane = 16 g + n % 16) =
// B[n = 16 t + lane % 16][k = 32 P + 8 g .. + 8), the whole matrix normalised by ONE power of two (any finite weight scale
// works).  Two parts, because the kernels stage their epilogue parameters between them (ahead of the first barrier).
// IGRAD: the kernel also takes the input-gradient form (`transpose_w`).
template <int K, int N, int WAVES, bool IGRAD = false>
struct WeightImage {
    static constexpr int KS = K / 32, NT = N / 16, IMG = KS * NT * 64;  // h16x8 fragments per (hi or lo) image
    static constexpr int THREADS = WAVES * MSSVT_WAVE, FR = (IMG + THREADS - 1) / THREADS;  // fragments per thread
    float4 v0[FR], v1[FR];

    // part 1: this thread's fragments of W (N, K) row-major -- or, with IGRAD and `transpose_w`, of W (K, N) row-major:
    // B[n][k] = W[k][n].  Returns their largest magnitude.
    __device__ __forceinline__ float load(const float *W, int transpose_w = 0) {
        float wmx = 0.f;
#pragma unroll
        for (int i = 0; i < FR; ++i) {
            const int f = threadIdx.x + i * THREADS;
            v0[i] = v1[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (f < IMG) {
                const int ln = f & 63, t = (f >> 6) % NT, P = (f >> 6) / NT;
                const int n = 16 * t + (ln & 15), k0 = 32 * P + 8 * (ln >> 4);
                if (!IGRAD || !transpose_w) {
                    v0[i] = *reinterpret_cast<const float4 *>(W + (size_t)n * K + k0);
                    v1[i] = *reinterpret_cast<const float4 *>(W + (size_t)n * K + k0 + 4);
                } else {
                    const float *c = W + (size_t)k0 * N + n;
                    v0[i] = make_float4(c[0], c[N], c[2 * N], c[3 * N]);
                    v1[i] = make_float4(c[4 * N], c[5 * N], c[6 * N], c[7 * N]);
                }
                wmx = fmaxf(wmx, abs_max8(v0[i], v1[i]));
            }
        }
        return wmx;
    }

    // part 2: the workgroup's maximum (one barrier), its power of two, the split images.  Returns 2^e, to undo it by.
    // The caller's barrier before the first fragment read publishes the images.
    __device__ __forceinline__ float store(float wmx, h16x8 *Bh, h16x8 *Bl) const {
        __shared__ float wmax_l[WAVES];
        wmx = wave_max(wmx);
        if (lane_id() == 0) wmax_l[threadIdx.x / MSSVT_WAVE] = wmx;
        __syncthreads();
        wmx = 0.f;
#pragma unroll
        for (int i = 0; i < WAVES; ++i) wmx = fmaxf(wmx, wmax_l[i]);
        float w_in, w_un;
        pow2_norm(wmx, w_in, w_un);
#pragma unroll
        for (int i = 0; i < FR; ++i) {
            const int f = threadIdx.x + i * THREADS;
            if (f < IMG) {
                h16x8 h, l;
                split8_scaled_rtz(v0[i], v1[i], w_in, h, l);
                Bh[f] = h;
                Bl[f] = l;
            }
        }
        return w_un;
    }
};

// ---- the 16-row tile product ---------------------------------------------------------------------------------------------
// One k step P of the Y^T tile of column tile t against the weight image above (A = the weights' rows n, B = the tile's rows
// m): mm += bh ah (hi hi), cr += bh al + bl ah (the cross terms); after all K / 32 steps the sum is mm + 2^-11 cr.
template <int NT>
__device__ __forceinline__ void split_product(f32x4 &mm, f32x4 &cr, const h16x8 *Bh, const h16x8 *Bl, int P, int t, int lane,
                                              const h16x8 ah, const h16x8 al) {
    const h16x8 bh = Bh[(P * NT + t) * 64 + lane], bl = Bl[(P * NT + t) * 64 + lane];
    MFMA_H(mm, bh, ah);
    MFMA_H(cr, bh, al);
    MFMA_H(cr, bl, ah);
}
