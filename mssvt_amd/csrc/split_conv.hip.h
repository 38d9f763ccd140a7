// split_conv.hip.h -- y = act(scale[c] * conv(x, w) + shift[c]) on channels-last fp32 pixels with split-fp16 matrix operands:
// the one kernel (k_split_conv), exponent-word kernel and weight packer behind bev_conv.hip and head_conv.hip.
// The library runs these convolutions on the fp32 matrix instruction (1/16 of the 16-bit rate); here every operand is split
// into fp16 halves (the arithmetic of csrc/split_f16.hip.h), both rounded to NEAREST (split8_scaled_rne: each operand is then
// off by at most 2^-23 of itself and the dropped lo lo term is at most 2^-22 of the product).
//
// A convolution over channels-last pixels is one row-GEMM per tap accumulated into one tile: M = output pixels, N = output
// columns, K = taps x Cin.  Nothing per tap is ever written to global memory: the lanes of a wave read the tap's input pixel
// of THEIR output pixel straight from x (32 bytes per lane and k step; a pixel outside the image is produced as zeros, never
// loaded).
//
//   * a wave owns BC_WAVE_PIXELS = 32 consecutive output pixels (two 16-row operand tiles that share every weight fragment
//     read) and NS <= 128 output columns; all 2 x NS / 16 accumulator tiles (mm: hi hi, cr: the cross terms) stay in
//     registers over every tap and all of Cin -- one accumulation chain per output element;
//   * a workgroup is 8 waves = BC_BLOCK_PIXELS = 256 output pixels; blockIdx.y is a SLICE of NS output columns (the up-2
//     form numbers its workgroups itself: at the OUT enum);
//   * the weights arrive packed (k_split_pack): per (slice, tap, 128-channel chunk of Cin) one contiguous block holding the hi
//     and the lo image as ready operand fragments [k step][column tile][lane] x 16 bytes.  A block (<= 64 KiB) is copied into
//     one of two LDS buffers while the previous one is multiplied: one barrier per block;
//   * range: fp16 is narrow, so every OUTPUT pixel's operands are normalised by one exact power of two taken from the largest
//     exponent over its whole receptive field (k_split_expmap, or a previous launch's epilogue, leaves one word per input
//     pixel), and the weights by one power of two per header record (at pack time); both are undone in the epilogue, exactly.
//     Scaling the input by a power of two therefore scales the result bit for bit;
//   * the epilogue applies scale / shift in fp32 (the BatchNorm fold is NOT rounded into the fp16 weights), the activation,
//     and stores; every output element has exactly one writer, no atomics.
//
// blob: [nsl records of 16 bytes: float w_in (2^-e), float w_un (2^e), int k (columns in use), int kbase (maps before it);
// zero-padded to 64 bytes][scale nsl NS][shift nsl NS][per slice: its weight blocks].
#pragma once
#include "split_f16.hip.h"

#define BC_WAVES 8
#define BC_WAVE_PIXELS MSSVT_BEV_CONV_WAVE_PIXELS
#define BC_BLOCK_PIXELS MSSVT_BEV_CONV_BLOCK_PIXELS
#define BC_THREADS (BC_WAVES * MSSVT_WAVE)
#define BC_REC_BYTES 16
#define BC_HDR(NSL) ((((NSL) * BC_REC_BYTES) + 63) / 64 * 64)
static_assert(BC_WAVE_PIXELS == 32 && BC_BLOCK_PIXELS == BC_WAVES * BC_WAVE_PIXELS, "tile constants of the header");

#define BC_KC(CIN) ((CIN) < 128 ? (CIN) : 128)  // input channels per staged weight block

// |v| as an integer: ordered like the magnitudes, every NaN above infinity (fmaxf would drop a NaN)
__device__ __forceinline__ int bc_abs_bits(float v) { return __builtin_bit_cast(int, v) & 0x7FFFFFFF; }

static bool bc_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
static bool bc_too_many_pixels(int B, int H, int W) { return (long long)B * H * W > 0x7FFFFFFFll - 4 * BC_BLOCK_PIXELS; }

// ---- one word per row of a (rows, C) matrix: the largest |x| of the row, as bits; LPR lanes share a row ------------------
template <int C, int LPR>
__global__ void __launch_bounds__(256) k_split_expmap(const float *x, long long rows, int *emap) {
    constexpr int RPW = MSSVT_WAVE / LPR;  // rows per wave
    const int lane = lane_id(), sub = lane % LPR;
    const long long row = ((long long)blockIdx.x * 4 + threadIdx.x / MSSVT_WAVE) * RPW + lane / LPR;
    int m = 0;
    if (row < rows) {
#pragma unroll
        for (int c = 0; c < C / 4; c += LPR) {
            const float4 v = *reinterpret_cast<const float4 *>(x + (size_t)row * C + 4 * (c + sub));
            m = max(m, max(max(bc_abs_bits(v.x), bc_abs_bits(v.y)), max(bc_abs_bits(v.z), bc_abs_bits(v.w))));
        }
    }
#pragma unroll
    for (int off = LPR / 2; off >= 1; off >>= 1) m = max(m, __shfl_xor(m, off));
    if (row < rows && sub == 0) emap[row] = m;
}

template <int C, int LPR>
static int bc_expmap(const float *x, long long rows, int *emap, hipStream_t st) {
    k_split_expmap<C, LPR><<<divup(rows, 4 * (MSSVT_WAVE / LPR)), 256, 0, st>>>(x, rows, emap);
    return mssvt_launch_status();
}

// ---- the convolution ---------------------------------------------------------------------------------------------------
template <int CIN, int NS>
struct bc_geom {
    static constexpr int KC = BC_KC(CIN), KS = KC / 32, NT = NS / 16, CHUNKS = CIN / KC;
    static constexpr int IMG = KS * NT * 64;  // 16-byte fragments per (hi or lo) image of a block
    static constexpr size_t LDS = 2 * (size_t)2 * IMG * 16;  // two buffers of a hi and a lo image
};

enum { BC_ROWS, BC_ROWS_WORDS, BC_PLANAR, BC_ROWS_INTO, BC_UP2, BC_DOWN2, BC_BRANCH, BC_MULTI };
#define BC_MAX_BRANCHES 64
// the extra (last) argument of the kernel: nothing, but for BC_MULTI the base pointers of its input tensors, by value
struct bc_ptrs {
    const float *p[BC_MAX_BRANCHES];
};
struct bc_none {};
template <int OUT>
struct bc_extra {
    typedef bc_none type;
};
template <>
struct bc_extra<BC_MULTI> {
    typedef bc_ptrs type;
};
// OUT: y (M, nsl NS) rows; rows and eout [pixel][nsl], the largest |y| of the pixel's slice as bits; slice sl's k <= 16 maps
// planar at float kbase B H W; rows of `ystride` floats of which the layer owns channels [ybase, ybase + nsl NS) (a slice of a
// wider tensor; ystride % 4 == ybase % 4 == 0 keeps the stores aligned); UP2: the four phases of a 2 x 2 stride-2 transposed
// convolution as ONE 1 x 1 launch over the INPUT pixels with nsl = 4 Cout / NS slices -- slice sl = (phase ph = dy 2 + dx,
// column slice cs) of blob columns ph Cout + n, stored to pixel (b, 2 iy + dy, 2 ix + dx) of a (B, 2 H, 2 W, ystride) tensor at
// channel ybase + cs NS.  The UP2 grid is one-dimensional: block id = ((pixel block / 8) nsl + sl) 8 + pixel block % 8, so the
// nsl slices that read one input tile follow each other at a distance of 8 ids (consecutive ids go round the chiplets: the
// slices of a tile share one L2); pixel blocks are padded to a multiple of 8 and a padding block leaves at once.
// DOWN2: the input gradient of a 3 x 3 stride-2 convolution (zero padding 1) as its four parity phases in ONE launch, grid
// (pixel blocks of the largest phase, nsl, 4).  x = dY on the H x W grid (CIN = the layer's output channels), y = dX on the
// Ho_ x Wo_ grid of the layer's INPUT (H = (Ho_ + 1) / 2), M = B H W.  blockIdx.z = 3 - (2 py + px): phase (py, px) is the
// (1 + py) x (1 + px) convolution at stride 1 without padding over dY whose output pixel (j, i) is row (b, 2 j + py, 2 i + px)
// of dX -- tap (ty, tx) reads dY (j + ty, i + tx), zeros beyond the grid (the ky = 0 tap of the last row of an even Ho_).  The
// phase grid is Ho_ / 2 (py = 1) or H (py = 0) rows by Wo_ / 2 or W columns: an empty phase (Ho_ = 1 or Wo_ = 1) and the blocks
// beyond a smaller phase leave at once; the 4-tap phase is dealt first.  The blob holds the layer's 9 taps in phase order
// (k_split_pack, transposed = 3) under one header record; ksize_, stride_ and dil_ are not read.
// BRANCH: rows as BC_ROWS, but slice-major: y is [nsl][M][NS], every slice a dense (M, NS) matrix.
// MULTI: y (M, NS) rows = the SUM over `gin` input tensors (the argument counts them in this form; SLICED is false) of their
// convolutions, as ONE convolution of gin CIN input channels: the stage loop runs over (tap, tensor) -- the "chunk" of a stage
// is the tensor, its rows come from that tensor's own base pointer (the kernel's last argument; x is not read), CIN <= 128 is
// one chunk.  emap is [tensor][pixel]; an output pixel's power of two is the largest over its receptive field AND all tensors
// (one accumulation chain per element).  The blob holds one block per (tap, tensor) under one header record.

// TAPS 0: ksize x ksize taps (3: padding = dil, 1: none) at `stride` / `dil`, output Ho x Wo;  TAPS 3: 3 x 3, stride 1,
// dilation 1, Ho = H, Wo = W as constants (those five arguments are not read).
// SLICED false: pixels of CIN floats, one exponent word per pixel, every slice under header record 0;  true: pixels of
// `xstride` floats of which slice sl reads channels [sl gin, sl gin + CIN), emap [pixel][egroups] of which it reads word sl
// when egroups > 1 (else word 0), and header record sl.
template <int CIN, int NS, int OUT>
__device__ __forceinline__ int bc_chunks(int, bc_none) { return bc_geom<CIN, NS>::CHUNKS; }
template <int CIN, int NS, int OUT>
__device__ __forceinline__ int bc_chunks(int gin, const bc_ptrs &) { return gin; }
// the rows of chunk `chunk`: x itself, or the chunk's own tensor
__device__ __forceinline__ const float *bc_rows(const float *x, int, bc_none) { return x; }
__device__ __forceinline__ const float *bc_rows(const float *, int chunk, const bc_ptrs &in) { return in.p[chunk]; }

template <int CIN, int NS, int TAPS, bool SLICED, int OUT>
__global__ void __launch_bounds__(BC_THREADS, 1)
    k_split_conv(const float *x, int xstride_, int gin, int H, int W, int Ho_, int Wo_, int M_, const unsigned char *blob, int nsl,
                 int ksize_, int stride_, int dil_, const int *emap, int egroups_, int relu, float *y, int *eout, int ystride,
                 int ybase, typename bc_extra<OUT>::type inputs) {
    using G = bc_geom<CIN, NS>;
    constexpr int KC = G::KC, KS = G::KS, NT = G::NT, IMG = G::IMG;
    constexpr bool MULTI = OUT == BC_MULTI;
    static_assert(!MULTI || (G::CHUNKS == 1 && !SLICED), "BC_MULTI: one chunk per input tensor");
    const int CHUNKS = bc_chunks<CIN, NS, OUT>(gin, inputs);  // (a constant in every form but MULTI)
    constexpr int FR = (2 * IMG + BC_THREADS - 1) / BC_THREADS;  // fragments of a block per thread ...
    constexpr int FP = (FR + KS - 1) / KS;  // ... of which a thread moves at most FP under each k step of the previous block
    extern __shared__ float4 bc_lds[];
    h16x8 *lds = reinterpret_cast<h16x8 *>(bc_lds);  // two buffers of 2 IMG fragments
    const int lane = lane_id(), la = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / MSSVT_WAVE);
    constexpr bool DN = OUT == BC_DOWN2;
    const int py = DN ? (3 - (int)blockIdx.z) >> 1 : 0, px = DN ? (3 - (int)blockIdx.z) & 1 : 0;  // DOWN2: the phase
    const int ksize = DN ? 1 : TAPS ? TAPS : ksize_, stride = (DN || TAPS) ? 1 : stride_, dil = (DN || TAPS) ? 1 : dil_;
    const int ksy = DN ? 1 + py : ksize, ksx = DN ? 1 + px : ksize;  // taps in y and in x
    const int Ho = DN ? (py ? Ho_ / 2 : H) : TAPS ? H : Ho_, Wo = DN ? (px ? Wo_ / 2 : W) : TAPS ? W : Wo_, HWo = Ho * Wo;
    const int M = DN ? (M_ / (H * W)) * HWo : M_;  // DOWN2: the phase's pixels
    const int nstages = ksy * ksx * CHUNKS, pad = ksize == 3 ? dil : 0;
    const int pb = OUT == BC_UP2 ? (int)(blockIdx.x / (8 * nsl)) * 8 + (int)(blockIdx.x % 8) : (int)blockIdx.x;  // pixel block
    const int sl = OUT == BC_UP2 ? (int)(blockIdx.x / 8) % nsl : (int)blockIdx.y;
    if ((OUT == BC_UP2 || DN) && pb * BC_BLOCK_PIXELS >= M) return;  // (the whole workgroup, before any barrier)
    const int cout = nsl * NS, hdr = SLICED ? BC_HDR(nsl) : BC_HDR(1);
    const int xstride = SLICED ? xstride_ : CIN, cbase = SLICED ? sl * gin : 0;
    const int egroups = SLICED ? egroups_ : 1, eoff = egroups > 1 ? sl : 0;
    const float *rec = reinterpret_cast<const float *>(blob + (SLICED ? (size_t)sl * BC_REC_BYTES : 0));
    const float w_un = rec[1];
    const float *scale = reinterpret_cast<const float *>(blob + hdr) + sl * NS, *shift = scale + cout;
    // DOWN2: a slice holds all 9 taps, the phase's own start at tap 0 (2 x 2), 4 (2 x 1), 6 (1 x 2), 8 (1 x 1)
    const int tap0 = DN ? (py ? (px ? 0 : 4) : (px ? 6 : 8)) : 0, slice_stages = DN ? 9 * CHUNKS : nstages;
    const h16x8 *wsrc = reinterpret_cast<const h16x8 *>(blob + hdr + (size_t)cout * 8) +
                        ((size_t)sl * slice_stages + tap0 * CHUNKS) * 2 * IMG;
    // block 0 of the weights -> LDS buffer 0
#pragma unroll
    for (int i = 0; i < FR; ++i) {
        const int f = threadIdx.x + i * BC_THREADS;
        if (f < 2 * IMG) lds[f] = wsrc[f];
    }
    // the wave's two 16-pixel tiles: lane (la, g) reads channels 8 g .. of pixel la of each tile
    int oy0[2], ox0[2];
    int img[2];  // first pixel of the tile's sample (B H W < 2^31)
    bool live[2];
    float s_in[2], un[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = pb * BC_BLOCK_PIXELS + wv * BC_WAVE_PIXELS + 16 * j + la;
        live[j] = m < M;
        const int mc = live[j] ? m : 0, b = mc / HWo, r = mc - b * HWo, oy = r / Wo;
        oy0[j] = oy * stride - pad;
        ox0[j] = (r - oy * Wo) * stride - pad;
        img[j] = b * (H * W);
        // the pixel's power of two: the largest exponent over its receptive field (all taps inside the image)
        int e = 0;
        if (live[j])
            for (int ky = 0; ky < ksy; ++ky)
                for (int kx = 0; kx < ksx; ++kx) {
                    const int iy = oy0[j] + ky * dil, ix = ox0[j] + kx * dil;
                    if (!(iy >= 0 && iy < H && ix >= 0 && ix < W)) continue;
                    if (MULTI) {
                        for (int c = 0; c < CHUNKS; ++c) e = max(e, emap[(size_t)c * M_ + img[j] + iy * W + ix]);
                    } else {
                        e = max(e, emap[(size_t)(img[j] + iy * W + ix) * egroups + eoff]);
                    }
                }
        float s_un;
        pow2_norm(__builtin_bit_cast(float, e), s_in[j], s_un);  // (the word's exponent alone counts: a NaN passes through)
        un[j] = s_un * w_un;
    }
    f32x4 mm[2][NT], cr[2][NT];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t) mm[j][t] = cr[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // the operand rows of k step (stage, P): 8 floats per tile, zeros where the tap falls outside the image
    float4 xa[2][2];
    auto load_rows = [&](int st, int P) {
        const int tap = st / CHUNKS, chunk = st - tap * CHUNKS;
        const int ky = (tap >= ksx) + (tap >= 2 * ksx), kx = tap - ky * ksx;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int iy = oy0[j] + ky * dil, ix = ox0[j] + kx * dil;
            xa[j][0] = xa[j][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live[j] && iy >= 0 && iy < H && ix >= 0 && ix < W) {
                const float *p = bc_rows(x, chunk, inputs) + (size_t)(img[j] + iy * W + ix) * xstride + cbase +
                                 (MULTI ? 0 : chunk * KC) + 32 * P + 8 * g;
                xa[j][0] = *reinterpret_cast<const float4 *>(p);
                xa[j][1] = *reinterpret_cast<const float4 *>(p + 4);
            }
        }
    };
    load_rows(0, 0);
    __syncthreads();
    for (int st = 0; st < nstages; ++st) {
        const bool more = st + 1 < nstages;
        const h16x8 *Bh = lds + (st & 1) * 2 * IMG, *Bl = Bh + IMG;
        h16x8 *dst = lds + ((st + 1) & 1) * 2 * IMG;  // last read during block st - 1: behind the previous barrier
#pragma unroll
        for (int P = 0; P < KS; ++P) {
            h16x8 wreg[FP];
            if (more) {  // a piece of the next block's fragments travels under this k step's products
#pragma unroll
                for (int i = 0; i < FP; ++i) {
                    const int f = threadIdx.x + (P * FP + i) * BC_THREADS;
                    if (P * FP + i < FR && f < 2 * IMG) wreg[i] = wsrc[(size_t)(st + 1) * 2 * IMG + f];
                }
            }
            h16x8 ah[2], al[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) split8_scaled_rne(xa[j][0], xa[j][1], s_in[j], ah[j], al[j]);
            if (P + 1 < KS) load_rows(st, P + 1);
            else if (more) load_rows(st + 1, 0);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const h16x8 bh = Bh[(P * NT + t) * 64 + lane], bl = Bl[(P * NT + t) * 64 + lane];
                // Y^T tile: A = the weights' rows n, B = the tile's pixels m
                MFMA_H(mm[0][t], bh, ah[0]);
                MFMA_H(mm[1][t], bh, ah[1]);
                MFMA_H(cr[0][t], bh, al[0]);
                MFMA_H(cr[1][t], bh, al[1]);
                MFMA_H(cr[0][t], bl, ah[0]);
                MFMA_H(cr[1][t], bl, ah[1]);
            }
            if (more) {
#pragma unroll
                for (int i = 0; i < FP; ++i) {
                    const int f = threadIdx.x + (P * FP + i) * BC_THREADS;
                    if (P * FP + i < FR && f < 2 * IMG) dst[f] = wreg[i];
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // (keeps the fragment reads of later k steps from being hoisted: spills)
        }
        __syncthreads();
    }
    // epilogue: lane (m = la, g) holds y[m][16 t + 4 g + i] of its slice
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (OUT != BC_ROWS_WORDS && !live[j]) continue;  // (with words the whole wave takes part in the exchange below)
        const int m = pb * BC_BLOCK_PIXELS + wv * BC_WAVE_PIXELS + 16 * j + la, mc = live[j] ? m : 0;
        int top = 0;  // the largest |y| of the lane's columns, as bits
        size_t row = 0;  // INTO / UP2 / DOWN2: the first float of the lane's pixel and slice in y
        if (OUT == BC_ROWS_INTO) row = (size_t)mc * ystride + ybase + sl * NS;
        if (DN) {  // pixel (j, i) of the phase's grid is pixel (2 j + py, 2 i + px) of the Ho_ x Wo_ tensor
            const int b = mc / HWo, r = mc - b * HWo, j2 = r / Wo, i2 = r - j2 * Wo;
            row = (((size_t)b * Ho_ + 2 * j2 + py) * Wo_ + 2 * i2 + px) * cout + sl * NS;
        }
        if (OUT == BC_UP2) {  // (Ho = H, Wo = W: the launch is a 1 x 1 layer over the input pixels)
            const int nc = nsl / 4, ph = sl / nc, b = mc / HWo, r = mc - b * HWo, iy = r / Wo, ix = r - iy * Wo;
            row = (((size_t)b * 2 * Ho + 2 * iy + (ph >> 1)) * (2 * Wo) + 2 * ix + (ph & 1)) * ystride + ybase + (sl - ph * nc) * NS;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float4 s4 = *reinterpret_cast<const float4 *>(scale + 16 * t + 4 * g);
            const float4 b4 = *reinterpret_cast<const float4 *>(shift + 16 * t + 4 * g);
            const float sv[4] = {s4.x, s4.y, s4.z, s4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // (x s_in) (w w_in) / (s_in w_in): both normalisations undone by exact powers of two, then scale / shift
                const float r = __builtin_fmaf(cr[j][t][i], SPLIT_INV, mm[j][t][i]) * un[j];
                o[i] = __builtin_fmaf(r, sv[i], bv[i]);
                if (relu) o[i] = o[i] < 0.f ? 0.f : o[i];  // (a NaN stays a NaN: fmaxf would turn it into 0)
                top = max(top, bc_abs_bits(o[i]));
            }
            if (!live[j]) continue;
            if (OUT == BC_PLANAR) {  // the address is formed per pixel: a wave's tile may straddle two samples
                const int kcols = reinterpret_cast<const int *>(rec)[2], kbase = reinterpret_cast<const int *>(rec)[3];
                const int b = mc / HWo, r = mc - b * HWo;
                float *out = y + ((size_t)kbase * (M / HWo) + (size_t)b * kcols) * HWo + r;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (4 * g + i < kcols) out[(size_t)(4 * g + i) * HWo] = o[i];
            } else if (OUT == BC_ROWS_INTO || OUT == BC_UP2 || DN) {
                *reinterpret_cast<float4 *>(y + row + 16 * t + 4 * g) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
                const size_t at = OUT == BC_BRANCH ? ((size_t)sl * M + mc) * NS : (size_t)mc * cout + sl * NS;
                *reinterpret_cast<float4 *>(y + at + 16 * t + 4 * g) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
        if (OUT == BC_ROWS_WORDS) {
            top = max(top, __shfl_xor(top, 16));
            top = max(top, __shfl_xor(top, 32));
            if (live[j] && g == 0) eout[(size_t)mc * nsl + sl] = top;
        }
    }
}

template <int CIN, int NS, int TAPS, bool SLICED, int OUT>
static int bc_launch(const float *x, int xstride, int gin, int H, int W, int Ho, int Wo, int M, const void *packed, int nsl,
                     int ksize, int stride, int dil, const int *emap, int egroups, int relu, float *y, int *eout, int ystride, int ybase,
                     hipStream_t st, typename bc_extra<OUT>::type inputs = {}) {
    const auto kernel = k_split_conv<CIN, NS, TAPS, SLICED, OUT>;
    constexpr size_t LDS = bc_geom<CIN, NS>::LDS;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
    if (e != hipSuccess) return (int)e;
    const int nblocks = divup(M, BC_BLOCK_PIXELS);
    const dim3 grid = OUT == BC_UP2 ? dim3((nblocks + 7) / 8 * 8 * nsl) : dim3(nblocks, nsl, OUT == BC_DOWN2 ? 4 : 1);
    kernel<<<grid, BC_THREADS, LDS, st>>>(x, xstride, gin, H, W, Ho, Wo, M, reinterpret_cast<const unsigned char *>(packed), nsl,
                                          ksize, stride, dil, emap, egroups, relu, y, eout, ystride, ybase, inputs);
    return mssvt_launch_status();
}

// ---- weight packing: the slices [sl, sl + n) of a blob of nsl from one weight tensor of k <= n ns output channels ---------
// (n = nsl, sl = 0 if `whole`, else n = 1).  The kernels are static: both translation units hold a copy.
// one workgroup: the power of two of the tensor's weights and the n ns folded scale / shift columns.  whole: record 0 and
// its zero padding to 64 bytes, [w_in, w_un, 0 ..]; else record sl, [w_in, w_un, k, kbase]
static __global__ void __launch_bounds__(1024) k_split_prep(const float *w, long long count, const float *bias, const float *bn_w,
                                                            const float *bn_b, const float *bn_mean, const float *bn_var,
                                                            float eps, int k, int kbase, int ns, int nsl, int sl, int whole,
                                                            int period, int hdr, unsigned char *blob) {
    __shared__ int part[16];
    int m = 0;
    for (long long i = threadIdx.x; i < count; i += blockDim.x) m = max(m, bc_abs_bits(w[i]));
    for (int off = 32; off; off >>= 1) m = max(m, __shfl_xor(m, off));
    if (lane_id() == 0) part[threadIdx.x / MSSVT_WAVE] = m;
    __syncthreads();
    if (threadIdx.x < (whole ? 16 : 4)) {
        m = 0;
        for (int i = 0; i < 16; ++i) m = max(m, part[i]);
        int eb;
        const bool norm = pow2_norm_exponent(m, eb);
        const int word[4] = {norm ? 0x7F000000 - eb : 0x3F800000, norm ? eb : 0x3F800000, whole ? 0 : k, whole ? 0 : kbase};
        reinterpret_cast<int *>(blob + (size_t)sl * BC_REC_BYTES)[threadIdx.x] = threadIdx.x < 4 ? word[threadIdx.x] : 0;
    }
    const int cols = (whole ? nsl : 1) * ns;
    float *scale = reinterpret_cast<float *>(blob + hdr) + (size_t)sl * ns, *shift = scale + (size_t)nsl * ns;
    for (int c = threadIdx.x; c < cols; c += blockDim.x) {
        // BatchNorm2d in eval mode: y = (v + bias - mean) gamma / sqrt(var + eps) + beta, folded in double, rounded once;
        // a column beyond k (the 16-column tile of a narrower branch) is never stored: scale 1, shift 0.  Column c is output
        // channel c % period (period = k, but k / 4 for the four phases of an up-2 layer)
        const int ch = c % period;
        double s = 1.0, t = (bias && c < k) ? (double)bias[ch] : 0.0;
        if (bn_mean && c < k) {
            s = (bn_w ? (double)bn_w[ch] : 1.0) / sqrt((double)bn_var[ch] + (double)eps);
            t = (t - (double)bn_mean[ch]) * s + (bn_b ? (double)bn_b[ch] : 0.0);
        }
        scale[c] = (float)s;
        shift[c] = (float)t;
    }
}

// one thread per operand fragment: (slice, stage = (tap, chunk), P, t, lane) -> 8 weights of output channel n = slice ns +
// 16 t + lane % 16 of the tensor (zeros beyond k), c = chunk KC + 32 P + 8 (lane / 16) .., split into the hi and the lo image
// of the stage's block.  The tensor is a Conv2d weight (k, cin, ksize, ksize), or a ConvTranspose2d weight: `transposed` 1:
// (cin, k, 1, 1); 2 (ksize = 1): (cin, k / 4, 2, 2), column n = phase (dy 2 + dx) k / 4 + output channel (the UP2 form);
// 3 (ksize = 3): the Conv2d weight (cin, k, 3, 3) of the layer whose INPUT gradient the blob computes (the DOWN2 form) -- the
// channel axes swap and stage tap s is tap (ky, kx) of the tensor in phase order: (2,2) (2,0) (0,2) (0,0) | (2,1) (0,1) |
// (1,2) (1,0) | (1,1), the dY offset (0 or 1) of a tap being its place in its phase's list;
// 4 (ksize = 3): the same tensor for the input gradient of the layer at STRIDE 1 -- the channel axes swap and stage tap t is
// tap 8 - t of the tensor (the taps rotated by 180 degrees).
// A slice holds nstages sstride blocks of which this call writes blocks st sstride + soff (sstride = 1, soff = 0: all of them;
// BC_MULTI: sstride input tensors, this one is soff)
static __global__ void __launch_bounds__(256) k_split_pack(const float *w, int transposed, int ksize, int cin, int k, int ns,
                                                           int nsl, int sl, int n_slices, int hdr, unsigned char *blob, int sstride,
                                                           int soff) {
    const int KC = BC_KC(cin), KS = KC / 32, NT = ns / 16, CHUNKS = cin / KC, IMG = KS * NT * 64;
    const int ntaps = ksize * ksize, nstages = ntaps * CHUNKS;
    const long long total = (long long)n_slices * nstages * IMG, id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int f = (int)(id % IMG), st = (int)((id / IMG) % nstages), slice = (int)(id / ((long long)IMG * nstages));
    const int ln = f & 63, t = (f >> 6) % NT, P = (f >> 6) / NT;
    const int tap = st / CHUNKS, chunk = st - tap * CHUNKS;
    const int n = slice * ns + 16 * t + (ln & 15), c0 = chunk * KC + 32 * P + 8 * (ln >> 4);
    const float w_in = reinterpret_cast<const float *>(blob + (size_t)sl * BC_REC_BYTES)[0];
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        v[i] = n >= k              ? 0.f
               : transposed == 4 ? w[((size_t)(c0 + i) * k + n) * 9 + 8 - tap]
               : transposed == 3 ? w[((size_t)(c0 + i) * k + n) * 9 + (int)((0x435170268ull >> (4 * tap)) & 15)]
               : transposed == 2 ? w[((size_t)(c0 + i) * (k / 4) + n % (k / 4)) * 4 + n / (k / 4)]
               : transposed      ? w[(size_t)(c0 + i) * k + n]
                                 : w[((size_t)n * cin + c0 + i) * ntaps + tap];
    h16x8 h, l;
    split8_scaled_rne(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), w_in, h, l);
    h16x8 *blk = reinterpret_cast<h16x8 *>(blob + hdr + (size_t)nsl * ns * 8) +
                    (((size_t)(sl + slice) * nstages + st) * sstride + soff) * 2 * IMG;
    blk[f] = h;
    blk[IMG + f] = l;
}

static bool bc_bad_bn(const float *bn_w, const float *bn_b, const float *bn_mean, const float *bn_var, float eps) {
    return (!bn_mean != !bn_var) || ((bn_w || bn_b) && !bn_mean) || (bn_mean && !(eps >= 0.f));
}

static int bc_pack(const float *w, int transposed, const float *bias, const float *bn_w, const float *bn_b, const float *bn_mean,
                   const float *bn_var, float eps, int ksize, int cin, int k, int kbase, int ns, int nsl, int sl, int whole,
                   void *packed, hipStream_t st) {
    unsigned char *blob = reinterpret_cast<unsigned char *>(packed);
    // a `whole` blob has ONE record (the kernel reads it with SLICED false: 64 header bytes whatever nsl is)
    const int n_slices = whole ? nsl : 1, hdr = whole ? BC_HDR(1) : BC_HDR(nsl), period = transposed == 2 ? k / 4 : k;
    k_split_prep<<<1, 1024, 0, st>>>(w, (long long)ksize * ksize * cin * k, bias, bn_w, bn_b, bn_mean, bn_var, eps, k, kbase, ns,
                                     nsl, sl, whole, period, hdr, blob);
    int status = mssvt_launch_status();
    if (status != MSSVT_OK) return status;
    k_split_pack<<<divup((long long)n_slices * ksize * ksize * cin * ns / 8, 256), 256, 0, st>>>(w, transposed, ksize, cin, k, ns,
                                                                                                 nsl, sl, n_slices, hdr, blob, 1, 0);
    return mssvt_launch_status();
}
