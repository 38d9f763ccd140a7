// split_wgrad.hip.h -- the weight gradient of a 3 x 3, stride-1 convolution (dilation d, zero padding d) on channels-last fp32
// tensors with split-fp16 matrix operands (the arithmetic of csrc/split_f16.hip.h, both halves rounded to NEAREST):
//     dW[o, c, ky, kx] = sum over (b, y, x) of dY[b, y, x, o] X[b, y + (ky - 1) d, x + (kx - 1) d, c]     (outside the image: 0)
// One GEMM per tap whose reduction runs over PIXELS: M = cout, N = cin, K = the B H W output pixels in memory order.
//
//   * the pixels are cut into SLICES of bw_slice_pixels(cin) (a function of the channel shape alone); a workgroup owns one
//     (slice, tap, 128 x 128 tile of (cout, cin)) and keeps its accumulators (mm: hi hi, cr: the cross terms) in registers over
//     the whole slice: one accumulation chain per element, a K step = 32 pixels = one v_mfma_f32_16x16x32_f16 per product;
//   * both operands are channel-contiguous in memory and the instruction wants 8 consecutive k = PIXELS per lane: a K step's
//     32 dY rows and the 32 X rows the tap reads (zeros where the tap leaves the image -- never loaded, and the dY row of such
//     a pixel is not loaded either) are split and staged as four [pixel][channel] fp16 images (dY hi, dY lo, X hi, X lo) in
//     one of two LDS buffers, and every fragment is a pair of ds_read_b64_tr_b16: lane (la, g) receives channel 16 t + la of
//     pixels 4 g .. 4 g + 3 and 16 + 4 g .. 16 + 4 g + 3 -- the same bijection of the 32 pixels onto k for both operands.
//     Rows of 2 C + 32 bytes: the 8 rows a 32-lane half of a transposed read touches start 8 banks apart (conflict-free),
//     every lane address is 8-byte aligned; the kernel has no static LDS, so the dynamic region starts aligned.  One barrier
//     per K step: the next step's rows are loaded ahead of the products and stored behind them into the other buffer;
//   * range: the slice's dY rows are normalised by ONE exact power of two (from the largest exponent over those pixels, all
//     channels: k_split_expmap's words) and the X rows the tap reads by another; both are undone exactly on the partial before
//     it is stored, so scaling X or dY by a power of two scales dW bit for bit;
//   * the partial of (slice, tap) is a slab [cout][cin] of the workspace, every element written by exactly one lane;
//     k_split_wgrad_sum adds the slabs in slice order (fp32, sequential) and writes dW in Conv2d's (cout, cin, 3, 3) layout.
//     No atomics: bit-identical from call to call, whatever the workspace held.
//
// The kernel itself is stated over a PLAIN operand (rows of the tile; read at the reduction pixel m itself) and a TAPPED one
// (columns; read at the pixel a tap map sends m to), each with its own row pitch, on a rectangular grid of C x C tiles:
//   BW_TAPS3   the 3 x 3 layer above: plain = dY (rows o), tapped = X at (y + (ky - 1) d, x + (kx - 1) d), 9 taps;
//   BW_PHASES  the weight gradient of a ConvTranspose2d whose kernel equals its stride s in {1, 2},
//                  dW[c, n, dy, dx] = sum over (b, iy, ix) of X[b, iy, ix, c] dY[b, s iy + dy, s ix + dx, n]:
//              plain = X (rows c, the B H W input pixels are the reduction), tapped = dY (columns n) of the (B, s H, s W) grid
//              at (s iy + dy, s ix + dx), s s taps (the phases; every tapped pixel lies inside).  dW (cin, cout, s, s) is again
//              [row][column][tap]: the same second launch writes it;
//   BW_DOWN    the 3 x 3 layer at stride 2 (dilation 1, zero padding 1) over an input of Ht x Wt pixels,
//                  dW[o, c, ky, kx] = sum over (b, oy, ox) of dY[b, oy, ox, o] X[b, 2 oy + ky - 1, 2 ox + kx - 1, c]:
//              plain = dY (rows o, the B Ho Wo OUTPUT pixels are the reduction, H x W = Ho x Wo), tapped = X (columns c) of the
//              (B, Ht, Wt) grid, 9 taps; a tap that leaves the image loads neither row, as in BW_TAPS3.
#pragma once
#include "split_conv.hip.h"

#define BW_STEP 32  // pixels per K step

typedef __fp16 bw_fp16v4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
// lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3 of the group's 4 x 16 block; lane i receives
// column i of the 4 rows.  EXEC must be all ones (the callers sit outside every divergent branch).
__device__ __forceinline__ h16x4 bw_read_tr16(const char *p) {
    return __builtin_bit_cast(h16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) bw_fp16v4 *)(p)));
}

static bool bw_channels(int cin, int cout) { return cin == cout && (cin == 128 || cin == 256 || cin == 32 || cin == 64); }
// pixels per slice: of the channel shape alone (the tests sit either side of one, two and three slices)
static int bw_slice_pixels(int c) { return c >= 256 ? 2048 : c >= 128 ? 4096 : 256; }
// the same for the transposed deblocks (stride, cin, cout): short slices, the grid at B = 1 has few tiles and phases
static bool bw_deblock_shape(int stride, int cin, int cout) {
    return stride == 1 ? (cin == 128 && cout == 256) || (cin == 32 && cout == 64)
                       : stride == 2 && ((cin == 256 && cout == 256) || (cin == 64 && cout == 32));
}
static int bw_deblock_slice_pixels(int cin) { return cin >= 256 ? 2048 : cin >= 128 ? 1024 : 256; }
// the stride-2 3 x 3 layer (cin, cout): slices of OUTPUT pixels
static bool bw_down_shape(int cin, int cout) { return (cin == 128 && cout == 256) || (cin == 32 && cout == 64); }
static int bw_down_slice_pixels(int cin) { return cin >= 128 ? 2048 : 256; }
static long long bw_round256(long long n) { return (n + 255) / 256 * 256; }

template <int C>
struct bw_geom {
    static constexpr int NT = C / 16, TM = 2, TN = NT < 4 ? NT : 4;  // 16-wide tiles per axis; per wave: TM (cout) x TN (cin)
    static constexpr int WC = NT / TN, WAVES = (NT / TM) * WC, THREADS = WAVES * MSSVT_WAVE;
    static constexpr int RS = 2 * C + 32, IMG = BW_STEP * RS, BUF = 4 * IMG;  // bytes: image row, image, buffer of four
    static constexpr int CH8 = C / 8, ITEMS = BW_STEP * CH8, IT = ITEMS / THREADS;  // 8-channel pieces of a K step per thread
    static constexpr size_t LDS = 2 * (size_t)BUF + 64;  // + the maxima of up to 8 waves
    static_assert(ITEMS % THREADS == 0 && NT % TM == 0 && NT % TN == 0 && RS % 16 == 0 && WAVES <= 8, "tiling");
};

enum { BW_TAPS3, BW_PHASES, BW_DOWN };
// MULTI: the plain operand is one tensor of C floats per pixel for every ROW TILE -- row tile b reads plain.p[b] and the words
// eplain + b M, so the slice's power of two of the plain operand is that tensor's own (rows = tiles x C; plain_op is not read)
template <bool MULTI>
struct bw_extra {
    typedef bc_none type;
};
template <>
struct bw_extra<true> {
    typedef bc_ptrs type;
};
__device__ __forceinline__ const float *bw_plain(const float *plain_op, int co0, int, bc_none) { return plain_op + co0; }
__device__ __forceinline__ const float *bw_plain(const float *, int, int tile, const bc_ptrs &in) { return in.p[tile]; }
// tapped_op: the TAPPED operand, pixels of `cols` floats (the tile's columns); plain_op: the PLAIN operand, M = B H W pixels of
// `rows` floats (the tile's rows); etapped / eplain: their k_split_expmap words; slab [slice][tap][rows][cols].  H, W: the grid
// of the reduction pixels; step: the dilation (BW_TAPS3) or the stride s (BW_PHASES: tapped_op then has s s M pixels); Ht, Wt:
// the grid of the tapped operand (read by BW_DOWN alone: the other maps derive it from H, W and step).
// BW_TAPS3, BW_DOWN: plain = dY, rows = cout, tapped = X, cols = cin;  BW_PHASES: plain = X, rows = cin, tapped = dY, cols = cout.
// grid (slices, (rows / C) (cols / C), taps)
template <int C, int MAP, bool MULTI = false>
__global__ void __launch_bounds__(bw_geom<C>::THREADS)
    k_split_wgrad(const float *tapped_op, const float *plain_op, int H, int W, int M, int cols, int rows, int step, int slice,
                  const int *etapped, const int *eplain_, float *slab, int Ht, int Wt, typename bw_extra<MULTI>::type plains) {
    using G = bw_geom<C>;
    constexpr int TM = G::TM, TN = G::TN, RS = G::RS, IMG = G::IMG, BUF = G::BUF, IT = G::IT, THREADS = G::THREADS;
    extern __shared__ __attribute__((aligned(16))) char bw_lds[];
    const int tid = threadIdx.x, lane = lane_id(), la = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid / MSSVT_WAVE);
    const int s = blockIdx.x, tiles = cols / C, co0 = ((int)blockIdx.y / tiles) * C, ci0 = ((int)blockIdx.y % tiles) * C;
    const int tap = blockIdx.z, ntaps = gridDim.z, kdim = MAP == BW_PHASES ? step : 3, ky = tap / kdim, kx = tap - kdim * ky;
    const int oy = MAP == BW_TAPS3 ? (ky - 1) * step : MAP == BW_DOWN ? ky - 1 : ky;
    const int ox = MAP == BW_TAPS3 ? (kx - 1) * step : MAP == BW_DOWN ? kx - 1 : kx;
    const int HW = H * W;
    const float *plain = bw_plain(plain_op, co0, co0 / C, plains);  // the first float of the tile's rows at pixel 0
    const int ppitch = MULTI ? C : rows;
    const int *eplain = MULTI ? eplain_ + (size_t)(co0 / C) * M : eplain_;
    const int m0 = s * slice, m1 = M - m0 > slice ? m0 + slice : M;  // the slice's pixels [m0, m1): may span two samples
    // the pixel the tap reads for reduction pixel m, or -1 outside the image (a phase never leaves it: s^2 M < 2^31)
    auto tapped = [&](int m) {
        const int b = m / HW, r = m - b * HW, y = r / W;
        if (MAP == BW_PHASES) return ((b * H + y) * step + oy) * (step * W) + (r - y * W) * step + ox;
        if (MAP == BW_DOWN) {  // (B Ht Wt < 2^31: the entry point's check)
            const int ty = 2 * y + oy, tx = 2 * (r - y * W) + ox;
            return (ty >= 0 && ty < Ht && tx >= 0 && tx < Wt) ? (b * Ht + ty) * Wt + tx : -1;
        }
        const int iy = y + oy, ix = r - y * W + ox;
        return (iy >= 0 && iy < H && ix >= 0 && ix < W) ? b * HW + iy * W + ix : -1;
    };
    // ---- the slice's two powers of two
    int edm = 0, exm = 0;
    for (int m = m0 + tid; m < m1; m += THREADS) {
        edm = max(edm, eplain[m]);
        const int q = tapped(m);
        if (q >= 0) exm = max(exm, etapped[q]);
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        edm = max(edm, __shfl_xor(edm, off));
        exm = max(exm, __shfl_xor(exm, off));
    }
    int *red = reinterpret_cast<int *>(bw_lds + 2 * BUF);
    if (lane == 0) {
        red[2 * wv] = edm;
        red[2 * wv + 1] = exm;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < G::WAVES; ++i) {
        edm = max(edm, red[2 * i]);
        exm = max(exm, red[2 * i + 1]);
    }
    float d_in, d_un, x_in, x_un;  // (the word's exponent alone counts: a NaN / inf maximum passes through unscaled)
    pow2_norm(__builtin_bit_cast(float, edm), d_in, d_un);
    pow2_norm(__builtin_bit_cast(float, exm), x_in, x_un);

    // ---- staging: item (pixel px of the step, channels 8 ch .. 8 ch + 7) of both operands
    float4 dv[IT][2], xv[IT][2];
    auto load_rows = [&](int k) {
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int id = tid + i * THREADS, px = id / G::CH8, ch = id - px * G::CH8;
            const int m = m0 + BW_STEP * k + px;
            dv[i][0] = dv[i][1] = xv[i][0] = xv[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            const int q = m < m1 ? tapped(m) : -1;
            if (q >= 0) {
                const float *pd = plain + (size_t)m * ppitch + 8 * ch;
                const float *pX = tapped_op + (size_t)q * cols + ci0 + 8 * ch;
                dv[i][0] = *reinterpret_cast<const float4 *>(pd);
                dv[i][1] = *reinterpret_cast<const float4 *>(pd + 4);
                xv[i][0] = *reinterpret_cast<const float4 *>(pX);
                xv[i][1] = *reinterpret_cast<const float4 *>(pX + 4);
            }
        }
    };
    auto store_rows = [&](int buf) {
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int id = tid + i * THREADS, px = id / G::CH8, ch = id - px * G::CH8;
            char *p = bw_lds + buf * BUF + px * RS + 16 * ch;
            h16x8 h, l;
            split8_scaled_rne(dv[i][0], dv[i][1], d_in, h, l);
            *reinterpret_cast<h16x8 *>(p) = h;
            *reinterpret_cast<h16x8 *>(p + IMG) = l;
            split8_scaled_rne(xv[i][0], xv[i][1], x_in, h, l);
            *reinterpret_cast<h16x8 *>(p + 2 * IMG) = h;
            *reinterpret_cast<h16x8 *>(p + 3 * IMG) = l;
        }
    };
    // ---- the wave's TM x TN tiles
    const int wr = wv / G::WC, wc = wv - wr * G::WC;
    const int lane_off = (4 * g + (la >> 2)) * RS + 8 * (la & 3);
    f32x4 mm[TM][TN], cr[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) mm[i][j] = cr[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // fragment of 16-channel tile t of an image pair (hi at p, lo at p + IMG): k slot (g, j) <-> pixel 16 (j / 4) + 4 g + j % 4
    auto frag = [&](const char *img, int t, h16x8 &h, h16x8 &l) {
        const char *p = img + 32 * t + lane_off;
        h = split_cat(bw_read_tr16(p), bw_read_tr16(p + 16 * RS));
        l = split_cat(bw_read_tr16(p + IMG), bw_read_tr16(p + IMG + 16 * RS));
    };
    const int nsteps = (m1 - m0 + BW_STEP - 1) / BW_STEP;
    load_rows(0);
    store_rows(0);
    __syncthreads();
    for (int k = 0; k < nsteps; ++k) {
        const bool more = k + 1 < nsteps;  // (uniform over the workgroup)
        if (more) load_rows(k + 1);
        const char *buf = bw_lds + (k & 1) * BUF;
        h16x8 ah[TM], al[TM];
#pragma unroll
        for (int i = 0; i < TM; ++i) frag(buf, TM * wr + i, ah[i], al[i]);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            h16x8 bh, bl;
            frag(buf + 2 * IMG, TN * wc + j, bh, bl);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                // dW tile: A = dY's channels o (rows), B = X's channels c (columns)
                MFMA_H(mm[i][j], ah[i], bh);
                MFMA_H(cr[i][j], ah[i], bl);
                MFMA_H(cr[i][j], al[i], bh);
            }
        }
        if (more) store_rows((k + 1) & 1);  // (last read during step k - 1: behind the previous barrier)
        __syncthreads();
    }
    // ---- the partial: lane (la, g) holds [o = 16 to + 4 g + r][c = 16 tc + la].  Both powers of two are undone exactly: as
    // one factor where they lie on opposite sides of 1 (their product is then a normal float), one after the other where
    // they lie on the same side (the intermediate then lies between the sum and the result)
    const bool opposite = (d_un >= 1.f) != (x_un >= 1.f);
    const float un1 = opposite ? d_un * x_un : d_un, un2 = opposite ? 1.f : x_un;
    float *out = slab + ((size_t)s * ntaps + tap) * rows * cols;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = co0 + 16 * (TM * wr + i) + 4 * g + r, c = ci0 + 16 * (TN * wc + j) + la;
                out[(size_t)o * cols + c] = __builtin_fmaf(cr[i][j][r], SPLIT_INV, mm[i][j][r]) * un1 * un2;
            }
}

// dw (rows, cols, taps) = the slabs added in slice order; one thread per element, (tap, o, c) with c fastest in the reads
static __global__ void __launch_bounds__(256) k_split_wgrad_sum(const float *slab, int nslices, int cols, int rows, int ntaps,
                                                                float *dw) {
    const int n = ntaps * cols * rows, id = blockIdx.x * 256 + threadIdx.x;
    if (id >= n) return;
    const int c = id % cols, o = (id / cols) % rows, tap = id / (cols * rows);
    float acc = slab[id];
    for (int s = 1; s < nslices; ++s) acc += slab[(size_t)s * n + id];
    dw[((size_t)o * cols + c) * ntaps + tap] = acc;
}

// (the kernel's arguments; dw is (rows, cols, taps))
template <int C, int MAP, bool MULTI = false>
static int bw_launch(const float *tapped_op, const float *plain_op, int H, int W, int M, int cols, int rows, int step, int ntaps,
                     int slice, const int *etapped, const int *eplain, float *slab, float *dw, hipStream_t st, int Ht = 0,
                     int Wt = 0, typename bw_extra<MULTI>::type plains = {}) {
    using G = bw_geom<C>;
    const auto kernel = k_split_wgrad<C, MAP, MULTI>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS);
    if (e != hipSuccess) return (int)e;
    const int nslices = divup(M, slice);
    kernel<<<dim3(nslices, (rows / C) * (cols / C), ntaps), G::THREADS, G::LDS, st>>>(tapped_op, plain_op, H, W, M, cols, rows, step, slice,
                                                                                   etapped, eplain, slab, Ht, Wt, plains);
    int status = mssvt_launch_status();
    if (status != MSSVT_OK) return status;
    k_split_wgrad_sum<<<divup(ntaps * cols * rows, 256), 256, 0, st>>>(slab, nslices, cols, rows, ntaps, dw);
    return mssvt_launch_status();
}
