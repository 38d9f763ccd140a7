// bev_conv.hip -- y = act(scale[c] * conv(x, w) + shift[c]) on NHWC fp32 tensors with split-fp16 matrix operands: the dense
// 3x3 / 1x1 convolutions behind the sparse backbone in eval mode (ref: the Conv2d + BatchNorm2d + ReLU triples of
// pcdet/models/backbones_2d/map_to_bev/height_compression.py:20-39 and pcdet/models/backbones_2d/base_bev_backbone.py:30-78).
// The library runs them on the fp32 matrix instruction (1/16 of the 16-bit rate); here every fp32 operand v is carried as
// hi = fp16(v), lo = fp16((v - hi) 2^11), a product sum = hi hi + 2^-11 (hi lo + lo hi) on v_mfma_f32_16x16x32_f16 with fp32
// accumulation: the arithmetic of k_linear_rows_h (csrc/linear_rows_h.hip), with both halves rounded to NEAREST here (each
// operand is then off by at most 2^-23 of itself and the dropped lo lo term is at most 2^-22 of the product).
//
// A convolution over channels-last pixels is one row-GEMM per tap accumulated into one tile: M = output pixels, N = Cout,
// K = taps x Cin.  Nothing per tap is ever written to global memory: the lanes of a wave read the tap's input pixel of THEIR
// output pixel straight from x (32 bytes per lane and k step; a pixel outside the image is produced as zeros, never loaded).
//
//   * a wave owns BC_WAVE_PIXELS = 32 consecutive output pixels (two 16-row operand tiles that share every weight fragment
//     read) and NS <= 128 output channels; all 2 x NS / 16 accumulator tiles (mm: hi hi, cr: the cross terms) stay in
//     registers over every tap and all of Cin -- one accumulation chain per output element;
//   * a workgroup is 8 waves = BC_BLOCK_PIXELS = 256 output pixels; Cout = 256 is two slices (blockIdx.y);
//   * the weights arrive packed (k_bc_pack below): per (slice, tap, 128-channel chunk of Cin) one contiguous block holding the
//     hi and the lo image as ready operand fragments [k step][column tile][lane] x 16 bytes.  A block (<= 64 KiB) is copied
//     into one of two LDS buffers while the previous one is multiplied: one barrier per block;
//   * range: fp16 is narrow, so every OUTPUT pixel's operands are normalised by one exact power of two taken from the largest
//     exponent over its whole receptive field (k_bc_expmap writes one word per input pixel first), and the weight tensor by
//     one power of two for all its elements (at pack time); both are undone in the epilogue, exactly.  Scaling the input by
//     a power of two therefore scales the result bit for bit;
//   * the epilogue applies scale / shift in fp32 (the BatchNorm fold is NOT rounded into the fp16 weights), the activation,
//     and stores 16 bytes per lane; every output element has exactly one writer, no atomics.
#include "common.hip.h"
#include "bev_conv.hip.h"

// ---- per input pixel: the largest |x| over its channels, as bits (one word per pixel) ------------------------------
template <int CIN>
__global__ void __launch_bounds__(256) k_bc_expmap(const float *x, long long pixels, int *emap) {
    constexpr int LPP = CIN / 4, PPW = MSSVT_WAVE / LPP;  // lanes per pixel (a float4 each), pixels per wave
    const int lane = lane_id();
    const long long pix = ((long long)blockIdx.x * 4 + threadIdx.x / MSSVT_WAVE) * PPW + lane / LPP;
    int m = 0;
    if (pix < pixels) {
        const float4 v = *reinterpret_cast<const float4 *>(x + (size_t)pix * CIN + 4 * (lane % LPP));
        m = max(max(bc_abs_bits(v.x), bc_abs_bits(v.y)), max(bc_abs_bits(v.z), bc_abs_bits(v.w)));
    }
#pragma unroll
    for (int off = LPP / 2; off >= 1; off >>= 1) m = max(m, __shfl_xor(m, off));
    if (pix < pixels && lane % LPP == 0) emap[pix] = m;
}

// ---- the convolution ---------------------------------------------------------------------------------------------------
template <int CIN, int NS>
__global__ void __launch_bounds__(BC_THREADS, 1)
    k_bev_conv(const float *x, int H, int W, int Ho, int Wo, int M, const unsigned char *blob, int cout, int ksize, int stride,
               int dil, int relu, const int *emap, float *y) {
    constexpr int KC = BC_KC(CIN), KS = KC / 32, NT = NS / 16, CHUNKS = CIN / KC;
    constexpr int IMG = KS * NT * 64;  // 16-byte fragments per (hi or lo) image of a block
    constexpr int FR = (2 * IMG + BC_THREADS - 1) / BC_THREADS;  // fragments of a block per thread ...
    extern __shared__ float4 bc_lds[];
    bc_h16x8 *lds = reinterpret_cast<bc_h16x8 *>(bc_lds);  // two buffers of 2 IMG fragments
    const int lane = lane_id(), la = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / MSSVT_WAVE);
    const int ntaps = ksize * ksize, nstages = ntaps * CHUNKS, pad = ksize == 3 ? dil : 0;
    const float *hdr = reinterpret_cast<const float *>(blob);
    const float w_un = hdr[1];
    const float *scale = hdr + BC_HDR_BYTES / 4, *shift = scale + cout;
    const bc_h16x8 *wsrc = reinterpret_cast<const bc_h16x8 *>(blob + BC_HDR_BYTES + (size_t)cout * 8) +
                           (size_t)blockIdx.y * nstages * 2 * IMG;
    // block 0 of the weights -> LDS buffer 0
    constexpr int FP = FR / KS;  // ... of which a thread moves FP under each k step of the previous block
    static_assert(FR % KS == 0, "a block's fragments are dealt evenly to the k steps");
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
        const int m = blockIdx.x * BC_BLOCK_PIXELS + wv * BC_WAVE_PIXELS + 16 * j + la;
        live[j] = m < M;
        const int mc = live[j] ? m : 0, b = mc / (Ho * Wo), r = mc - b * (Ho * Wo), oy = r / Wo;
        oy0[j] = oy * stride - pad;
        ox0[j] = (r - oy * Wo) * stride - pad;
        img[j] = b * H * W;
        // the pixel's power of two: the largest exponent over its receptive field (all taps inside the image)
        int e = 0;
        if (live[j])
            for (int ky = 0; ky < ksize; ++ky)
                for (int kx = 0; kx < ksize; ++kx) {
                    const int iy = oy0[j] + ky * dil, ix = ox0[j] + kx * dil;
                    if (iy >= 0 && iy < H && ix >= 0 && ix < W) e = max(e, emap[img[j] + iy * W + ix]);
                }
        const int eb = e & 0x7F800000;
        const bool norm = eb != 0 && eb < 0x7F000000;  // zero / denormal fields and inf / nan fields pass through unscaled
        s_in[j] = norm ? __builtin_bit_cast(float, 0x7F000000 - eb) : 1.0f;
        un[j] = (norm ? __builtin_bit_cast(float, eb) : 1.0f) * w_un;
    }
    bc_f32x4 mm[2][NT], cr[2][NT];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int t = 0; t < NT; ++t) mm[j][t] = cr[j][t] = bc_f32x4{0.f, 0.f, 0.f, 0.f};
    // the operand rows of k step ks = (stage, P): 8 floats per tile, zeros where the tap falls outside the image
    float4 xa[2][2];
    auto load_rows = [&](int st, int P) {
        const int tap = st / CHUNKS, chunk = st - tap * CHUNKS;
        const int ky = (tap >= ksize) + (tap >= 2 * ksize), kx = tap - ky * ksize;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int iy = oy0[j] + ky * dil, ix = ox0[j] + kx * dil;
            xa[j][0] = xa[j][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live[j] && iy >= 0 && iy < H && ix >= 0 && ix < W) {
                const float *p = x + (size_t)(img[j] + iy * W + ix) * CIN + chunk * KC + 32 * P + 8 * g;
                xa[j][0] = *reinterpret_cast<const float4 *>(p);
                xa[j][1] = *reinterpret_cast<const float4 *>(p + 4);
            }
        }
    };
    load_rows(0, 0);
    __syncthreads();
    for (int st = 0; st < nstages; ++st) {
        const bool more = st + 1 < nstages;
        const bc_h16x8 *Bh = lds + (st & 1) * 2 * IMG, *Bl = Bh + IMG;
        bc_h16x8 *dst = lds + ((st + 1) & 1) * 2 * IMG;  // last read during block st - 1: behind the previous barrier
#pragma unroll
        for (int P = 0; P < KS; ++P) {
            bc_h16x8 wreg[FP];
            if (more) {  // a piece of the next block's fragments travels under this k step's products
#pragma unroll
                for (int i = 0; i < FP; ++i) {
                    const int f = threadIdx.x + (P * FP + i) * BC_THREADS;
                    if (f < 2 * IMG) wreg[i] = wsrc[(size_t)(st + 1) * 2 * IMG + f];
                }
            }
            bc_h16x8 ah[2], al[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) bc_split8(xa[j][0], xa[j][1], s_in[j], ah[j], al[j]);
            if (P + 1 < KS) load_rows(st, P + 1);
            else if (more) load_rows(st + 1, 0);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bc_h16x8 bh = Bh[(P * NT + t) * 64 + lane], bl = Bl[(P * NT + t) * 64 + lane];
                // Y^T tile: A = the weights' rows n, B = the tile's pixels m
                BC_MFMA(mm[0][t], bh, ah[0]);
                BC_MFMA(mm[1][t], bh, ah[1]);
                BC_MFMA(cr[0][t], bh, al[0]);
                BC_MFMA(cr[1][t], bh, al[1]);
                BC_MFMA(cr[0][t], bl, ah[0]);
                BC_MFMA(cr[1][t], bl, ah[1]);
            }
            if (more) {
#pragma unroll
                for (int i = 0; i < FP; ++i) {
                    const int f = threadIdx.x + (P * FP + i) * BC_THREADS;
                    if (f < 2 * IMG) dst[f] = wreg[i];
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // (keeps the fragment reads of later k steps from being hoisted: spills)
        }
        __syncthreads();
    }
    // epilogue: lane (m = la, g) holds y[m][16 t + 4 g + i] of its slice
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = blockIdx.x * BC_BLOCK_PIXELS + wv * BC_WAVE_PIXELS + 16 * j + la;
        if (!live[j]) continue;
        float *out = y + (size_t)m * cout + blockIdx.y * NS + 4 * g;
        const float *sc = scale + blockIdx.y * NS + 4 * g, *sh = shift + blockIdx.y * NS + 4 * g;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float4 s4 = *reinterpret_cast<const float4 *>(sc + 16 * t), b4 = *reinterpret_cast<const float4 *>(sh + 16 * t);
            const float sv[4] = {s4.x, s4.y, s4.z, s4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // (x s_in) (w w_in) / (s_in w_in): both normalisations undone by exact powers of two, then scale / shift
                const float r = __builtin_fmaf(cr[j][t][i], BC_INV, mm[j][t][i]) * un[j];
                o[i] = __builtin_fmaf(r, sv[i], bv[i]);
                if (relu) o[i] = o[i] < 0.f ? 0.f : o[i];  // (a NaN stays a NaN: fmaxf would turn it into 0)
            }
            *reinterpret_cast<float4 *>(out + 16 * t) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// ---- weight packing ------------------------------------------------------------------------------------------------------
// element (n, c, tap) of a Conv2d weight (Cout, Cin, k, k), or of a ConvTranspose2d(k = 1, s = 1) weight (Cin, Cout, 1, 1)
__device__ __forceinline__ float bc_weight(const float *w, int transposed, int n, int c, int tap, int cin, int cout, int ntaps) {
    return transposed ? w[(size_t)c * cout + n] : w[((size_t)n * cin + c) * ntaps + tap];
}

// one workgroup: the tensor's power of two (header) and the folded scale / shift
__global__ void __launch_bounds__(1024) k_bc_prep(const float *w, long long count, const float *bias, const float *bn_w,
                                                  const float *bn_b, const float *bn_mean, const float *bn_var, float eps,
                                                  int cout, float *hdr) {
    __shared__ int part[16];
    int m = 0;
    for (long long i = threadIdx.x; i < count; i += blockDim.x) m = max(m, bc_abs_bits(w[i]));
    for (int off = 32; off; off >>= 1) m = max(m, __shfl_xor(m, off));
    if (lane_id() == 0) part[threadIdx.x / MSSVT_WAVE] = m;
    __syncthreads();
    if (threadIdx.x < 16) {
        m = 0;
        for (int i = 0; i < 16; ++i) m = max(m, part[i]);
        const int eb = m & 0x7F800000;
        const bool norm = eb != 0 && eb < 0x7F000000;
        if (threadIdx.x == 0) hdr[0] = norm ? __builtin_bit_cast(float, 0x7F000000 - eb) : 1.0f;
        if (threadIdx.x == 1) hdr[1] = norm ? __builtin_bit_cast(float, eb) : 1.0f;
        if (threadIdx.x >= 2) hdr[threadIdx.x] = 0.f;
    }
    float *scale = hdr + BC_HDR_BYTES / 4, *shift = scale + cout;
    for (int c = threadIdx.x; c < cout; c += blockDim.x) {
        // BatchNorm2d in eval mode: y = (v + bias - mean) gamma / sqrt(var + eps) + beta, folded in double, rounded once
        double s = 1.0, t = bias ? (double)bias[c] : 0.0;
        if (bn_mean) {
            s = (bn_w ? (double)bn_w[c] : 1.0) / sqrt((double)bn_var[c] + (double)eps);
            t = (t - (double)bn_mean[c]) * s + (bn_b ? (double)bn_b[c] : 0.0);
        }
        scale[c] = (float)s;
        shift[c] = (float)t;
    }
}

// one thread per operand fragment: (slice, stage = (tap, chunk), P, t, lane) -> 8 weights n = slice NS + 16 t + lane % 16,
// c = chunk KC + 32 P + 8 (lane / 16) .., split into the hi and the lo image of the stage's block
__global__ void __launch_bounds__(256) k_bc_pack(const float *w, int transposed, int ksize, int cin, int cout, unsigned char *blob) {
    const int KC = BC_KC(cin), NS = BC_NS(cout), KS = KC / 32, NT = NS / 16, CHUNKS = cin / KC, IMG = KS * NT * 64;
    const int ntaps = ksize * ksize, nstages = ntaps * CHUNKS, slices = cout / NS;
    const long long total = (long long)slices * nstages * IMG, id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int f = (int)(id % IMG), st = (int)((id / IMG) % nstages), slice = (int)(id / ((long long)IMG * nstages));
    const int ln = f & 63, t = (f >> 6) % NT, P = (f >> 6) / NT;
    const int tap = st / CHUNKS, chunk = st - tap * CHUNKS;
    const int n = slice * NS + 16 * t + (ln & 15), c0 = chunk * KC + 32 * P + 8 * (ln >> 4);
    const float w_in = reinterpret_cast<const float *>(blob)[0];
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = bc_weight(w, transposed, n, c0 + i, tap, cin, cout, ntaps);
    bc_h16x8 h, l;
    bc_split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), w_in, h, l);
    bc_h16x8 *blk = reinterpret_cast<bc_h16x8 *>(blob + BC_HDR_BYTES + (size_t)cout * 8) + ((size_t)slice * nstages + st) * 2 * IMG;
    blk[f] = h;
    blk[IMG + f] = l;
}

static bool bc_channels(int cin, int cout) {
    return (cin == 128 && cout == 128) || (cin == 128 && cout == 256) || (cin == 256 && cout == 256) ||
           (cin == 32 && cout == 32) || (cin == 32 && cout == 64) || (cin == 64 && cout == 64);
}

extern "C" int mssvt_bev_conv_supported(int ksize, int cin, int cout, int stride, int dilation) {
    if (!bc_channels(cin, cout)) return 0;
    if (ksize == 3) return (stride == 1 || stride == 2) && (dilation == 1 || dilation == 2) ? 1 : 0;
    return ksize == 1 && stride == 1 && dilation == 1 ? 1 : 0;
}

extern "C" long long mssvt_bev_conv_pack_bytes(int ksize, int cin, int cout) {
    if (!mssvt_bev_conv_supported(ksize, cin, cout, 1, 1)) return 0;
    return BC_HDR_BYTES + 8ll * cout + 4ll * ksize * ksize * cin * cout;
}

extern "C" int mssvt_bev_conv_pack(const float *weight, int transposed, const float *bias, const float *bn_weight,
                                   const float *bn_bias, const float *bn_mean, const float *bn_var, float bn_eps, int ksize,
                                   int cin, int cout, void *packed, void *stream) {
    if (!weight || !packed || ksize <= 0 || cin <= 0 || cout <= 0 || (transposed && ksize != 1) || (!bn_mean != !bn_var) ||
        ((bn_weight || bn_bias) && !bn_mean) || (bn_mean && !(bn_eps >= 0.f)) || (reinterpret_cast<uintptr_t>(packed) & 15))
        return MSSVT_E_BADARG;
    if (!mssvt_bev_conv_supported(ksize, cin, cout, 1, 1)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    const long long count = (long long)ksize * ksize * cin * cout;
    k_bc_prep<<<1, 1024, 0, st>>>(weight, count, bias, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, cout,
                                  reinterpret_cast<float *>(packed));
    int status = mssvt_launch_status();
    if (status != MSSVT_OK) return status;
    k_bc_pack<<<divup(count / 8, 256), 256, 0, st>>>(weight, transposed, ksize, cin, cout, reinterpret_cast<unsigned char *>(packed));
    return mssvt_launch_status();
}

template <int CIN, int NS>
static int bc_launch(const float *x, int B, int H, int W, int Ho, int Wo, const void *packed, int cout, int ksize, int stride,
                     int dil, int relu, int *emap, float *y, hipStream_t st) {
    constexpr int KC = BC_KC(CIN);
    const long long pixels = (long long)B * H * W;
    const int M = B * Ho * Wo;
    constexpr int PPB = 4 * (MSSVT_WAVE / (CIN / 4));
    k_bc_expmap<CIN><<<divup(pixels, PPB), 256, 0, st>>>(x, pixels, emap);
    int status = mssvt_launch_status();
    if (status != MSSVT_OK) return status;
    const size_t lds = 2 * (size_t)KC * NS * 4;  // two buffers of a hi and a lo image
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_bev_conv<CIN, NS>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    k_bev_conv<CIN, NS><<<dim3(divup(M, BC_BLOCK_PIXELS), cout / NS), BC_THREADS, lds, st>>>(
        x, H, W, Ho, Wo, M, reinterpret_cast<const unsigned char *>(packed), cout, ksize, stride, dil, relu, emap, y);
    return mssvt_launch_status();
}

// x (B, H, W, cin) f32, packed = mssvt_bev_conv_pack's blob, exp_workspace (B H W) int32 (written here, no need to clear),
// y (B, Ho, Wo, cout) f32 with Ho = (H + 2 p - 2 d (k - 1) / 2 - 1) / stride + 1, p = d for 3 x 3 and 0 for 1 x 1
extern "C" int mssvt_bev_conv(const float *x, int B, int H, int W, int cin, const void *packed, int ksize, int cout, int stride,
                              int dilation, int relu, int *exp_workspace, float *y, void *stream) {
    if (!x || !packed || !exp_workspace || !y || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || cout <= 0 || ksize <= 0 ||
        stride <= 0 || dilation <= 0 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) |
                                          reinterpret_cast<uintptr_t>(packed)) & 15))
        return MSSVT_E_BADARG;
    if (!mssvt_bev_conv_supported(ksize, cin, cout, stride, dilation)) return MSSVT_E_TOOLARGE;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;  // padding = dilation (3 x 3) / 0 (1 x 1)
    if ((long long)B * H * W > 0x7FFFFFFFll - 4 * BC_BLOCK_PIXELS) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
#define BC_GO(CI, NSL)                                                                                                     \
    if (cin == CI && BC_NS(cout) == NSL)                                                                                   \
        return bc_launch<CI, NSL>(x, B, H, W, Ho, Wo, packed, cout, ksize, stride, dilation, relu, exp_workspace, y, st);
    BC_GO(128, 128) BC_GO(256, 128) BC_GO(32, 32) BC_GO(32, 64) BC_GO(64, 64)
#undef BC_GO
    return MSSVT_E_TOOLARGE;
}
