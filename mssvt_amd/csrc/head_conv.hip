// head_conv.hip -- CenterHead's eleven 3x3 convolutions in eval mode as three launches on channels-last fp32 tensors with
// split-fp16 matrix operands (ref pcdet/models/dense_heads/center_head.py: shared_conv :76-84, SeparateHead :11-46, forward
// :350-360).  The arithmetic is bev_conv.hip's (bev_conv.hip.h): every fp32 operand as fp16 hi / lo halves rounded to nearest,
// a product sum = hi hi + 2^-11 (hi lo + lo hi) on v_mfma_f32_16x16x32_f16 with fp32 accumulation, one chain per output
// element kept in registers over the nine taps and all input channels, operands normalised by exact powers of two (per output
// pixel over its receptive field, per weight tensor at pack time), scale / shift in fp32 in the epilogue, zeros for taps
// outside the image (never loaded), one writer per output element, no atomics.
//
// One kernel template, k_head_conv<CIN, NS, PLANAR>, serves the three stages; blockIdx.y is a SLICE of NS output columns
// with its own weight block, its own weight power of two and its own scale / shift:
//   shared  3x3 Cin -> S + BN + ReLU:            1 slice, reads all Cin channels, writes (B, H, W, S) and one exponent
//                                                 word per pixel (the largest |y| of the pixel, from the epilogue);
//   trunk   3x3 S -> nb S + BN + ReLU:           nb slices (the first convolution of every branch of every head), all read
//                                                 the same S channels, slice b writes columns [b S, (b + 1) S) of
//                                                 (B, H, W, nb S) and exponent word [pixel][b]: ONE WORD PER PIXEL AND
//                                                 BRANCH, so that a branch whose BatchNorm leaves it many binades below
//                                                 another keeps its own normalisation in the next stage;
//   finals  3x3 S -> k_b + bias, no activation:  nb slices of one 16-column tile, slice b reads only channels
//                                                 [b S, (b + 1) S) of the trunk tensor under its own exponent words and
//                                                 writes its k_b <= 16 maps PLANAR: y[kbase_b B H W + (b' k_b + c) H W + r]
//                                                 for sample b', map c, cell r -- the address is formed per pixel (a wave's
//                                                 tile may straddle two samples).
// A wave owns 32 consecutive pixels (two 16-row operand tiles sharing every weight fragment read), a workgroup 8 waves = 256
// pixels.  The weights of a slice arrive packed as operand fragments per (tap, 128-channel chunk of Cin) block, hi image
// then lo image, and stream through two LDS buffers, one barrier per block, as in k_bev_conv.  (Reading a small slice's nine
// taps into LDS once instead was measured on the finals at 470 x 470: 2 % slower, so there is one form.)
#include "common.hip.h"
#include "bev_conv.hip.h"

#define HC_REC_BYTES 16  // per slice: float w_in (2^-e), float w_un (2^e), int k (columns in use), int kbase (maps before it)
#define HC_HDR(NSL) ((((NSL) * HC_REC_BYTES) + 63) / 64 * 64)
#define HC_MAX_SLICES 64

// ---- one word per row of a (rows, C) matrix: the largest |x| of the row, as bits ---------------------------------------
template <int C>
__global__ void __launch_bounds__(256) k_hc_expmap(const float *x, long long rows, int *emap) {
    constexpr int LPR = C / 4 < 16 ? C / 4 : 16, RPW = MSSVT_WAVE / LPR;  // lanes per row, rows per wave
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

template <int CIN, int NS>
struct hc_geom {
    static constexpr int KC = BC_KC(CIN), KS = KC / 32, NT = NS / 16, CHUNKS = CIN / KC, NSTAGES = 9 * CHUNKS;
    static constexpr int IMG = KS * NT * 64;  // 16-byte fragments per (hi or lo) image of a block
    static constexpr size_t LDS = 2 * (size_t)2 * IMG * 16;  // two buffers of a hi and a lo image
};

// x: pixels of `xstride` floats, slice sl reads channels [sl gin, sl gin + CIN); emap: [pixel][egroups] words, slice sl
// reads word sl of its pixel when egroups > 1, else word 0; y: (M, nsl NS) rows, or planar; eout: [pixel][nsl] or NULL
template <int CIN, int NS, bool PLANAR>
__global__ void __launch_bounds__(BC_THREADS, 1)
    k_head_conv(const float *x, int xstride, int gin, int H, int W, int M, const unsigned char *blob, int nsl, const int *emap,
                int egroups, int relu, float *y, int *eout) {
    using G = hc_geom<CIN, NS>;
    constexpr int KC = G::KC, KS = G::KS, NT = G::NT, CHUNKS = G::CHUNKS, NSTAGES = G::NSTAGES, IMG = G::IMG;
    constexpr int FR = (2 * IMG + BC_THREADS - 1) / BC_THREADS;  // fragments of a block per thread ...
    constexpr int FP = (FR + KS - 1) / KS;  // ... of which a thread moves at most FP under each k step of the previous block
    extern __shared__ float4 hc_lds[];
    bc_h16x8 *lds = reinterpret_cast<bc_h16x8 *>(hc_lds);
    const int lane = lane_id(), la = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / MSSVT_WAVE);
    const int sl = blockIdx.y, HW = H * W;
    const float *rec = reinterpret_cast<const float *>(blob + (size_t)sl * HC_REC_BYTES);
    const float w_un = rec[1];
    const float *scale = reinterpret_cast<const float *>(blob + HC_HDR(nsl)) + sl * NS, *shift = scale + (size_t)nsl * NS;
    const bc_h16x8 *wsrc = reinterpret_cast<const bc_h16x8 *>(blob + HC_HDR(nsl) + (size_t)nsl * NS * 8) +
                           (size_t)sl * NSTAGES * 2 * IMG;
    const int cbase = sl * gin, eoff = egroups > 1 ? sl : 0;
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
        const int m = blockIdx.x * BC_BLOCK_PIXELS + wv * BC_WAVE_PIXELS + 16 * j + la;
        live[j] = m < M;
        const int mc = live[j] ? m : 0, b = mc / HW, r = mc - b * HW, oy = r / W;
        oy0[j] = oy - 1;
        ox0[j] = r - oy * W - 1;
        img[j] = b * HW;
        // the pixel's power of two: the largest exponent over its receptive field (all taps inside the image)
        int e = 0;
        if (live[j])
            for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx) {
                    const int iy = oy0[j] + ky, ix = ox0[j] + kx;
                    if (iy >= 0 && iy < H && ix >= 0 && ix < W) e = max(e, emap[(size_t)(img[j] + iy * W + ix) * egroups + eoff]);
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
    // the operand rows of k step (stage, P): 8 floats per tile, zeros where the tap falls outside the image
    float4 xa[2][2];
    auto load_rows = [&](int st, int P) {
        const int tap = st / CHUNKS, chunk = st - tap * CHUNKS;
        const int ky = (tap >= 3) + (tap >= 6), kx = tap - ky * 3;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int iy = oy0[j] + ky, ix = ox0[j] + kx;
            xa[j][0] = xa[j][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live[j] && iy >= 0 && iy < H && ix >= 0 && ix < W) {
                const float *p = x + (size_t)(img[j] + iy * W + ix) * xstride + cbase + chunk * KC + 32 * P + 8 * g;
                xa[j][0] = *reinterpret_cast<const float4 *>(p);
                xa[j][1] = *reinterpret_cast<const float4 *>(p + 4);
            }
        }
    };
    load_rows(0, 0);
    __syncthreads();
    for (int st = 0; st < NSTAGES; ++st) {
        const bool more = st + 1 < NSTAGES;
        const bc_h16x8 *Bh = lds + (st & 1) * 2 * IMG, *Bl = Bh + IMG;
        bc_h16x8 *dst = lds + ((st + 1) & 1) * 2 * IMG;  // last read during block st - 1: behind the previous barrier
#pragma unroll
        for (int P = 0; P < KS; ++P) {
            bc_h16x8 wreg[FP];
            if (more) {  // a piece of the next block's fragments travels under this k step's products
#pragma unroll
                for (int i = 0; i < FP; ++i) {
                    const int f = threadIdx.x + (P * FP + i) * BC_THREADS;
                    if (P * FP + i < FR && f < 2 * IMG) wreg[i] = wsrc[(size_t)(st + 1) * 2 * IMG + f];
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
                    if (P * FP + i < FR && f < 2 * IMG) dst[f] = wreg[i];
                }
            }
            __builtin_amdgcn_sched_barrier(0);  // (keeps the fragment reads of later k steps from being hoisted: spills)
        }
        __syncthreads();
    }
    // epilogue: lane (m = la, g) holds y[m][16 t + 4 g + i] of its slice
    const int kcols = reinterpret_cast<const int *>(rec)[2], kbase = reinterpret_cast<const int *>(rec)[3];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int m = blockIdx.x * BC_BLOCK_PIXELS + wv * BC_WAVE_PIXELS + 16 * j + la;
        const int mc = live[j] ? m : 0;
        int top = 0;  // the largest |y| of the lane's columns, as bits
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float4 s4 = *reinterpret_cast<const float4 *>(scale + 16 * t + 4 * g);
            const float4 b4 = *reinterpret_cast<const float4 *>(shift + 16 * t + 4 * g);
            const float sv[4] = {s4.x, s4.y, s4.z, s4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // (x s_in) (w w_in) / (s_in w_in): both normalisations undone by exact powers of two, then scale / shift
                const float r = __builtin_fmaf(cr[j][t][i], BC_INV, mm[j][t][i]) * un[j];
                o[i] = __builtin_fmaf(r, sv[i], bv[i]);
                if (relu) o[i] = o[i] < 0.f ? 0.f : o[i];  // (a NaN stays a NaN: fmaxf would turn it into 0)
                top = max(top, bc_abs_bits(o[i]));
            }
            if (!live[j]) continue;
            if (PLANAR) {
                const int b = mc / HW, r = mc - b * HW;
                float *out = y + ((size_t)kbase * (M / HW) + (size_t)b * kcols) * HW + r;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (4 * g + i < kcols) out[(size_t)(4 * g + i) * HW] = o[i];
            } else {
                *reinterpret_cast<float4 *>(y + (size_t)mc * nsl * NS + sl * NS + 16 * t + 4 * g) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
        if (eout) {  // (wave-uniform: the whole wave takes part in the exchange)
            top = max(top, __shfl_xor(top, 16));
            top = max(top, __shfl_xor(top, 32));
            if (live[j] && g == 0) eout[(size_t)mc * nsl + sl] = top;
        }
    }
}

// ---- weight packing: one slice per call ----------------------------------------------------------------------------------
// one workgroup: the slice's record (power of two of its weights, k, kbase) and its NS folded scale / shift columns
__global__ void __launch_bounds__(1024) k_hc_prep(const float *w, long long count, const float *bias, const float *bn_w,
                                                  const float *bn_b, const float *bn_mean, const float *bn_var, float eps, int k,
                                                  int kbase, int ns, int nsl, int sl, unsigned char *blob) {
    __shared__ int part[16];
    int m = 0;
    for (long long i = threadIdx.x; i < count; i += blockDim.x) m = max(m, bc_abs_bits(w[i]));
    for (int off = 32; off; off >>= 1) m = max(m, __shfl_xor(m, off));
    if (lane_id() == 0) part[threadIdx.x / MSSVT_WAVE] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = 0;
        for (int i = 0; i < 16; ++i) m = max(m, part[i]);
        const int eb = m & 0x7F800000;
        const bool norm = eb != 0 && eb < 0x7F000000;
        float *rec = reinterpret_cast<float *>(blob + (size_t)sl * HC_REC_BYTES);
        rec[0] = norm ? __builtin_bit_cast(float, 0x7F000000 - eb) : 1.0f;
        rec[1] = norm ? __builtin_bit_cast(float, eb) : 1.0f;
        reinterpret_cast<int *>(rec)[2] = k;
        reinterpret_cast<int *>(rec)[3] = kbase;
    }
    float *scale = reinterpret_cast<float *>(blob + HC_HDR(nsl)) + (size_t)sl * ns, *shift = scale + (size_t)nsl * ns;
    for (int c = threadIdx.x; c < ns; c += blockDim.x) {
        // BatchNorm2d in eval mode: y = (v + bias - mean) gamma / sqrt(var + eps) + beta, folded in double, rounded once;
        // a column beyond k (the 16-column tile of a narrower branch) is never stored: scale 1, shift 0
        double s = 1.0, t = (bias && c < k) ? (double)bias[c] : 0.0;
        if (bn_mean && c < k) {
            s = (bn_w ? (double)bn_w[c] : 1.0) / sqrt((double)bn_var[c] + (double)eps);
            t = (t - (double)bn_mean[c]) * s + (bn_b ? (double)bn_b[c] : 0.0);
        }
        scale[c] = (float)s;
        shift[c] = (float)t;
    }
}

// one thread per operand fragment of the slice: (stage = (tap, chunk), P, t, lane) -> 8 weights n = 16 t + lane % 16 (zeros
// beyond k), c = chunk KC + 32 P + 8 (lane / 16) .., split into the hi and the lo image of the stage's block
__global__ void __launch_bounds__(256) k_hc_pack(const float *w, int cin, int k, int ns, int nsl, int sl, unsigned char *blob) {
    const int KC = BC_KC(cin), KS = KC / 32, NT = ns / 16, CHUNKS = cin / KC, IMG = KS * NT * 64, nstages = 9 * CHUNKS;
    const int total = nstages * IMG, id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const int f = id % IMG, st = id / IMG;
    const int ln = f & 63, t = (f >> 6) % NT, P = (f >> 6) / NT;
    const int tap = st / CHUNKS, chunk = st - tap * CHUNKS;
    const int n = 16 * t + (ln & 15), c0 = chunk * KC + 32 * P + 8 * (ln >> 4);
    const float w_in = reinterpret_cast<const float *>(blob + (size_t)sl * HC_REC_BYTES)[0];
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = n < k ? w[((size_t)n * cin + c0 + i) * 9 + tap] : 0.f;
    bc_h16x8 h, l;
    bc_split8(make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), w_in, h, l);
    bc_h16x8 *blk = reinterpret_cast<bc_h16x8 *>(blob + HC_HDR(nsl) + (size_t)nsl * ns * 8) + ((size_t)sl * nstages + st) * 2 * IMG;
    blk[f] = h;
    blk[IMG + f] = l;
}

static bool hc_cin(int cin) { return cin == 64 || cin == 256 || cin == 384 || cin == 512; }
static bool hc_s(int s) { return s == 32 || s == 64; }
static bool hc_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

extern "C" int mssvt_head_conv_supported(int cin, int s, int nb, int kmax) {
    return hc_cin(cin) && hc_s(s) && nb >= 1 && nb <= HC_MAX_SLICES && kmax >= 1 && kmax <= 16 ? 1 : 0;
}

static long long hc_bytes(int cin, int ns, int nsl) { return HC_HDR(nsl) + 8ll * nsl * ns + 36ll * cin * nsl * ns; }

extern "C" long long mssvt_head_conv_shared_pack_bytes(int cin, int s) {
    return hc_cin(cin) && hc_s(s) ? hc_bytes(cin, s, 1) : 0;
}
extern "C" long long mssvt_head_conv_trunk_pack_bytes(int s, int nb) {
    return hc_s(s) && nb >= 1 && nb <= HC_MAX_SLICES ? hc_bytes(s, s, nb) : 0;
}
extern "C" long long mssvt_head_conv_finals_pack_bytes(int s, int nb) {
    return hc_s(s) && nb >= 1 && nb <= HC_MAX_SLICES ? hc_bytes(s, 16, nb) : 0;
}

static int hc_pack_slice(const float *w, const float *bias, const float *bn_w, const float *bn_b, const float *bn_mean,
                         const float *bn_var, float eps, int cin, int k, int kbase, int ns, int nsl, int sl, void *packed,
                         hipStream_t st) {
    unsigned char *blob = reinterpret_cast<unsigned char *>(packed);
    k_hc_prep<<<1, 1024, 0, st>>>(w, 9ll * cin * k, bias, bn_w, bn_b, bn_mean, bn_var, eps, k, kbase, ns, nsl, sl, blob);
    int status = mssvt_launch_status();
    if (status != MSSVT_OK) return status;
    k_hc_pack<<<divup(9ll * cin * ns / 8, 256), 256, 0, st>>>(w, cin, k, ns, nsl, sl, blob);
    return mssvt_launch_status();
}

static bool hc_bad_bn(const float *bn_w, const float *bn_b, const float *bn_mean, const float *bn_var, float eps) {
    return (!bn_mean != !bn_var) || ((bn_w || bn_b) && !bn_mean) || (bn_mean && !(eps >= 0.f));
}

extern "C" int mssvt_head_conv_shared_pack(const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                           const float *bn_mean, const float *bn_var, float bn_eps, int cin, int s, void *packed,
                                           void *stream) {
    if (!weight || !packed || cin <= 0 || s <= 0 || hc_bad_bn(bn_weight, bn_bias, bn_mean, bn_var, bn_eps) || hc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_cin(cin) || !hc_s(s)) return MSSVT_E_TOOLARGE;
    return hc_pack_slice(weight, bias, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, cin, s, 0, s, 1, 0, packed, (hipStream_t)stream);
}

extern "C" int mssvt_head_conv_trunk_pack(const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                          const float *bn_mean, const float *bn_var, float bn_eps, int s, int nb, int branch,
                                          void *packed, void *stream) {
    if (!weight || !packed || s <= 0 || nb <= 0 || branch < 0 || branch >= nb ||
        hc_bad_bn(bn_weight, bn_bias, bn_mean, bn_var, bn_eps) || hc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES) return MSSVT_E_TOOLARGE;
    return hc_pack_slice(weight, bias, bn_weight, bn_bias, bn_mean, bn_var, bn_eps, s, s, 0, s, nb, branch, packed, (hipStream_t)stream);
}

extern "C" int mssvt_head_conv_finals_pack(const float *weight, const float *bias, int s, int nb, int branch, int k, int kbase,
                                           void *packed, void *stream) {
    if (!weight || !packed || s <= 0 || nb <= 0 || branch < 0 || branch >= nb || k <= 0 || kbase < 0 || hc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES || k > 16 || kbase > 16 * HC_MAX_SLICES) return MSSVT_E_TOOLARGE;
    return hc_pack_slice(weight, bias, nullptr, nullptr, nullptr, nullptr, 0.f, s, k, kbase, 16, nb, branch, packed, (hipStream_t)stream);
}

static bool hc_too_many_pixels(int B, int H, int W) { return (long long)B * H * W > 0x7FFFFFFFll - 4 * BC_BLOCK_PIXELS; }

static int hc_expmap(const float *x, long long rows, int c, int *emap, hipStream_t st) {
#define HC_EXP(C)                                                                                       \
    if (c == C) {                                                                                       \
        constexpr int RPB = 4 * (MSSVT_WAVE / (C / 4 < 16 ? C / 4 : 16));                               \
        k_hc_expmap<C><<<divup(rows, RPB), 256, 0, st>>>(x, rows, emap);                                \
        return mssvt_launch_status();                                                                   \
    }
    HC_EXP(32) HC_EXP(64) HC_EXP(256) HC_EXP(384) HC_EXP(512)
#undef HC_EXP
    return MSSVT_E_TOOLARGE;
}

// x (rows, c) f32 -> exp_words (rows) int32: the largest |x| of every row as bits (what the stages' exp_out hold)
extern "C" int mssvt_head_conv_expmap(const float *x, long long rows, int c, int *exp_words, void *stream) {
    if (!x || !exp_words || rows <= 0 || c <= 0 || hc_misaligned(x)) return MSSVT_E_BADARG;
    if (!(hc_cin(c) || hc_s(c)) || rows > 0x7FFFFFFFll * 16) return MSSVT_E_TOOLARGE;
    return hc_expmap(x, rows, c, exp_words, (hipStream_t)stream);
}

template <int CIN, int NS, bool PLANAR>
static int hc_launch(const float *x, int xstride, int gin, int B, int H, int W, const void *packed, int nsl, const int *emap,
                     int egroups, int relu, float *y, int *eout, hipStream_t st) {
    using G = hc_geom<CIN, NS>;
    const int M = B * H * W;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_head_conv<CIN, NS, PLANAR>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)G::LDS);
    if (e != hipSuccess) return (int)e;
    k_head_conv<CIN, NS, PLANAR><<<dim3(divup(M, BC_BLOCK_PIXELS), nsl), BC_THREADS, G::LDS, st>>>(
        x, xstride, gin, H, W, M, reinterpret_cast<const unsigned char *>(packed), nsl, emap, egroups, relu, y, eout);
    return mssvt_launch_status();
}

// x (B, H, W, cin) -> y (B, H, W, s) = relu(scale conv + shift); exp_workspace (B H W) int32 written here (the input's
// exponent words); exp_out (B H W) int32: y's exponent words, for the trunk
extern "C" int mssvt_head_conv_shared(const float *x, int B, int H, int W, int cin, int s, const void *packed, int *exp_workspace,
                                      float *y, int *exp_out, void *stream) {
    if (!x || !packed || !exp_workspace || !y || !exp_out || B <= 0 || H <= 0 || W <= 0 || cin <= 0 || s <= 0 ||
        hc_misaligned(x) || hc_misaligned(y) || hc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_cin(cin) || !hc_s(s) || hc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    int status = hc_expmap(x, (long long)B * H * W, cin, exp_workspace, st);
    if (status != MSSVT_OK) return status;
#define HC_GO(CI, S) \
    if (cin == CI && s == S) return hc_launch<CI, S, false>(x, CI, 0, B, H, W, packed, 1, exp_workspace, 1, 1, y, exp_out, st);
    HC_GO(64, 32) HC_GO(64, 64) HC_GO(256, 32) HC_GO(256, 64) HC_GO(384, 32) HC_GO(384, 64) HC_GO(512, 32) HC_GO(512, 64)
#undef HC_GO
    return MSSVT_E_TOOLARGE;
}

// x (B, H, W, s) with its exponent words exp_in (B H W) -> y (B, H, W, nb s), exp_out (B H W, nb): one word per pixel and branch
extern "C" int mssvt_head_conv_trunk(const float *x, int B, int H, int W, int s, int nb, const void *packed, const int *exp_in,
                                     float *y, int *exp_out, void *stream) {
    if (!x || !packed || !exp_in || !y || !exp_out || B <= 0 || H <= 0 || W <= 0 || s <= 0 || nb <= 0 || hc_misaligned(x) ||
        hc_misaligned(y) || hc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES || hc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    if (s == 32) return hc_launch<32, 32, false>(x, 32, 0, B, H, W, packed, nb, exp_in, 1, 1, y, exp_out, st);
    return hc_launch<64, 64, false>(x, 64, 0, B, H, W, packed, nb, exp_in, 1, 1, y, exp_out, st);
}

// x (B, H, W, nb s) with exp_in (B H W, nb) -> y planar: branch b's (B, k_b, H, W) maps start at float kbase_b B H W
extern "C" int mssvt_head_conv_finals(const float *x, int B, int H, int W, int s, int nb, const void *packed, const int *exp_in,
                                      float *y, void *stream) {
    if (!x || !packed || !exp_in || !y || B <= 0 || H <= 0 || W <= 0 || s <= 0 || nb <= 0 || hc_misaligned(x) ||
        hc_misaligned(y) || hc_misaligned(packed))
        return MSSVT_E_BADARG;
    if (!hc_s(s) || nb > HC_MAX_SLICES || hc_too_many_pixels(B, H, W)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    if (s == 32) return hc_launch<32, 16, true>(x, nb * 32, 32, B, H, W, packed, nb, exp_in, nb, 0, y, nullptr, st);
    return hc_launch<64, 16, true>(x, nb * 64, 64, B, H, W, packed, nb, exp_in, nb, 0, y, nullptr, st);
}
