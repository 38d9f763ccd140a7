// linear_rows_h.hip -- Y = s * act(X B^T + bias) over compact rows with split-fp16 matrix operands, for the LARGE weight
// matrices of the training path (128 <-> 256: linear1 / linear2 of a Block and their input gradients; 64 <-> 128: to_kvs;
// 128 x 128: pos_proj.2 of the CompressBlock -- SURVEY.md section 8 f3; ref nn.Linear in mssvt_backbone.py:339-343,
// mssvt_utils.py:80-83 and their autograd backward).  The framework's library GEMM runs these shapes at 47 - 85 TFLOP/s
// (fp32 instruction; 24 % of the training step's GPU time in round 4); the inference kernel k_ffn_ws sustains 3 x that on
// the same shapes with the arithmetic used here: split-fp16 operands, both halves rounded toward zero (csrc/split_f16.hip.h).
//
// fp16 has a narrow range and gradients do not respect it, so every ROW of X is normalised by a power of two first
// (s_m = 2^-e(max |X[m][:]|), exact; Y[m][:] depends on X[m][:] only, so the row's results are multiplied by 2^e again --
// also exact): the operand halves always see values in (-2, 2), whatever the scale of the activations or gradients.  The
// weight matrix gets ONE power of two for all its elements the same way (computed while it is staged).
//
// One workgroup of 16 waves per CU: the whole weight matrix sits in LDS as ready B^T fragments (hi and lo images,
// [k step][column tile][lane] x 16 bytes: one conflict-free ds_read_b128 per fragment), staged once and split on the way in
// (`transpose_w`: B[n][k] = W[k][n], the input-gradient form).  A wave streams 16-row tiles: its lanes read the rows as
// 32-byte pieces (lane (m, g) <-> row m, columns 32 P + 8 g ..), split them in registers (the A^T operand of every column
// tile), and produce Y^T[n][m] tile by tile -- the accumulator of the transposed product holds four consecutive n of one
// row, so the epilogue (bias, relu, scales) ends in 16-byte stores.  The next tile's rows are in flight under the
// current tile's products.
#include "split_f16.hip.h"

// waves per workgroup: 16 (4 per SIMD, <= 128 registers each) for K <= 128; 8 for K = 256 (the row's 64 prefetch registers +
// 64 accumulator registers do not fit 128: the 16-wave form spilled 742 registers)
#define LH_WAVES_OF(K) ((K) > 128 ? 8 : 16)

template <int K, int N>
__global__ void __launch_bounds__(LH_WAVES_OF(K) *MSSVT_WAVE, 1) k_linear_rows_h(int M, const float *X, int ldx, const float *W, int transpose_w,
                                                                           const float *bias, int relu, float out_scale, float *Y,
                                                                           int ldy) {
    constexpr int KS = K / 32, NT = N / 16, IMG = KS * NT * 64;  // h16x8 fragments per (hi or lo) image
    constexpr int LH_WAVES = LH_WAVES_OF(K);
    extern __shared__ float4 lds4[];
    h16x8 *Bh = reinterpret_cast<h16x8 *>(lds4), *Bl = Bh + IMG;
    __shared__ float4 bias_l[N / 4];  // (a global load per column tile inside the row loop is a dependent round trip per tile)
    for (int e = threadIdx.x; e < N / 4; e += blockDim.x)
        bias_l[e] = bias ? reinterpret_cast<const float4 *>(bias)[e] : make_float4(0.f, 0.f, 0.f, 0.f);
    // stage + split the weights (split_f16.hip.h): normalised by ONE power of two, undone in the epilogue
    WeightImage<K, N, LH_WAVES, true> wimg;
    const float wmx = wimg.load(W, transpose_w);
    const float w_un = wimg.store(wmx, Bh, Bl);
    const int lane = lane_id(), la = lane & 15, g = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / MSSVT_WAVE);
    __syncthreads();
    const int tiles = (M + 15) / 16, step = gridDim.x * LH_WAVES;
    int tile = blockIdx.x * LH_WAVES + wv;
    float4 xn[KS][2];
    if (tile < tiles) {
        const float *row = X + (size_t)min(tile * 16 + la, M - 1) * ldx + 8 * g;
#pragma unroll
        for (int P = 0; P < KS; ++P) {
            xn[P][0] = *reinterpret_cast<const float4 *>(row + 32 * P);
            xn[P][1] = *reinterpret_cast<const float4 *>(row + 32 * P + 4);
        }
    }
    for (; tile < tiles; tile += step) {
        // the row's power-of-two normalisation: s = 2^(127 - E), E = biased exponent of max |x| over the row (all four g lanes)
        float mx = 0.f;
#pragma unroll
        for (int P = 0; P < KS; ++P)
            mx = fmaxf(mx, abs_max8(xn[P][0], xn[P][1]));
        mx = fmaxf(mx, lane_xor16(mx));
        mx = fmaxf(mx, lane_xor32(mx));
        float s_in, s_un;
        pow2_norm(mx, s_in, s_un);
        const float un = s_un * w_un;  // both normalisations undone: exact powers of two
        const int m = tile * 16 + la;
        float *out = Y + (size_t)min(m, M - 1) * ldy + 4 * g;
        // epilogue of column tile t: lane (m = la, g) holds Y[m][16 t + 4 g + i]
        auto finish = [&](int t, const f32x4 &mm, const f32x4 &cr) {
            const float4 b4 = bias_l[4 * t + g];
            float r[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = __builtin_fmaf(cr[i], SPLIT_INV, mm[i]);
            // (x s_in) (W w_in)^T / (s_in w_in): the products come back at their own scale before the bias joins them
            float4 o;
            o.x = r[0] * un + b4.x; o.y = r[1] * un + b4.y; o.z = r[2] * un + b4.z; o.w = r[3] * un + b4.w;
            if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
            o.x *= out_scale; o.y *= out_scale; o.z *= out_scale; o.w *= out_scale;
            if (m < M) *reinterpret_cast<float4 *>(out + 16 * t) = o;
        };
        if constexpr (KS <= 4) {
            // few k steps: the row's fragments stay in registers (8 KS), column tiles one after the other
            h16x8 ah[KS], al[KS];
#pragma unroll
            for (int P = 0; P < KS; ++P) split8_scaled_rtz(xn[P][0], xn[P][1], s_in, ah[P], al[P]);
            if (tile + step < tiles) {
                const float *row = X + (size_t)min((tile + step) * 16 + la, M - 1) * ldx + 8 * g;
#pragma unroll
                for (int P = 0; P < KS; ++P) {
                    xn[P][0] = *reinterpret_cast<const float4 *>(row + 32 * P);
                    xn[P][1] = *reinterpret_cast<const float4 *>(row + 32 * P + 4);
                }
            }
#pragma unroll 2
            for (int t = 0; t < NT; ++t) {
                f32x4 mm = f32x4{0.f, 0.f, 0.f, 0.f}, cr = mm;
#pragma unroll
                for (int P = 0; P < KS; ++P) split_product<NT>(mm, cr, Bh, Bl, P, t, lane, ah[P], al[P]);
                finish(t, mm, cr);
            }
        } else {
            // many k steps, few column tiles (256 -> 128): every column tile's sums stay in registers (8 NT), the row's
            // fragments are split one k step at a time (8 live registers instead of 8 KS)
            static_assert(NT <= 8, "accumulators of all column tiles in registers");
            f32x4 mm[NT], cr[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) mm[t] = cr[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int P = 0; P < KS; ++P) {
                h16x8 ah, al;
                split8_scaled_rtz(xn[P][0], xn[P][1], s_in, ah, al);
#pragma unroll
                for (int t = 0; t < NT; ++t) split_product<NT>(mm[t], cr[t], Bh, Bl, P, t, lane, ah, al);
                __builtin_amdgcn_sched_barrier(0);  // (the scheduler would hoist every fragment read of the unrolled loop: spills)
            }
            if (tile + step < tiles) {
                const float *row = X + (size_t)min((tile + step) * 16 + la, M - 1) * ldx + 8 * g;
#pragma unroll
                for (int P = 0; P < KS; ++P) {
                    xn[P][0] = *reinterpret_cast<const float4 *>(row + 32 * P);
                    xn[P][1] = *reinterpret_cast<const float4 *>(row + 32 * P + 4);
                }
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) finish(t, mm[t], cr[t]);
        }
    }
}

static bool lh_shape(int K, int N) {
    return (K == 128 && N == 256) || (K == 256 && N == 128) || (K == 64 && N == 128) || (K == 128 && N == 64) ||
           (K == 128 && N == 128) || (K == 64 && N == 64);
}

extern "C" int mssvt_linear_rows_h_supported(int K, int N) { return lh_shape(K, N) ? 1 : 0; }

// X (M, ldx >= K) f32, W (N, K) -- or (K, N) with transpose_w -- f32, bias (N) or NULL,
// Y (M, ldy >= N) f32 = out_scale * act(X B^T + bias); ldx, ldy multiples of 4.
extern "C" int mssvt_linear_rows_h(int M, int K, int N, const float *X, int ldx, const float *W, int transpose_w, const float *bias,
                                   int relu, float out_scale, float *Y, int ldy, void *stream) {
    if (M < 0 || !X || !W || !Y || ldx < K || ldy < N || (ldx & 3) || (ldy & 3) || out_scale == 0.f) return MSSVT_E_BADARG;
    if (!lh_shape(K, N)) return MSSVT_E_TOOLARGE;
    if (M == 0) return MSSVT_OK;
    hipStream_t st = (hipStream_t)stream;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus = 256;
    const int grid = min(cus, divup(M, 16 * LH_WAVES_OF(K)));
    const size_t lds = (size_t)K * N * 4;  // two fp16 images
#define LH_GO(KK, NN)                                                                                                    \
    if (K == KK && N == NN) {                                                                                            \
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_linear_rows_h<KK, NN>),                   \
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                    \
        if (e != hipSuccess) return (int)e;                                                                              \
        k_linear_rows_h<KK, NN><<<grid, LH_WAVES_OF(KK) * MSSVT_WAVE, lds, st>>>(M, X, ldx, W, transpose_w, bias, relu, out_scale, Y, ldy); \
        return mssvt_launch_status();                                                                                    \
    }
    LH_GO(128, 256) LH_GO(256, 128) LH_GO(64, 128) LH_GO(128, 64) LH_GO(128, 128) LH_GO(64, 64)
#undef LH_GO
    return MSSVT_E_TOOLARGE;
}
