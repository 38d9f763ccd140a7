// ceiling.hip -- TIMING-ONLY launches (never on the product path; results are not read by anything).
//
// "What can a launch of this shape reach?"  For the two kernels that own most of a frame -- k_ffn_ws (ffn.hip) and
// k_attn_kvh (block_attn.hip) -- these kernels move the SAME bytes from and to the SAME addresses (the real tables,
// work order and metadata of the frame), issue the SAME number of matrix instructions of the same type and the same
// number of vector instructions per unit of work, in workgroups of the same shape and register footprint -- and remove
// every dependency between them: no LDS hand-off, no barrier, no phase that waits for another phase's values; loads are
// consumed by the vector filler of the SAME iteration only through one add.  The measured duration is the ceiling of the
// structure "this instruction and byte mix on this many waves", the number bench.py reports as `roofline.ceiling_us`
// beside the kernel's own time: the gap between the two is what the dependency chain (rows -> LDS -> product -> LDS ->
// product -> rows; tokens -> image -> scores -> softmax -> second product) costs, the gap to the HBM roof is what the mix
// itself costs.  ("Next round" item 1.)
#include "split_f16.hip.h"


// NV independent fused multiply-adds per lane, eight chains (a chain's dependent latency is hidden by the others)
template <int NV>
__device__ __forceinline__ float valu_filler(float seed, float c) {
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = seed + (float)i;
#pragma unroll
    for (int k = 0; k < NV / 8; ++k)
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = __builtin_fmaf(v[i], c, 1.0f);
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

// ---- the FFN tail's mix: per 16-row tile and wave 48 v_mfma_f32_16x16x32_f16 on 128 resident fragment registers,
// ~260 vector instructions (filler sized so that SQ_INSTS_VALU / SQ_INSTS_MFMA of a launch match k_ffn_ws's: tools/pmc_ceiling.sh), per row 512 B in + 3 gathered 512-B rows + 32 B of table + 2 x 512 B out ------------------
__global__ void __launch_bounds__(512, 2) k_ceiling_ffn_ws(int n_rows, const float4 *x_in, const int4 *tab_row, const float4 *tab_w,
                                                           const float4 *attn, const h16x8 *frags, float4 *y, float4 *yn) {
    const int lane = lane_id(), wv = threadIdx.x / MSSVT_WAVE;
    // the stationary fragments of k_ffn_ws: 2 x 16 h16x8 per lane (128 VGPRs), loaded once
    h16x8 w[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) w[i] = frags[((size_t)wv * 32 + i) * 64 + lane];
    const int tiles = (n_rows + 15) >> 4;
    const int r_in_tile = threadIdx.x >> 5, piece = threadIdx.x & 31;  // lane = 4 channels of a row (32 lanes per row)
    f32x4 acc[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float sink = 0.f;
    // the next tile's rows are requested before this tile's work (as every streaming kernel of the library does)
    float4 x_n, tw_n, a0_n, a1_n, a2_n;
#define CEIL_LOAD(t_)                                                                  \
    {                                                                                  \
        const int row_ = min((t_) * 16 + r_in_tile, n_rows - 1);                       \
        x_n = x_in[(size_t)row_ * 32 + piece];                                         \
        const int4 tr_ = tab_row[row_];                                                \
        tw_n = tab_w[row_];                                                            \
        a0_n = attn[(size_t)max(tr_.x, 0) * 32 + piece];                               \
        a1_n = attn[(size_t)max(tr_.y, 0) * 32 + piece];                               \
        a2_n = attn[(size_t)max(tr_.z, 0) * 32 + piece];                               \
    }
    if ((int)blockIdx.x < tiles) CEIL_LOAD(blockIdx.x)
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int row = min(t * 16 + r_in_tile, n_rows - 1);
        const float4 x = x_n, tw = tw_n, a0 = a0_n, a1 = a1_n, a2 = a2_n;
        CEIL_LOAD(min(t + (int)gridDim.x, tiles - 1))
        const h16x8 bfrag = h16x8{(_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1};
#pragma unroll
        for (int k = 0; k < 48; ++k)
            acc[k % 6] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[k % 32], bfrag, acc[k % 6], 0, 0, 0);
        const float in = ((x.x + a0.x * tw.x) + (a1.y * tw.y + a2.z * tw.z)) + (x.w + x.y);
        const float f = valu_filler<144>(in, 0.999f);  // + the loop's own ~115 vector instructions = k_ffn_ws's 262 per wave and tile (PMC)
        sink += f;
        y[(size_t)row * 32 + piece] = make_float4(f, in, x.z, a0.w);
        yn[(size_t)row * 32 + piece] = make_float4(in, f, a1.w, a2.w);
    }
#undef CEIL_LOAD
    float s = sink;
#pragma unroll
    for (int i = 0; i < 6; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 123.456f) y[0] = make_float4(s, s, s, s);  // (keeps the matrix results alive)
}

extern "C" int mssvt_ceiling_ffn_ws(int n_rows, const float *x_in, const int *tab_row, const float *tab_w, const float *attn,
                                    const void *fragments_256k, float *y, float *y_norm, void *stream) {
    if (n_rows <= 0 || !x_in || !tab_row || !tab_w || !attn || !fragments_256k || !y || !y_norm) return MSSVT_E_BADARG;
    k_ceiling_ffn_ws<<<256, 512, 0, (hipStream_t)stream>>>(n_rows, (const float4 *)x_in, (const int4 *)tab_row, (const float4 *)tab_w,
                                                           (const float4 *)attn, (const h16x8 *)fragments_256k, (float4 *)y,
                                                           (float4 *)y_norm);
    return mssvt_launch_status();
}

// ---- round 6: WHICH mix could the FFN tail run on?  The same launch with the mix as template parameters --------------
// MODE 0: no matrix instructions; 1: 48 v_mfma_f32_16x16x32_f16 per wave and 16-row tile (the product kernel's);
// 2: 48 v_mfma_f32_32x32x16_f16 per wave and 32-ROW tile -- the same matrix FLOP per row in half the instructions, each
// of which blocks the SIMD's vector issue for 8 of its 32 cycles instead of 8 of 16 (MI355X_MICROARCH.md, cycle constants);
// a lane then owns 8 channels of a row (two 16-byte pieces 256 B apart: every load instruction still covers whole
// 256-byte half rows), so per-lane overheads (addresses, DPP reductions) are paid once per 8 channels.
// NV: filler vector instructions per wave and tile; the loop's own count comes out of the PMC pass (tools/pmc_ceiling.sh).
typedef float f32x16 __attribute__((ext_vector_type(16)));
template <int MODE, int NV>
__global__ void __launch_bounds__(512, 2) k_ceiling_ffn_mix(int n_rows, const float4 *x_in, const int4 *tab_row, const float4 *tab_w,
                                                            const float4 *attn, const h16x8 *frags, float4 *y, float4 *yn) {
    constexpr int ROWS = MODE == 2 ? 32 : 16, PCS = MODE == 2 ? 2 : 1, LPR = 32 / PCS;
    const int lane = lane_id(), wv = threadIdx.x / MSSVT_WAVE;
    h16x8 w[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) w[i] = frags[((size_t)wv * 32 + i) * 64 + lane];
    const int tiles = (n_rows + ROWS - 1) / ROWS;
    const int r_in_tile = threadIdx.x / LPR, piece = threadIdx.x % LPR;
    f32x4 acc[6];
    f32x16 big[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 16; ++j) big[i][j] = 0.f;
    float sink = 0.f;
    float4 x_n[PCS], tw_n, a0_n[PCS], a1_n[PCS], a2_n[PCS];
#define CEIL_LOAD(t_)                                                                  \
    {                                                                                  \
        const int row_ = min((t_) * ROWS + r_in_tile, n_rows - 1);                     \
        const int4 tr_ = tab_row[row_];                                                \
        tw_n = tab_w[row_];                                                            \
        _Pragma("unroll") for (int c = 0; c < PCS; ++c) {                              \
            x_n[c] = x_in[(size_t)row_ * 32 + piece + 16 * c];                         \
            a0_n[c] = attn[(size_t)max(tr_.x, 0) * 32 + piece + 16 * c];               \
            a1_n[c] = attn[(size_t)max(tr_.y, 0) * 32 + piece + 16 * c];               \
            a2_n[c] = attn[(size_t)max(tr_.z, 0) * 32 + piece + 16 * c];               \
        }                                                                              \
    }
    if ((int)blockIdx.x < tiles) CEIL_LOAD(blockIdx.x)
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int row = min(t * ROWS + r_in_tile, n_rows - 1);
        float4 x[PCS], a0[PCS], a1[PCS], a2[PCS];
        const float4 tw = tw_n;
#pragma unroll
        for (int c = 0; c < PCS; ++c) { x[c] = x_n[c]; a0[c] = a0_n[c]; a1[c] = a1_n[c]; a2[c] = a2_n[c]; }
        CEIL_LOAD(min(t + (int)gridDim.x, tiles - 1))
        const h16x8 bfrag = h16x8{(_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1};
        if (MODE == 1) {
#pragma unroll
            for (int k = 0; k < 48; ++k)
                acc[k % 6] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[k % 32], bfrag, acc[k % 6], 0, 0, 0);
        } else if (MODE == 2) {
#pragma unroll
            for (int k = 0; k < 48; ++k)
                big[k % 2] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w[k % 32], bfrag, big[k % 2], 0, 0, 0);
        }
        float in = 0.f;
#pragma unroll
        for (int c = 0; c < PCS; ++c) in += ((x[c].x + a0[c].x * tw.x) + (a1[c].y * tw.y + a2[c].z * tw.z)) + (x[c].w + x[c].y);
        const float f = NV > 0 ? valu_filler<(NV > 0 ? NV : 8)>(in, 0.999f) : in * 0.5f;
        sink += f;
#pragma unroll
        for (int c = 0; c < PCS; ++c) {
            y[(size_t)row * 32 + piece + 16 * c] = make_float4(f, in, x[c].z, a0[c].w);
            yn[(size_t)row * 32 + piece + 16 * c] = make_float4(in, f, a1[c].w, a2[c].w);
        }
    }
#undef CEIL_LOAD
    float s = sink;
#pragma unroll
    for (int i = 0; i < 6; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
#pragma unroll
    for (int i = 0; i < 2; ++i) s += big[i][0] + big[i][5] + big[i][10] + big[i][15];
    if (s == 123.456f) y[0] = make_float4(s, s, s, s);
}

// variant = 100 * MODE + index into {0, 72, 144, 216, 288, 400} filler instructions per wave and tile
extern "C" int mssvt_ceiling_ffn_mix(int variant, int n_rows, const float *x_in, const int *tab_row, const float *tab_w, const float *attn,
                                     const void *fragments_256k, float *y, float *y_norm, void *stream) {
    if (n_rows <= 0 || !x_in || !tab_row || !tab_w || !attn || !fragments_256k || !y || !y_norm) return MSSVT_E_BADARG;
#define MIX_GO(M_, I_, NV_)                                                                                                  \
    if (variant == 100 * M_ + I_) {                                                                                          \
        k_ceiling_ffn_mix<M_, NV_><<<256, 512, 0, (hipStream_t)stream>>>(n_rows, (const float4 *)x_in, (const int4 *)tab_row, \
            (const float4 *)tab_w, (const float4 *)attn, (const h16x8 *)fragments_256k, (float4 *)y, (float4 *)y_norm);      \
        return mssvt_launch_status();                                                                                        \
    }
#define MIX_MODE(M_) MIX_GO(M_, 0, 0) MIX_GO(M_, 1, 72) MIX_GO(M_, 2, 144) MIX_GO(M_, 3, 216) MIX_GO(M_, 4, 288) MIX_GO(M_, 5, 400)
    MIX_MODE(0) MIX_MODE(1) MIX_MODE(2)
#undef MIX_MODE
#undef MIX_GO
    return MSSVT_E_BADARG;
}

// ---- the window attention's mix (k_attn_kvh<64, 16, 4, 2, true>): one wave per (window, head group) of the real work
// order; per window 32 key rows x 256 B gathered through the real metadata, 8 fp32 + 42 split-fp16 matrix instructions
// and ~190 vector instructions per pass of 4 queries (+ ~210 per window; sized so that the launch's SQ_INSTS_VALU /
// SQ_INSTS_MFMA match k_attn_kvh's over both query patterns: tools/pmc_ceiling.sh), 16 B of Q' in and 4 x 16 B of Xbar out per lane
// and pass ------------------------------------------------------------------------------------------------------------
struct CeilKvh {
    const float *xhat;
    const float4 *kmeta[2];
    const int *perm, *num_act, *q_off, *nq_valid;
    float *qbuf;
    int C, c0[2], K, row_capacity;
};
// VAR 0: the product's mix.  VAR 1 (round 6): "Wv at the end of the window launch" -- per pass 24 more
// split-fp16 matrix instructions (4 heads x 2 k-steps x 3 products: V^T = Wv_h Xbar_h on the pass's 16 (query, head) columns)
// and ~40 more vector instructions (the operand split of Xbar), and the hand-off shrinks from 4 x 16 B per lane (Xbar: 64 floats
// per query and head) to 16 B (V: 16 floats per query and head).  Round 6 also removed what made this ceiling SLOWER than the
// product (114k against 104k cycles): the first pass's Q' was a dependent load inside the pass loop; it now travels with the
// next window's rows, one window ahead, like everything else.
template <int VAR>
__global__ void __launch_bounds__(256, 3) k_ceiling_attn_kvh(CeilKvh a) {
    const int g = blockIdx.y, lane = lane_id(), la = lane & 15, gq = lane >> 4, wv = threadIdx.x / MSSVT_WAVE;
    const int n_act = *a.num_act, wstep = gridDim.x * 4;
    f32x4 acc[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float sink = 0.f;
    const h16x8 one = h16x8{(_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1, (_Float16)1};
    // the next window's key rows, counts and first Q' piece are requested before this window's work
    float4 rows_n[2][4], qp_n;
    int w_n = 0, nqv_n = 0;
    size_t qbase_n = 0;
#define CEIL_QROW(qbase_, q_) (reinterpret_cast<float4 *>(a.qbuf + (size_t)g * a.row_capacity * 256 + ((qbase_) + (q_)) * 256 + (la % 4) * 64) + gq)
#define CEIL_ROWS(wi_)                                                                                   \
    {                                                                                                    \
        w_n = a.perm[min((wi_), n_act - 1)];                                                             \
        _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                                  \
            const float4 km = a.kmeta[g][(size_t)w_n * a.K + min(16 * t + la, a.K - 1)];                 \
            const int r = max(__builtin_bit_cast(int, km.w), 0);                                         \
            const float4 *src = reinterpret_cast<const float4 *>(a.xhat + (size_t)r * a.C + a.c0[g]) + gq; \
            _Pragma("unroll") for (int S = 0; S < 4; ++S) rows_n[t][S] = src[4 * S];                     \
        }                                                                                                \
        const int qo_ = a.q_off[w_n], nv_ = a.nq_valid[w_n];                                             \
        nqv_n = qo_ + nv_ <= a.row_capacity ? nv_ : 0;                                                   \
        qbase_n = (size_t)qo_;                                                                           \
        qp_n = CEIL_QROW(qbase_n, min(la / 4, max(nqv_n - 1, 0)))[0];                                    \
    }
    if ((int)(blockIdx.x * 4 + wv) < n_act) CEIL_ROWS((int)(blockIdx.x * 4 + wv))
    for (int wi = blockIdx.x * 4 + wv; wi < n_act; wi += wstep) {
        const int nqv = nqv_n;
        const size_t qbase = qbase_n;
        float4 rows[2][4], qp = qp_n;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int S = 0; S < 4; ++S) rows[t][S] = rows_n[t][S];
        CEIL_ROWS(wi + wstep)
        float tok = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int S = 0; S < 4; ++S) tok += rows[t][S].x + rows[t][S].w;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k % 6] = __builtin_amdgcn_mfma_f32_16x16x4f32(tok, 1.0f, acc[k % 6], 0, 0, 0);
        sink += valu_filler<176>(tok, 0.999f);
        for (int q0 = 0; q0 < nqv; q0 += 4) {
            const int q = min(q0 + la / 4, nqv - 1);
            float4 *xrow = CEIL_QROW(qbase, q);
            if (q0 > 0) qp = xrow[0];
#pragma unroll
            for (int k = 0; k < (VAR == 1 ? 66 : 42); ++k) acc[k % 6] = __builtin_amdgcn_mfma_f32_16x16x32_f16(one, one, acc[k % 6], 0, 0, 0);
            const float f = valu_filler<(VAR == 1 ? 200 : 160)>(qp.x + qp.w, 0.999f);
            sink += f;
            if (q0 + la / 4 < nqv) {
#pragma unroll
                for (int u = 0; u < (VAR == 1 ? 1 : 4); ++u) xrow[4 * u] = make_float4(f, qp.y, qp.z, qp.x);
            }
        }
    }
#undef CEIL_ROWS
#undef CEIL_QROW
    float s = sink;
#pragma unroll
    for (int i = 0; i < 6; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    if (s == 123.456f) a.qbuf[0] = s;
}

static int ceiling_attn_kvh_launch(int variant, int C, int c0_group0, int c0_group1, int K, const float *xhat, const float *kmeta0,
                                   const float *kmeta1, const int *perm, const int *num_active_dev, const int *q_off,
                                   const int *nq_valid, int row_capacity, int win_capacity, float *qbuf, void *stream) {
    if (C <= 0 || K <= 0 || !xhat || !kmeta0 || !kmeta1 || !perm || !num_active_dev || !q_off || !nq_valid || !qbuf || win_capacity <= 0)
        return MSSVT_E_BADARG;
    CeilKvh a;
    a.xhat = xhat; a.kmeta[0] = (const float4 *)kmeta0; a.kmeta[1] = (const float4 *)kmeta1;
    a.perm = perm; a.num_act = num_active_dev; a.q_off = q_off; a.nq_valid = nq_valid; a.qbuf = qbuf;
    a.C = C; a.c0[0] = c0_group0; a.c0[1] = c0_group1; a.K = K; a.row_capacity = row_capacity;
    const int grid = min(divup(win_capacity, 4), 512);  // the product launch: (256 CUs x 4 workgroups / 2 groups, 2) at 3 waves per SIMD
    if (variant == 1) k_ceiling_attn_kvh<1><<<dim3(grid, 2), 256, 0, (hipStream_t)stream>>>(a);
    else k_ceiling_attn_kvh<0><<<dim3(grid, 2), 256, 0, (hipStream_t)stream>>>(a);
    return mssvt_launch_status();
}

extern "C" int mssvt_ceiling_attn_kvh(int C, int c0_group0, int c0_group1, int K, const float *xhat, const float *kmeta0,
                                      const float *kmeta1, const int *perm, const int *num_active_dev, const int *q_off,
                                      const int *nq_valid, int row_capacity, int win_capacity, float *qbuf, void *stream) {
    return ceiling_attn_kvh_launch(0, C, c0_group0, c0_group1, K, xhat, kmeta0, kmeta1, perm, num_active_dev, q_off, nq_valid,
                                   row_capacity, win_capacity, qbuf, stream);
}

// variant 1: the mix of "Wv applied at the end of the window launch" (24 more matrix instructions, ~40 more vector instructions
// per pass, a quarter of the hand-off bytes) -- the timing-only answer to "would that fusion pay?"
extern "C" int mssvt_ceiling_attn_kvh_variant(int variant, int C, int c0_group0, int c0_group1, int K, const float *xhat,
                                              const float *kmeta0, const float *kmeta1, const int *perm, const int *num_active_dev,
                                              const int *q_off, const int *nq_valid, int row_capacity, int win_capacity, float *qbuf,
                                              void *stream) {
    return ceiling_attn_kvh_launch(variant, C, c0_group0, c0_group1, K, xhat, kmeta0, kmeta1, perm, num_active_dev, q_off, nq_valid,
                                   row_capacity, win_capacity, qbuf, stream);
}
