// block_attn.hip -- fused mixed-scale window attention of one MsSVT Block (fp32).
//
// Replaces, for one head group g of one Block, the reference's
//   7 x K5 feature/coordinate gathers           (ref: mssvt_backbone.py:260-268)
//   relative coordinates + positional MLP        (ref: :269-282, pos_proj :43-47)
//   MixedScaleAttention.forward for group g      (ref: mssvt_utils.py:112-150)
// and, in the table kernel at the end of this file, K9 + K10 + the interpolation weights
// (ref: mssvt_backbone.py:298-311).  Nothing padded is written to HBM.
//
// Arithmetic is re-associated around the small side of the problem (#queries << #keys: ~2 valid
// queries against ~4 + ~20 unmasked keys per window at 160k points): with q' = Wq x_q + b_q,
//   score_h(k)  = scale q'_h . (Wk_h x_k + bk_h) = (scale Wk_h^T q'_h) . x_k + const_h
//   out_h       = sum_k p_hk (Wv_h x_k + bv_h)   = Wv_h (sum_k p_hk x_k) + bv_h
// (const_h cancels in the softmax, sum_k p_hk = 1): keys are never projected; per query 4 mat-vecs
// of size Cg^2, per (query,key) pair 2*heads*Cg MACs.  Masked key slots (additive -100 in the
// reference -> relative weight <= e^-100) are skipped; slot 0 of each scale is never masked, so
// no key set is empty.  Differences to the reference are re-association only (~1e-6 relative).
//
// THREE LAUNCHES:
//   A  k_attn_q  : rows = the compact list of valid queries (mssvt_plan_order), 16 per wavefront:
//                  x_q = xhat row + pos. embedding; Q' = X_q Wq^T + b; Qt_h = scale Q'_h Wk_h -> qbuf
//   B  k_attn_kv : one wavefront per window, lane = channel: key tokens (xhat rows + pos. embedding)
//                  -> LDS; per query scores, softmax, xbar_h = sum_k p_hk x_k -> qbuf (in place of Qt)
//   C  k_attn_o  : rows again: V = Xbar_{head} Wv^T + bv; out = V Wo^T + bo -> attn rows
// A single fused kernel (first version) needs all four Cg x Cg matrices (64 KiB) PLUS the key tile
// (9 KiB per wave) in LDS: 7-8 waves per CU, every LDS / DPP / gather latency exposed (all pipes
// ~25 % busy, 190 us per launch); and a per-query mat-vec re-reads a whole matrix from LDS per query.
// Split, B holds no weights at all (14 waves per CU), and A / C are plain row-tiled GEMMs on the fp32
// matrix cores (v_mfma_f32_16x16x4_f32, exact fp32 products, fp32 accumulation): weights are read
// from LDS once per 16 queries.  The price is one 4*HP*Cg-byte row per query and group written by A,
// rewritten by B, read by C (qbuf, L2/MALL resident).
//
// MFMA mapping of A and C (lane l: r = l % 16 = query row of the tile, g = l / 16): every GEMM is
// computed TRANSPOSED, D^T[out][row] = sum_k W[out][k] X[row][k], A operand = weight rows (one
// ds_read_b128 of the natural row-major matrix feeds 4 k-steps: k-step (S, j) <-> column 16 S + 4 g + j),
// B operand = the activations.  The accumulator layout (lane (r, g), register i = output 4 g + i of
// the 16-tile) then IS the B operand of the next GEMM, step by step, with no shuffle or LDS round
// trip; and it is 4 consecutive channels of one row = one 16-byte global load / store.
// LDS rows are padded to Cg + 4 floats: the 16 lanes of a b128 phase hit 16 x 4 distinct banks.
//
// Windows (B) are processed in the plan's work order (heaviest first), dealt round-robin to the
// wavefronts of a persistent grid.
#include "split_f16.hip.h"

#define ATTN_ROW_WAVES 4  // waves per workgroup of the per-window launch
// waves per workgroup of the row-tiled launches (q, o): ONE workgroup per CU and head group -- the weights are staged
// once per CU (two Cg x Cg matrices, 37 KiB) instead of once per 4-wave workgroup (four of them per CU: 148 KiB at the
// ~11 B/clk a CU fills at = the larger part of a launch on 8k query rows); 66-71 VGPRs leave room for 4 waves / SIMD
#define ATTN_QO_WAVES 16
#define AST_UN 16        // weight elements per matrix and thread in flight while staging (64 x 64 / 256 threads)

struct AttnArgs {
    int C, c0, heads, hd;
    float scale;
    int nq, K;
    const float *xhat;
    const int *num_wins;  // number of entries of `perm` (windows with at least one valid query)
    const int *perm;      // work order: heavy windows first
    const int *q_off;     // (cap) first compact query row of each window
    const int *nq_valid;  // (cap) valid queries of each window
    // compact query rows (mssvt_plan_order): (rel.x, rel.y, rel.z, bits(global feature row));
    // (window, attn row)
    const int *num_rows;
    const float4 *qrow_meta;
    const int2 *qrow_src;
    // per-key-slot metadata resolved by the plan kernel (window_plan.hip): (rel.x, rel.y, rel.z,
    // bits(global feature row or -1)); wcentre = window centre in metres
    const float4 *kmeta, *wcentre;
    const float *Wq, *bq, *Wkv, *bkv, *Wo, *bo, *Wp, *bp;
    float *qbuf;  // (query rows, HP*CG): Qt after A, Xbar after B
    float *attn;
    int row_capacity;  // rows of qbuf / the compact row arrays
    const void *packed;  // split-fp16 weight fragments of this group (mssvt_attn_pack_weights) or null
    // work list of k_attn_kvh: *num_steps steps of step_stride ints.  Stride 1: `perm`, every step one window.  Stride 2:
    // (wA, wB) from mssvt_plan_order_steps, wB = -1 for a single; a pair = two windows of this group whose live keys all
    // sit in slots 0 .. 15 (k_attn_kvh<.., 2, true> only)
    const int *steps, *num_steps;
    int step_stride;
};

// head groups of equal shape run in ONE launch: blockIdx.y = group (their work is independent: channel
// slices of the same rows); a light group fills the gaps of a heavy one and launches / tails halve
#define ATTN_MAX_GROUPS 4
struct AttnPack {
    AttnArgs g[ATTN_MAX_GROUPS];
};

// ---- split-fp16 operands (kv16 form of launch B, see k_attn_kvh): the arithmetic of split_f16.hip.h, packed-multiply form,
// both halves rounded toward zero -------------------------------------------------------------------------------
typedef __fp16 fp16v4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
// kv16 operand order: k slot (g, j) of a 32-wide step P <-> index 32 P + 16 (j / 4) + 4 g + j % 4 -- what a lane holds after
// two DENSE 16-byte row pieces S = 2 P, 2 P + 1 (piece S of lane (., g) = indices 16 S + 4 g .. + 3: the four g lanes of a
// row read 64 contiguous bytes), and equally the accumulator registers of two consecutive 16-row output tiles

// Store of the Q~ / Xbar hand-off rows.  (Measured: written through with `sc1` instead of left dirty for the
// write-back at the kernel boundary, the 67 MB per launch cost the same ~11 us -- k_attn_q 20.6 -> 19.2 us,
// k_attn_kv 46.0 -> 47.2 us: it is the bytes, not when they leave the L2.)
__device__ __forceinline__ void store_handoff(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

#ifdef MSSVT_STAMPS
__device__ unsigned long long g_attn_q_stamps[64 * 8];
extern "C" int mssvt_debug_read_attn_q_stamps(unsigned long long *host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_attn_q_stamps), sizeof(g_attn_q_stamps));
}
#define QSTAMP(k_) if (threadIdx.x == 0 && blockIdx.x < 64 && blockIdx.y == 0) g_attn_q_stamps[blockIdx.x * 8 + (k_)] = __builtin_readcyclecounter();
#else
#define QSTAMP(k_)
#endif
// ---- A: queries -> Qt --------------------------------------------------------------------------
// KV16: Qt rows leave as (hi, lo) fp16 fragments in the operand order of k_attn_kvh (same bytes per row): per head,
// [step P][g][hi x 8 | lo x 8], the 8 = this lane's accumulator registers of output tiles 2 P and 2 P + 1
template <int CG, int HD, int HP, bool KV16>
__global__ void __launch_bounds__(ATTN_QO_WAVES *MSSVT_WAVE) k_attn_q(AttnPack pack) {
    static_assert(!KV16 || CG % 32 == 0, "kv16 operand order: 32-channel steps");
    const AttnArgs &a = pack.g[blockIdx.y];
    constexpr int CGP = (CG + 15) / 16 * 16, NT = CGP / 16, LS = CGP + 4, NH = CG / HD, QROW = HP * CG;
    extern __shared__ float4 lds4[];
    float *Wq_l = reinterpret_cast<float *>(lds4);  // [o][c]   natural nn.Linear layout, padded rows
    float *WkT_l = Wq_l + CGP * LS;                 // [c][o] = Wk[o][c]
    float *Wp_l = WkT_l + CGP * LS;                 // [c][8] = pos_proj row (6 weights, bias, 0)
    float *bq_l = Wp_l + CGP * 8;                   // [o]
    // tile k * grid + block -> wave k % waves: a short row list is spread over all CUs; a workgroup without a tile
    // leaves before it stages anything
    QSTAMP(0)
    const int lane = lane_id(), r = lane & 15, g = lane >> 4;
    const int rows = *a.num_rows, tiles = (rows + 15) >> 4;
    const int wv = threadIdx.x / MSSVT_WAVE;
    if ((int)blockIdx.x >= tiles) return;
    QSTAMP(1)
    // the first tile's row metadata travels while the weights are staged, its feature rows while the workgroup
    // meets at the barrier: metadata -> rows -> products is a chain of round trips as long as the staging itself
    int tile = wv * gridDim.x + blockIdx.x;
    float4 rm = a.qrow_meta[min(tile * 16 + r, rows - 1)];
    int2 src = a.qrow_src[min(tile * 16 + r, rows - 1)];
    // AST_UN elements of each matrix in flight per thread (a plain copy loop waits for every load before
    // its store: one global round trip per element)
    for (int e0 = threadIdx.x; e0 < CGP * CGP; e0 += blockDim.x * AST_UN) {
        float vq[AST_UN], vk[AST_UN];
#pragma unroll
        for (int u = 0; u < AST_UN; ++u) {
            const int e = e0 + u * blockDim.x, o = e / CGP, c = e % CGP;
            const bool in = e < CGP * CGP && o < CG && c < CG;
            vq[u] = in ? a.Wq[o * CG + c] : 0.f;
            vk[u] = in ? a.Wkv[o * CG + c] : 0.f;  // rows [0,CG) of to_kvs = K projection
        }
#pragma unroll
        for (int u = 0; u < AST_UN; ++u) {
            const int e = e0 + u * blockDim.x, o = e / CGP, c = e % CGP;
            if (e < CGP * CGP) {
                Wq_l[o * LS + c] = vq[u];
                WkT_l[c * LS + o] = vk[u];
            }
        }
    }
    for (int e = threadIdx.x; e < CGP * 8; e += blockDim.x) {
        const int c = e >> 3, t = e & 7;
        Wp_l[e] = c < CG ? (t < 6 ? a.Wp[(size_t)(a.c0 + c) * 6 + t] : (t == 6 ? a.bp[a.c0 + c] : 0.f)) : 0.f;
    }
    for (int e = threadIdx.x; e < CGP; e += blockDim.x) bq_l[e] = e < CG ? a.bq[e] : 0.f;
    QSTAMP(2)
    float4 wc = a.wcentre[src.x];
    f32x4 xq[NT];
#define ATTN_Q_ROWS()                                                                                     \
    {                                                                                                     \
        const float *xrow_ = a.xhat + (size_t)__builtin_bit_cast(int, rm.w) * a.C + a.c0;                 \
        _Pragma("unroll") for (int S = 0; S < NT; ++S) {                                                  \
            const int c_ = 16 * S + 4 * g;                                                                \
            const float4 v_ = (CGP == CG || c_ < CG) ? *reinterpret_cast<const float4 *>(xrow_ + c_)      \
                                                     : make_float4(0.f, 0.f, 0.f, 0.f);                   \
            xq[S] = f32x4{v_.x, v_.y, v_.z, v_.w};                                                        \
        }                                                                                                 \
    }
    ATTN_Q_ROWS()
    __syncthreads();
    QSTAMP(3)
    for (bool first = true; tile < tiles; tile += gridDim.x * ATTN_QO_WAVES, first = false) {
        const int row = min(tile * 16 + r, rows - 1);
        if (!first) {
            rm = a.qrow_meta[row];
            src = a.qrow_src[row];
            wc = a.wcentre[src.x];
            // B operand of GEMM1: this lane's 4 channels 16 S + 4 g + j of its query token
            ATTN_Q_ROWS()
        }
#pragma unroll
        for (int S = 0; S < NT; ++S) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float4 p0 = *reinterpret_cast<const float4 *>(Wp_l + (16 * S + 4 * g + j) * 8);
                const float4 p1 = *reinterpret_cast<const float4 *>(Wp_l + (16 * S + 4 * g + j) * 8 + 4);
                const float posc = p1.z + p0.w * wc.x + p1.x * wc.y + p1.y * wc.z;  // window part of the pos. MLP
                xq[S][j] += fmaxf(posc + p0.x * rm.x + p0.y * rm.y + p0.z * rm.z, 0.0f);
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the LDS reads of later steps from being hoisted (VGPRs)
        }
        // GEMM1^T: Q'^T[o][row] = sum_c Wq[o][c] xq[row][c] + bq[o]
        f32x4 qp[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float4 b = *reinterpret_cast<const float4 *>(bq_l + 16 * t + 4 * g);
            qp[t] = f32x4{b.x, b.y, b.z, b.w};
        }
#pragma unroll
        for (int S = 0; S < NT; ++S) {
            float4 w[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) w[t] = *reinterpret_cast<const float4 *>(Wq_l + (16 * t + r) * LS + 16 * S + 4 * g);
#pragma unroll
            for (int t = 0; t < NT; ++t) MFMA4(qp[t], w[t].x, xq[S][0]);
#pragma unroll
            for (int t = 0; t < NT; ++t) MFMA4(qp[t], w[t].y, xq[S][1]);
#pragma unroll
            for (int t = 0; t < NT; ++t) MFMA4(qp[t], w[t].z, xq[S][2]);
#pragma unroll
            for (int t = 0; t < NT; ++t) MFMA4(qp[t], w[t].w, xq[S][3]);
            __builtin_amdgcn_sched_barrier(0);
        }
        // GEMM2^T per head: Qt_h^T[c][row] = scale sum_{o in head h} Wk[o][c] Q'[row][o]
        const bool row_ok = tile * 16 + r < rows;
        float *dst = a.qbuf + (size_t)(tile * 16 + r) * QROW;
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            f32x4 acc[NT];
#pragma unroll
            for (int u = 0; u < NT; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (16 * t >= (h + 1) * HD || 16 * (t + 1) <= h * HD) continue;  // tile outside this head
                // 4 consecutive outputs 16 t + 4 g + i of Q' belong to one head (HD % 4 == 0)
                const bool mine = (HD % 16 == 0) || (16 * t + 4 * g) / HD == h;
                const f32x4 bq4 = mine ? qp[t] : f32x4{0.f, 0.f, 0.f, 0.f};
                float4 w[NT];
#pragma unroll
                for (int u = 0; u < NT; ++u) w[u] = *reinterpret_cast<const float4 *>(WkT_l + (16 * u + r) * LS + 16 * t + 4 * g);
#pragma unroll
                for (int u = 0; u < NT; ++u) MFMA4(acc[u], w[u].x, bq4[0]);
#pragma unroll
                for (int u = 0; u < NT; ++u) MFMA4(acc[u], w[u].y, bq4[1]);
#pragma unroll
                for (int u = 0; u < NT; ++u) MFMA4(acc[u], w[u].z, bq4[2]);
#pragma unroll
                for (int u = 0; u < NT; ++u) MFMA4(acc[u], w[u].w, bq4[3]);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (KV16) {
                h16x8 *dsth = reinterpret_cast<h16x8 *>(dst + h * CG);
#pragma unroll
                for (int P = 0; P < NT / 2; ++P) {
                    h16x8 hi, lo;
                    split8_rtz(acc[2 * P] * a.scale, acc[2 * P + 1] * a.scale, hi, lo);
                    if (row_ok) {
                        dsth[(P * 4 + g) * 2] = hi;
                        dsth[(P * 4 + g) * 2 + 1] = lo;
                    }
                }
                continue;
            }
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const int c = 16 * u + 4 * g;
                if (row_ok && (CGP == CG || c < CG))
                    store_handoff(dst + h * CG + c,
                                  f32x4{acc[u][0] * a.scale, acc[u][1] * a.scale, acc[u][2] * a.scale, acc[u][3] * a.scale});
            }
        }
    }
    QSTAMP(4)
}

// ---- C: Xbar -> attention output rows ----------------------------------------------------------
template <int CG, int HD, int HP>
__global__ void __launch_bounds__(ATTN_QO_WAVES *MSSVT_WAVE) k_attn_o(AttnPack pack) {
    const AttnArgs &a = pack.g[blockIdx.y];
    constexpr int CGP = (CG + 15) / 16 * 16, NT = CGP / 16, LS = CGP + 4, NH = CG / HD, QROW = HP * CG;
    extern __shared__ float4 lds4[];
    float *Wv_l = reinterpret_cast<float *>(lds4);  // [o][c]
    float *Wo_l = Wv_l + CGP * LS;                  // [p][o]
    float *bv_l = Wo_l + CGP * LS, *bo_l = bv_l + CGP;
    const int lane = lane_id(), r = lane & 15, g = lane >> 4;
    const int rows = *a.num_rows, tiles = (rows + 15) >> 4;
    const int wv = threadIdx.x / MSSVT_WAVE;
    if ((int)blockIdx.x >= tiles) return;
    // the first tile's Xbar rows of head 0 travel while the weights are staged
    int tile = wv * gridDim.x + blockIdx.x;
    f32x4 x[NT], xn[NT];
#define ATTN_O_ROWS(dst_, row_, h_)                                                                       \
    {                                                                                                     \
        const float *xb_ = a.qbuf + (size_t)(row_) * QROW + (h_) * CG;                                    \
        _Pragma("unroll") for (int S = 0; S < NT; ++S) {                                                  \
            const int c_ = 16 * S + 4 * g;                                                                \
            const float4 t4_ = (CGP == CG || c_ < CG) ? *reinterpret_cast<const float4 *>(xb_ + c_)       \
                                                      : make_float4(0.f, 0.f, 0.f, 0.f);                  \
            dst_[S] = f32x4{t4_.x, t4_.y, t4_.z, t4_.w};                                                  \
        }                                                                                                 \
    }
    ATTN_O_ROWS(x, min(tile * 16 + r, rows - 1), 0)
    for (int e0 = threadIdx.x; e0 < CGP * CGP; e0 += blockDim.x * AST_UN) {
        float vv[AST_UN], vo[AST_UN];
#pragma unroll
        for (int u = 0; u < AST_UN; ++u) {
            const int e = e0 + u * blockDim.x, o = e / CGP, c = e % CGP;
            const bool in = e < CGP * CGP && o < CG && c < CG;
            vv[u] = in ? a.Wkv[(size_t)(CG + o) * CG + c] : 0.f;  // rows [CG,2CG) of to_kvs = V projection
            vo[u] = in ? a.Wo[o * CG + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < AST_UN; ++u) {
            const int e = e0 + u * blockDim.x, o = e / CGP, c = e % CGP;
            if (e < CGP * CGP) {
                Wv_l[o * LS + c] = vv[u];
                Wo_l[o * LS + c] = vo[u];
            }
        }
    }
    for (int e = threadIdx.x; e < CGP; e += blockDim.x) {
        bv_l[e] = e < CG ? a.bkv[CG + e] : 0.f;
        bo_l[e] = e < CG ? a.bo[e] : 0.f;
    }
    __syncthreads();
    for (bool first = true; tile < tiles; tile += gridDim.x * ATTN_QO_WAVES, first = false) {
        const int row = min(tile * 16 + r, rows - 1);
        const bool row_ok = tile * 16 + r < rows;
        const int dest = a.qrow_src[row].y;
        if (!first) ATTN_O_ROWS(x, row, 0)
        // GEMM3^T: V^T[o][row] = sum_c Wv[o][c] Xbar_{head(o)}[row][c] + bv[o]
        f32x4 v[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float4 b = *reinterpret_cast<const float4 *>(bv_l + 16 * t + 4 * g);
            v[t] = f32x4{b.x, b.y, b.z, b.w};
        }
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            if (h + 1 < NH) ATTN_O_ROWS(xn, row, h + 1)  // the next head's rows under this head's products
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (16 * t >= (h + 1) * HD || 16 * (t + 1) <= h * HD) continue;
                // A rows o = 16 t + r outside head h contribute nothing to this head's pass
                const bool mine = (HD % 16 == 0) || (16 * t + r) / HD == h;
#pragma unroll
                for (int S = 0; S < NT; ++S) {
                    float4 w = *reinterpret_cast<const float4 *>(Wv_l + (16 * t + r) * LS + 16 * S + 4 * g);
                    if (!mine) w = make_float4(0.f, 0.f, 0.f, 0.f);
                    MFMA4(v[t], w.x, x[S][0]);
                    MFMA4(v[t], w.y, x[S][1]);
                    MFMA4(v[t], w.z, x[S][2]);
                    MFMA4(v[t], w.w, x[S][3]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int S = 0; S < NT; ++S) x[S] = xn[S];
        }
        // GEMM4^T: out^T[p][row] = sum_o Wo[p][o] V[row][o] + bo[p]
        f32x4 out[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const float4 b = *reinterpret_cast<const float4 *>(bo_l + 16 * u + 4 * g);
            out[u] = f32x4{b.x, b.y, b.z, b.w};
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float4 w[NT];
#pragma unroll
            for (int u = 0; u < NT; ++u) w[u] = *reinterpret_cast<const float4 *>(Wo_l + (16 * u + r) * LS + 16 * t + 4 * g);
#pragma unroll
            for (int u = 0; u < NT; ++u) MFMA4(out[u], w[u].x, v[t][0]);
#pragma unroll
            for (int u = 0; u < NT; ++u) MFMA4(out[u], w[u].y, v[t][1]);
#pragma unroll
            for (int u = 0; u < NT; ++u) MFMA4(out[u], w[u].z, v[t][2]);
#pragma unroll
            for (int u = 0; u < NT; ++u) MFMA4(out[u], w[u].w, v[t][3]);
            __builtin_amdgcn_sched_barrier(0);
        }
        float *dst = a.attn + (size_t)dest * a.C + a.c0;
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int c = 16 * u + 4 * g;
            if (row_ok && (CGP == CG || c < CG))
                *reinterpret_cast<float4 *>(dst + c) = make_float4(out[u][0], out[u][1], out[u][2], out[u][3]);
        }
    }
}

// ---- A and C with split-fp16 operands (kv16 form) ---------------------------------------------------------------
// The row-tiled launches above are bound by the fp32 matrix instruction too: 128 v_mfma_f32_16x16x4_f32 = 4 096 pipe cycles
// per 16-row tile, four waves per SIMD.  Here the four Cg x Cg matrices are split ONCE per parameter version into (hi, lo)
// fp16 fragments in MFMA operand order (k_attn_pack; the softmax scale folded into Wk), staged by a straight 16-byte copy
// (32 KiB per launch and workgroup instead of 37 KiB of element-wise transposes), and a tile costs 72 (A) / 48 (C)
// sixteen-cycle instructions.  Workgroups are 8 waves so that BOTH head groups of a launch are resident side by side
// (the 16-wave form ran its two groups one after the other: 90 VGPRs allow one such workgroup per CU).
// Fragment blob of one head group (bytes; NT = Cg / 16 output tiles, NP = Cg / 32 steps; HD = 16: head h = tile h):
//   WqF [t][P][hi | lo][lane] x 16 B   A rows o = 16 t + m,        k slot (g, j) <-> channel 32 P + 16 (j / 4) + 4 g + j % 4
//   WkF [h][u][hi | lo][lane] x  8 B   A rows c = (16 * u + m), k slot (g, j) <-> o = 16 h + 4 g + j   (x scale)
//   WvF [t][P][hi | lo][lane] x 16 B   A rows o = 16 t + m,        k slot (g, j) <-> the same channel of Xbar_t
//   WoF [u][s][hi | lo][lane] x 16 B   A rows p = 16 u + m,        k slot (g, j) <-> o = 32 s + 16 (j / 4) + 4 g + j % 4
//   WkF2 [p][u][hi | lo][lane] x 16 B  WkF (x log2 e) of heads 2 p (j < 4) and 2 p + 1 (j >= 4) side by side: one K = 32 instruction
//                                      per head PAIR in k_attn_kvh<.., QP> (its B operand is zero outside the column's head)
#define ATTN_QO16_WAVES 8
template <int CG>
struct AttnBlob {
    static constexpr int NT = CG / 16, NP = CG / 32;
    static constexpr int WQ = 0, WK = WQ + NT * NP * 2 * 64 * 16, WV = WK + NT * NT * 2 * 64 * 8, WO = WV + NT * NP * 2 * 64 * 16,
                         WK2 = WO + NT * NP * 2 * 64 * 16, WV2 = WK2 + (NT / 2) * NT * 2 * 64 * 16,
                         BYTES = WV2 + NT * NP * 2 * 64 * 16;
    // WvF2 [t][P][hi | lo][lane] x 16 B (round 6): Wv for the window launch -- A rows o = 16 t + m, k slot (g, j) <-> channel
    // 32 P + 16 (g % 2) + 8 (j / 4) + 4 (g / 2) + j % 4 = the order in which k_attn_kvh's Xbar accumulators sit in its lanes
};

template <int CG>
__global__ void __launch_bounds__(MSSVT_WAVE) k_attn_pack(const float *Wq, const float *Wkv, const float *Wo, float scale, char *blob) {
    using L = AttnBlob<CG>;
    constexpr int NT = L::NT, NP = L::NP;
    const int lane = lane_id(), m = lane & 15, g = lane >> 4, f = blockIdx.x;  // fragment index within its matrix
    const int which = blockIdx.y;                                              // 0 Wq, 1 Wk, 2 Wv, 3 Wo, 4 Wk head pairs, 5 Wv (window launch)
    if (which == 1) {
        if (f >= NT * NT) return;
        const int h = f / NT, u = f % NT;
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = Wkv[(size_t)(16 * h + 4 * g + j) * CG + (16 * u + m)] * scale;
        h16x4 hi, lo;
        split4_rtz(v, hi, lo);
        h16x4 *dst = reinterpret_cast<h16x4 *>(blob + L::WK) + (size_t)f * 2 * 64 + lane;
        dst[0] = hi;
        dst[64] = lo;
        return;
    }
    if (which == 4) {
        if (f >= (NT / 2) * NT) return;
        const int pr = f / NT, u = f % NT;
        f32x4 v0, v1;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // (x log2 e: k_attn_kvh<.., QP> takes its softmax in base 2)
            v0[j] = Wkv[(size_t)(16 * (2 * pr) + 4 * g + j) * CG + (16 * u + m)] * (scale * 1.4426950408889634f);
            v1[j] = Wkv[(size_t)(16 * (2 * pr + 1) + 4 * g + j) * CG + (16 * u + m)] * (scale * 1.4426950408889634f);
        }
        h16x8 hi, lo;
        split8_rtz(v0, v1, hi, lo);
        h16x8 *dst = reinterpret_cast<h16x8 *>(blob + L::WK2) + (size_t)f * 2 * 64 + lane;
        dst[0] = hi;
        dst[64] = lo;
        return;
    }
    if (f >= NT * NP) return;
    const int t = f / NP, P = f % NP;
    if (which == 5) {  // Wv in the lane order of k_attn_kvh's Xbar tiles (AttnBlob::WV2)
        const float *rowp = Wkv + (size_t)(CG + 16 * t + m) * CG + 32 * P + 16 * (g & 1) + 4 * (g >> 1);
        const float4 w0 = *reinterpret_cast<const float4 *>(rowp), w1 = *reinterpret_cast<const float4 *>(rowp + 8);
        h16x8 hi, lo;
        split8_rtz(f32x4{w0.x, w0.y, w0.z, w0.w}, f32x4{w1.x, w1.y, w1.z, w1.w}, hi, lo);
        h16x8 *dst = reinterpret_cast<h16x8 *>(blob + L::WV2) + (size_t)f * 2 * 64 + lane;
        dst[0] = hi;
        dst[64] = lo;
        return;
    }
    // 8 k slots of a lane = two runs of 4 consecutive columns, 16 apart (kv16 operand order)
    const float *rowp = (which == 0 ? Wq + (size_t)(16 * t + m) * CG : which == 2 ? Wkv + (size_t)(CG + 16 * t + m) * CG
                                                                                  : Wo + (size_t)(16 * t + m) * CG) + 32 * P + 4 * g;
    const float4 w0 = *reinterpret_cast<const float4 *>(rowp), w1 = *reinterpret_cast<const float4 *>(rowp + 16);
    h16x8 hi, lo;
    split8_rtz(f32x4{w0.x, w0.y, w0.z, w0.w}, f32x4{w1.x, w1.y, w1.z, w1.w}, hi, lo);
    h16x8 *dst = reinterpret_cast<h16x8 *>(blob + (which == 0 ? L::WQ : which == 2 ? L::WV : L::WO)) + (size_t)f * 2 * 64 + lane;
    dst[0] = hi;
    dst[64] = lo;
}

// straight copy of n16 16-byte pieces into the LDS, every load of a thread in flight before its first store (in two
// halves, so that a caller can put loads of its own between them: k_attn_kvh)
template <int N16, int THREADS>
__device__ __forceinline__ void attn_stage16_load(float4 (&v)[(N16 + THREADS - 1) / THREADS], const float4 *src) {
#pragma unroll
    for (int k = 0; k < (N16 + THREADS - 1) / THREADS; ++k) {
        const int e = threadIdx.x + k * THREADS;
        if (N16 % THREADS == 0 || e < N16) v[k] = src[e];
    }
}
template <int N16, int THREADS>
__device__ __forceinline__ void attn_stage16_store(float4 *lds, const float4 (&v)[(N16 + THREADS - 1) / THREADS]) {
#pragma unroll
    for (int k = 0; k < (N16 + THREADS - 1) / THREADS; ++k) {
        const int e = threadIdx.x + k * THREADS;
        if (N16 % THREADS == 0 || e < N16) lds[e] = v[k];
    }
}
template <int N16, int THREADS>
__device__ __forceinline__ void attn_stage16(float4 *lds, const float4 *src) {
    float4 v[(N16 + THREADS - 1) / THREADS];
    attn_stage16_load<N16, THREADS>(v, src);
    attn_stage16_store<N16, THREADS>(lds, v);
}

// ---- A, kv16 form: rows -> Qt.  OUT 0: Qt in fp32 for k_attn_kv; 1: Qt as (hi, lo) fragments for k_attn_kvh<.., false>;
// 2: only Q' (scaled by the Wk fragments later) as (hi, lo) B fragments of the K = 16 product, [head][g][hi x 4 | lo x 4]
// = 4 Cg bytes at the start of the row -- k_attn_kvh<.., true> multiplies by Wk_h itself: a quarter of the hand-off bytes
// (this launch is bound by writing them: 67 MB for 33 k query rows) and of this launch's matrix work
// (sched_barriers: without them the scheduler hoists the fragment reads of every step and spills ~100 registers)
template <int CG, int HP, int OUT>
__global__ void __launch_bounds__(ATTN_QO16_WAVES *MSSVT_WAVE, 4) k_attn_q16(AttnPack pack) {
    const AttnArgs &a = pack.g[blockIdx.y];
    using L = AttnBlob<CG>;
    constexpr int NT = CG / 16, NP = CG / 32, QROW = HP * CG;
    extern __shared__ float4 lds4[];
    const h16x8 *WqF = reinterpret_cast<const h16x8 *>(lds4);
    const h16x4 *WkF = reinterpret_cast<const h16x4 *>(reinterpret_cast<const char *>(lds4) + L::WK);
    constexpr int STAGED = OUT == 2 ? L::WK : L::WV;  // Wq fragments (+ Wk fragments)
    float *bq_l = reinterpret_cast<float *>(reinterpret_cast<char *>(lds4) + STAGED);
    const int lane = lane_id(), r = lane & 15, g = lane >> 4;
    const int rows = *a.num_rows, tiles = (rows + 15) >> 4;
    const int wv = threadIdx.x / MSSVT_WAVE;
    if ((int)blockIdx.x >= tiles) return;
    int tile = wv * gridDim.x + blockIdx.x;
    float4 rm = a.qrow_meta[min(tile * 16 + r, rows - 1)];
    int2 src = a.qrow_src[min(tile * 16 + r, rows - 1)];
    attn_stage16<STAGED / 16, ATTN_QO16_WAVES * MSSVT_WAVE>(lds4, reinterpret_cast<const float4 *>(a.packed));
    if (threadIdx.x < CG) bq_l[threadIdx.x] = a.bq[threadIdx.x];
    // positional MLP as two K = 4 products (relative offset | 1, window centre): A row r of tile u <-> channel (16 * u + r)
    float wrel[NT], wctr[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const float *wp = a.Wp + (size_t)(a.c0 + (16 * u + r)) * 6;
        wrel[u] = g < 3 ? wp[g] : a.bp[a.c0 + (16 * u + r)];
        wctr[u] = g < 3 ? wp[3 + g] : 0.f;
    }
    float4 wc = a.wcentre[src.x];
    f32x4 xq[NT];  // piece S: channels 16 S + 4 g + i of the row
#define ATTN_Q16_ROWS()                                                                                   \
    {                                                                                                     \
        const float *xrow_ = a.xhat + (size_t)__builtin_bit_cast(int, rm.w) * a.C + a.c0 + 4 * g;         \
        _Pragma("unroll") for (int S = 0; S < NT; ++S) {                                                  \
            const float4 v_ = *reinterpret_cast<const float4 *>(xrow_ + 16 * S);                          \
            xq[S] = f32x4{v_.x, v_.y, v_.z, v_.w};                                                        \
        }                                                                                                 \
    }
    ATTN_Q16_ROWS()
    __syncthreads();
    for (bool first = true; tile < tiles; tile += gridDim.x * ATTN_QO16_WAVES, first = false) {
        const int row = min(tile * 16 + r, rows - 1);
        if (!first) {
            rm = a.qrow_meta[row];
            src = a.qrow_src[row];
            wc = a.wcentre[src.x];
            ATTN_Q16_ROWS()
        }
        const float relb = lane_pick4(g, rm.x, rm.y, rm.z, 1.0f);
        const float ctrb = lane_pick4(g, wc.x, wc.y, wc.z, 0.0f);
        h16x8 xh[NP], xl[NP];
#pragma unroll
        for (int P = 0; P < NP; ++P) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4 p1 = f32x4{0.f, 0.f, 0.f, 0.f};
                MFMA4(p1, wrel[2 * P + h], relb);
                MFMA4(p1, wctr[2 * P + h], ctrb);
#pragma unroll
                for (int i = 0; i < 4; ++i) xq[2 * P + h][i] += fmaxf(p1[i], 0.0f);
            }
            split8_rtz(xq[2 * P], xq[2 * P + 1], xh[P], xl[P]);
        }
        __builtin_amdgcn_sched_barrier(0);
        // GEMM1^T: Q'^T[o][row] = sum_c Wq[o][c] xq[row][c] + bq[o]; accumulator (row, g), i <-> o = 16 t + 4 g + i
        h16x4 qh[NT], ql[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float4 b = *reinterpret_cast<const float4 *>(bq_l + 16 * t + 4 * g);
            f32x4 mm = f32x4{b.x, b.y, b.z, b.w}, cr = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int P = 0; P < NP; ++P) {
                const h16x8 wh = WqF[((t * NP + P) * 2) * 64 + lane], wl = WqF[((t * NP + P) * 2 + 1) * 64 + lane];
                MFMA_H(mm, wh, xh[P]);
                MFMA_H(cr, wh, xl[P]);
                MFMA_H(cr, wl, xh[P]);
            }
            split4_rtz(f32x4{__builtin_fmaf(cr[0], SPLIT_INV, mm[0]), __builtin_fmaf(cr[1], SPLIT_INV, mm[1]),
                             __builtin_fmaf(cr[2], SPLIT_INV, mm[2]), __builtin_fmaf(cr[3], SPLIT_INV, mm[3])}, qh[t], ql[t]);
            if (t & 1) __builtin_amdgcn_sched_barrier(0);
        }
        const bool row_ok = tile * 16 + r < rows;
        float *dst = a.qbuf + (size_t)(tile * 16 + r) * QROW;
        if (OUT == 2) {  // lane (row, g) holds Q'[row][16 t + 4 g + i]: the B fragment of head t, lanes (., g)
            h16x8 *dq = reinterpret_cast<h16x8 *>(dst);
#pragma unroll
            for (int t = 0; t < NT; ++t)
                if (row_ok) dq[t * 4 + g] = split_cat(qh[t], ql[t]);
            continue;
        }
        // GEMM2^T per head (= tile h): Qt_h^T[c][row] = sum_{o in head h} (scale Wk[o][c]) Q'[row][o]
#pragma unroll
        for (int h = 0; h < NT; ++h) {
#pragma unroll
            for (int P = 0; P < NP; ++P) {
                f32x4 acc[2];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int u = 2 * P + e;
                    const h16x4 wh = WkF[((h * NT + u) * 2) * 64 + lane], wl = WkF[((h * NT + u) * 2 + 1) * 64 + lane];
                    f32x4 mm = f32x4{0.f, 0.f, 0.f, 0.f}, cr = mm;
                    MFMA_H16(mm, wh, qh[h]);
                    MFMA_H16(cr, wh, ql[h]);
                    MFMA_H16(cr, wl, qh[h]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[e][i] = __builtin_fmaf(cr[i], SPLIT_INV, mm[i]);
                }
                if (OUT == 1) {
                    h16x8 *dsth = reinterpret_cast<h16x8 *>(dst + h * CG);
                    h16x8 hi, lo;
                    split8_rtz(acc[0], acc[1], hi, lo);
                    if (row_ok) {
                        dsth[(P * 4 + g) * 2] = hi;
                        dsth[(P * 4 + g) * 2 + 1] = lo;
                    }
                } else if (row_ok) {
                    store_handoff(dst + h * CG + (32 * P + 4 * g), acc[0]);
                    store_handoff(dst + h * CG + (32 * P + 16 + 4 * g), acc[1]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef ATTN_Q16_ROWS
}

// ---- C, kv16 form: Xbar -> attention output rows
template <int CG, int HP>
__global__ void __launch_bounds__(ATTN_QO16_WAVES *MSSVT_WAVE, 4) k_attn_o16(AttnPack pack) {
    const AttnArgs &a = pack.g[blockIdx.y];
    using L = AttnBlob<CG>;
    constexpr int NT = CG / 16, NP = CG / 32, QROW = HP * CG;
    extern __shared__ float4 lds4[];
    const h16x8 *WvF = reinterpret_cast<const h16x8 *>(lds4);
    const h16x8 *WoF = reinterpret_cast<const h16x8 *>(reinterpret_cast<const char *>(lds4) + (L::WO - L::WV));
    float *bv_l = reinterpret_cast<float *>(reinterpret_cast<char *>(lds4) + (L::WK2 - L::WV)), *bo_l = bv_l + CG;
    const int lane = lane_id(), r = lane & 15, g = lane >> 4;
    const int rows = *a.num_rows, tiles = (rows + 15) >> 4;
    const int wv = threadIdx.x / MSSVT_WAVE;
    if ((int)blockIdx.x >= tiles) return;
    int tile = wv * gridDim.x + blockIdx.x;
    f32x4 x[NT], xn[NT];  // piece S of one head's Xbar row: channels 16 S + 4 g + i
#define ATTN_O16_ROWS(dst_, row_, h_)                                                                     \
    {                                                                                                     \
        const float *xb_ = a.qbuf + (size_t)(row_) * QROW + (h_) * CG + 4 * g;                            \
        _Pragma("unroll") for (int S = 0; S < NT; ++S) {                                                  \
            const float4 t4_ = *reinterpret_cast<const float4 *>(xb_ + 16 * S);                           \
            dst_[S] = f32x4{t4_.x, t4_.y, t4_.z, t4_.w};                                                  \
        }                                                                                                 \
    }
    ATTN_O16_ROWS(x, min(tile * 16 + r, rows - 1), 0)
    attn_stage16<(L::WK2 - L::WV) / 16, ATTN_QO16_WAVES * MSSVT_WAVE>(
        lds4, reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(a.packed) + L::WV));
    if (threadIdx.x < CG) {
        bv_l[threadIdx.x] = a.bkv[CG + threadIdx.x];
        bo_l[threadIdx.x] = a.bo[threadIdx.x];
    }
    __syncthreads();
    for (bool first = true; tile < tiles; tile += gridDim.x * ATTN_QO16_WAVES, first = false) {
        const int row = min(tile * 16 + r, rows - 1);
        const bool row_ok = tile * 16 + r < rows;
        const int dest = a.qrow_src[row].y;
        if (!first) ATTN_O16_ROWS(x, row, 0)
        // GEMM3^T: V^T[o][row] = sum_c Wv[o][c] Xbar_{head(o)}[row][c] + bv[o]  (head of tile t = t)
        f32x4 v[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t + 1 < NT) ATTN_O16_ROWS(xn, row, t + 1)  // the next head's row pieces under this head's products
            const float4 b = *reinterpret_cast<const float4 *>(bv_l + 16 * t + 4 * g);
            f32x4 mm = f32x4{b.x, b.y, b.z, b.w}, cr = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int P = 0; P < NP; ++P) {
                h16x8 xh, xl;
                split8_rtz(x[2 * P], x[2 * P + 1], xh, xl);
                const h16x8 wh = WvF[((t * NP + P) * 2) * 64 + lane], wl = WvF[((t * NP + P) * 2 + 1) * 64 + lane];
                MFMA_H(mm, wh, xh);
                MFMA_H(cr, wh, xl);
                MFMA_H(cr, wl, xh);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) v[t][i] = __builtin_fmaf(cr[i], SPLIT_INV, mm[i]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int S = 0; S < NT; ++S) x[S] = xn[S];
        }
        // GEMM4^T: out^T[p][row] = sum_o Wo[p][o] V[row][o] + bo[p]; two V tiles = one 32-wide step of the B operand
        h16x8 vh[NP], vl[NP];
#pragma unroll
        for (int s = 0; s < NP; ++s) split8_rtz(v[2 * s], v[2 * s + 1], vh[s], vl[s]);
        float *dst = a.attn + (size_t)dest * a.C + a.c0 + 4 * g;
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const float4 b = *reinterpret_cast<const float4 *>(bo_l + 16 * u + 4 * g);
            f32x4 mm = f32x4{b.x, b.y, b.z, b.w}, cr = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < NP; ++s) {
                const h16x8 wh = WoF[((u * NP + s) * 2) * 64 + lane], wl = WoF[((u * NP + s) * 2 + 1) * 64 + lane];
                MFMA_H(mm, wh, vh[s]);
                MFMA_H(cr, wh, vl[s]);
                MFMA_H(cr, wl, vh[s]);
            }
            if (row_ok)
                *reinterpret_cast<float4 *>(dst + 16 * u) = make_float4(__builtin_fmaf(cr[0], SPLIT_INV, mm[0]), __builtin_fmaf(cr[1], SPLIT_INV, mm[1]),
                                                                        __builtin_fmaf(cr[2], SPLIT_INV, mm[2]), __builtin_fmaf(cr[3], SPLIT_INV, mm[3]));
            if (u & 1) __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef ATTN_O16_ROWS
}

// ---- B: keys, scores, softmax, xbar (one wavefront per window) ------------------------------------
// Per window the key tokens T[key][c] = xhat row + relu(pos. MLP) are needed in BOTH matrix-core
// operand layouts (lane l: a = l % 16, g = l / 16):
//   T1: lane (a = key % 16, g)  channels 16 S + 4 g + j   -> A operand of  S = T Qt^T   (reduce over c)
//   T2: lane (a = c % 16,  g)   keys     16 t + 4 g + i   -> A operand of  Xbar^T = T^T P (reduce over keys)
// T1 is gathered from HBM as 16-byte pieces of the rows and kept in registers; T2 is T1 transposed
// through a per-wave LDS tile (row stride Cg + 4: the b128 writes and the b32 column reads are both
// conflict free).  The positional MLP is a K = 4 product (rel.x, rel.y, rel.z, 1) x (wp0, wp1, wp2,
// window part) = one MFMA per 16 x 16 tile.  Queries go through in passes of 16 / HP (column n =
// query * HP + head); the softmax over keys is 8 in-lane values + two cross-row shuffles, and the
// normalised P accumulator IS the B operand of the second product.  Key slots are not compacted:
// masked slots score -inf (the reference adds -100: weight <= e^-100); key tiles without an unmasked
// slot are skipped.  Software pipeline across windows: metadata two windows ahead, the feature rows
// of the next window in flight under this window's MFMAs.
#ifdef MSSVT_STAMPS
// per wave: [0] entry, [1] first rows issued, [2] exit, [3] windows done, [4..9] cycles summed over its windows:
// token build (waits for the row gathers), prefetch issue, tile -> LDS, scores + softmax (waits for Qt), PV + store, passes
__device__ unsigned long long g_attn_kv_stamps[8192 * 12];
extern "C" int mssvt_debug_read_attn_kv_stamps(unsigned long long *host) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_attn_kv_stamps), sizeof(g_attn_kv_stamps));
}
#define KVS_T() __builtin_readcyclecounter()
#else
#define KVS_T() 0ull
#endif
template <int CG, int HD, int HP, int KT>
__global__ void __launch_bounds__(ATTN_ROW_WAVES *MSSVT_WAVE, 2) k_attn_kv(AttnPack pack) {
    const AttnArgs &a = pack.g[blockIdx.y];
    unsigned long long ks_entry = KVS_T(), ks_first = 0, ks_sum[6] = {0, 0, 0, 0, 0, 0}, ks_n = 0, ks_t = 0;
    (void)ks_entry; (void)ks_first; (void)ks_sum; (void)ks_n; (void)ks_t;
    constexpr int CGP = (CG + 15) / 16 * 16, NT = CGP / 16, NH = CG / HD, QROW = HP * CG, QPP = 16 / HP;
    constexpr int LSK = CGP + 4;  // LDS row stride of the key tile
    extern __shared__ float4 lds4[];
    const int lane = lane_id(), la = lane & 15, g = lane >> 4;
    const int wv = threadIdx.x / MSSVT_WAVE;
    float *Tl = reinterpret_cast<float *>(lds4) + (size_t)wv * KT * 16 * LSK;
    // positional MLP operand of this lane (channel 16 u + la, input g): constant part + window part
    float wconst[NT], w3[NT], w4[NT], w5[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int c = 16 * u + la;
        const bool in = CGP == CG || c < CG;
        const float *wp = a.Wp + (size_t)(a.c0 + (in ? c : 0)) * 6;
        wconst[u] = in ? (g < 3 ? wp[g] : a.bp[a.c0 + c]) : 0.f;
        w3[u] = in && g == 3 ? wp[3] : 0.f;
        w4[u] = in && g == 3 ? wp[4] : 0.f;
        w5[u] = in && g == 3 ? wp[5] : 0.f;
    }
    // static round-robin over the heaviest-first work order: wave i takes entries i, i + T, i + 2T ...
    // (T = waves in the grid), i.e. one window of every weight tier -- as balanced as dynamic tickets
    // without their atomics (a drained single-address ticket costs ~11 ns chip-wide, x 8192 waves)
    const int n_act = __builtin_amdgcn_readfirstlane(*a.num_wins);
    const int wstep = gridDim.x * ATTN_ROW_WAVES;
    const int K = a.K;
    int wi = __builtin_amdgcn_readfirstlane(blockIdx.x * ATTN_ROW_WAVES + wv);  // wave-uniform: scalar metadata loads
    if (wi >= n_act) return;
    // gathers through buffer descriptors: 32-bit lane offsets instead of 64-bit address arithmetic per load
    const __amdgpu_buffer_rsrc_t xr_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.xhat), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t km_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(a.kmeta), 0, -1, 0x00020000);
    const unsigned row_bytes = (unsigned)a.C * 4u, lane_off = ((unsigned)a.c0 + 4u * g) * 4u;
#define KV_ROW4(off_, S_) __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr_rs, (off_) + 64u * (S_), 0, 0))
    // Software pipeline over the wave's windows with every load of the loop body UNCONDITIONAL (indices clamped
    // to the last window; rows of empty slots read row 0): a guarded load makes the wait counts path dependent and
    // the compiler falls back to vmcnt(0), which drains the prefetches.  vmcnt retires in order -- a wait for a
    // load also waits for every load issued before it -- hence window ids three steps ahead (stage P, scalar),
    // metadata two (stage M: centre / counts scalar, key slots vector), raw rows one (stage R).
    int w_p;
    // stage M: metadata of a window (perm -> kmeta would otherwise be dependent round trips per window)
    float4 wc_m, km_m[KT];
    int nqv_m, qbase_m;
#define KV_LOAD_META()                                                                     \
    {                                                                                      \
        wc_m = a.wcentre[w_p];                                                             \
        nqv_m = a.nq_valid[w_p];                                                           \
        qbase_m = a.q_off[w_p];                                                            \
        _Pragma("unroll") for (int t = 0; t < KT; ++t)                                     \
            km_m[t] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(    \
                km_rs, ((unsigned)w_p * (unsigned)K + (unsigned)min(16 * t + la, K - 1)) * 16u, 0, 0)); \
    }
    // stage R: resolved metadata + raw feature rows of a window (T1 layout)
    float4 wc_r;
    int nqv_r, qbase_r;
    float rel_r[KT];
    unsigned vmask_r;    // bit 4 t + i: key 16 t + 4 g + i is unmasked
    unsigned used_r;     // bit t: tile t has an unmasked key (wave-uniform)
    f32x4 T1n[KT][NT];
#define KV_ISSUE_ROWS()                                                                    \
    {                                                                                      \
        wc_r = wc_m; nqv_r = nqv_m; qbase_r = qbase_m;                                     \
        vmask_r = 0; used_r = 0;                                                           \
        _Pragma("unroll") for (int t = 0; t < KT; ++t) {                                   \
            const int r_ = __builtin_bit_cast(int, km_m[t].w);                             \
            const bool ok_ = 16 * t + la < K && r_ >= 0;                                   \
            const unsigned long long bal_ = __ballot(ok_);  /* bits 0..15: keys 16 t + 0..15 */ \
            vmask_r |= (unsigned)((bal_ >> (4 * g)) & 15ull) << (4 * t);                   \
            used_r |= (t == 0 || (bal_ & 0xFFFFull) != 0ull) ? 1u << t : 0u;               \
            rel_r[t] = lane_pick4(g, km_m[t].x, km_m[t].y, km_m[t].z, 1.0f); \
            const unsigned ro_ = (unsigned)__umul24((unsigned)(ok_ ? r_ : 0), row_bytes) + lane_off; \
            _Pragma("unroll") for (int S = 0; S < NT; ++S)                                 \
                T1n[t][S] = (CGP == CG || 16 * S + 4 * g < CG) ? KV_ROW4(ro_, S) : f32x4{0.f, 0.f, 0.f, 0.f}; \
        }                                                                                  \
    }
    const int w_last = n_act - 1;
    w_p = a.perm[wi];
    KV_LOAD_META()
    w_p = a.perm[min(wi + wstep, w_last)];
    KV_ISSUE_ROWS()
    KV_LOAD_META()
    w_p = a.perm[min(wi + 2 * wstep, w_last)];
    ks_first = KVS_T();
    for (; wi < n_act; wi += wstep) {
        ks_t = KVS_T();
        // ---- this window: stage R -> working registers ------------------------------------------------
        const float4 wc = wc_r;
        // a window whose rows would not fit the compact arrays is skipped (cannot happen with the caller's bound)
        const int nqv = qbase_r + nqv_r <= a.row_capacity ? nqv_r : 0;
        const size_t qbase = (size_t)qbase_r;
        const unsigned vmask = vmask_r, used = used_r;
        f32x4 T1[KT][NT];
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            if (!(used >> t & 1)) continue;
            // + relu(positional MLP): rows = channels 16 u + 4 g + i, column = key 16 t + la
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const float wu = ((wconst[u] + w3[u] * wc.x) + w4[u] * wc.y) + w5[u] * wc.z;
                f32x4 p1 = f32x4{0.f, 0.f, 0.f, 0.f};
                MFMA4(p1, wu, rel_r[t]);
#pragma unroll
                for (int i = 0; i < 4; ++i) T1[t][u][i] = T1n[t][u][i] + fmaxf(p1[i], 0.0f);
            }
        }
#ifdef MSSVT_STAMPS
        asm volatile("" :: "v"(T1[0][0][0]));
        { const unsigned long long t_ = KVS_T(); ks_sum[0] += t_ - ks_t; ks_t = t_; }
#endif
        // first query pass: its Qt rows travel while the key tile is transposed
        const int hh = la % HP;
        const bool head_ok = hh < NH;
        float *qrow = a.qbuf + (qbase + min(la / HP, nqv - 1)) * QROW + (head_ok ? hh : 0) * CG;
        f32x4 qt[NT];
#pragma unroll
        for (int S = 0; S < NT; ++S) {
            const int c = 16 * S + 4 * g;
            const float4 v = (CGP == CG || c < CG) ? *reinterpret_cast<const float4 *>(qrow + c)
                                                   : make_float4(0.f, 0.f, 0.f, 0.f);
            qt[S] = f32x4{v.x, v.y, v.z, v.w};
        }
        // ---- next window: rows in flight under this window's MFMAs, metadata one further ahead (past the end
        // of the work list the last window is fetched again) ------------------------------------------------
        KV_ISSUE_ROWS()
        KV_LOAD_META()
        w_p = a.perm[min(wi + 3 * wstep, w_last)];
#ifdef MSSVT_STAMPS
        { const unsigned long long t_ = KVS_T(); ks_sum[1] += t_ - ks_t; ks_t = t_; }
#endif
        // key tile -> LDS (the T2 operand is read back column-wise)
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            if (!(used >> t & 1)) continue;
#pragma unroll
            for (int S = 0; S < NT; ++S)
                *reinterpret_cast<float4 *>(Tl + (16 * t + la) * LSK + 16 * S + 4 * g) =
                    make_float4(T1[t][S][0], T1[t][S][1], T1[t][S][2], T1[t][S][3]);
        }
        wave_lds_sync();
#ifdef MSSVT_STAMPS
        { const unsigned long long t_ = KVS_T(); ks_sum[2] += t_ - ks_t; ks_t = t_; }
#endif
        // queries, QPP per pass: column la = query * HP + head
        for (int q0 = 0; q0 < nqv; q0 += QPP) {
            ++ks_sum[5];
            const int q = q0 + la / HP;
            const bool q_ok = q < nqv && head_ok;
            if (q0 > 0) {
                qrow = a.qbuf + (qbase + min(q, nqv - 1)) * QROW + (head_ok ? hh : 0) * CG;
#pragma unroll
                for (int S = 0; S < NT; ++S) {
                    const int c = 16 * S + 4 * g;
                    const float4 v = (CGP == CG || c < CG) ? *reinterpret_cast<const float4 *>(qrow + c)
                                                           : make_float4(0.f, 0.f, 0.f, 0.f);
                    qt[S] = f32x4{v.x, v.y, v.z, v.w};
                }
            }
            // scores: S[key][col] = sum_c T[key][c] Qt[col][c]; even / odd channel tiles accumulate
            // separately (two independent MFMA chains per key tile)
            f32x4 sc[KT], sc2[KT];
#pragma unroll
            for (int t = 0; t < KT; ++t) sc[t] = sc2[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            // Tiles in DESCENDING order, tile 0 (never empty: slot 0 of a list is never masked) unconditionally and
            // last: the reads below then follow a chain in straight-line code -- behind a branch that skips the tail
            // of the chain the compiler's padding came out one wait state short (tools/mfma_hazard_check.py)
#pragma unroll
            for (int t = KT - 1; t >= 0; --t) {
                if (t > 0 && !(used >> t & 1)) continue;
#pragma unroll
                for (int S = 0; S < NT; S += 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        MFMA4(sc[t], T1[t][S][j], qt[S][j]);
                        if (S + 1 < NT) MFMA4(sc2[t], T1[t][S + 1][j], qt[S + 1][j]);
                    }
                }
            }
            // softmax over the unmasked keys: lane (col, g) holds keys 16 t + 4 g + i
            float mx = -INFINITY;
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    sc[t][i] += sc2[t][i];
                    mx = fmaxf(mx, (vmask >> (4 * t + i) & 1) ? sc[t][i] : -INFINITY);
                }
            mx = fmaxf(mx, lane_xor16(mx));
            mx = fmaxf(mx, lane_xor32(mx));
            float sum = 0.f;
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float e = (vmask >> (4 * t + i) & 1) ? __expf(sc[t][i] - mx) : 0.0f;
                    sc[t][i] = e;
                    sum += e;
                }
            sum += lane_xor16(sum);
            sum += lane_xor32(sum);
            const float inv = __builtin_amdgcn_rcpf(sum);  // slot 0 of a list is never masked: sum >= 1
#ifdef MSSVT_STAMPS
            asm volatile("" :: "v"(inv));
            { const unsigned long long t_ = KVS_T(); ks_sum[3] += t_ - ks_t; ks_t = t_; }
#endif
            // Xbar^T[c][col] = sum_key T[key][c] P[key][col]; A operand = the LDS tile read column-wise
            f32x4 acc[NT];
#pragma unroll
            for (int u = 0; u < NT; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = KT - 1; t >= 0; --t) {  // (descending, tile 0 unconditionally: as for the scores)
                if (t > 0 && !(used >> t & 1)) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float pv = sc[t][i] * inv;
                    const float *col = Tl + (16 * t + 4 * g + i) * LSK + la;
                    float tv[NT];
#pragma unroll
                    for (int u = 0; u < NT; ++u) tv[u] = col[16 * u];
#pragma unroll
                    for (int u = 0; u < NT; ++u) MFMA4(acc[u], tv[u], pv);
                }
            }
            if (q_ok) {
#pragma unroll
                for (int u = 0; u < NT; ++u) {
                    const int c = 16 * u + 4 * g;
                    if (CGP == CG || c < CG)  // xbar replaces qt in place (this lane's own 16 bytes)
                        store_handoff(qrow + c, acc[u]);
                }
            }
#ifdef MSSVT_STAMPS
            { const unsigned long long t_ = KVS_T(); ks_sum[4] += t_ - ks_t; ks_t = t_; }
#endif
        }
        wave_lds_sync();  // the next window rewrites the tile
        ++ks_n;
    }
#ifdef MSSVT_STAMPS
    {
        const int wid = (blockIdx.y * gridDim.x + blockIdx.x) * ATTN_ROW_WAVES + wv;
        if (lane == 0 && wid < 8192) {
            unsigned long long *o = g_attn_kv_stamps + (size_t)wid * 12;
            o[0] = ks_entry; o[1] = ks_first; o[2] = KVS_T(); o[3] = ks_n;
            for (int i = 0; i < 6; ++i) o[4 + i] = ks_sum[i];
        }
    }
#endif
#undef ATTN_Q_ROWS
#undef ATTN_O_ROWS
#undef KV_LOAD_META
#undef KV_ISSUE_ROWS
#undef KV_ROW4
}


// ---- B, kv16 form: the same launch with split-fp16 matrix operands --------------------------------------------
// Launch B above is bound by the fp32 matrix instruction (v_mfma_f32_16x16x4_f32, 32 cycles for a 16 x 16 x 4 tile: 72 of
// them per window, pass and head group at K = 32 -- ~2.3 k of the ~3.2 k cycles a window keeps its SIMD busy).  Here every
// product sum is three v_mfma_f32_16x16x32_f16 on (hi, lo) halves (see h16_split4; fp32 accumulation, the error of the fp32
// instruction as in csrc/ffn.hip): 12 + 12 sixteen-cycle instructions per window and pass instead of 32 + 32 thirty-two-cycle
// ones.  What makes it cheaper here than in a single-launch form that projects the keys (round 2: ~20 fragment splits per window, slower): the
// key tokens are the only operand split in this kernel, ONCE per window (Qt arrives split from k_attn_q<KV16>, P is 8
// values per lane and pass), and the transposed operand of the second product comes out of the LDS image by
// ds_read_b64_tr_b16 instead of 32 scalar column reads.
//   channels: k slot (g, j) of step P <-> channel 32 P + 16 (j / 4) + 4 g + j % 4 in BOTH operands of the score product (two
//             dense 16-byte pieces of a key row per step; Qt is stored in that order by launch A); the image keeps the
//             lane's 8 slots together (column 32 P + 8 g + j), so the second product's output rows come out in slot
//             order and the Xbar store undoes the permutation in its address;
//   keys:     k slot (g, j) of step s <-> key 32 s + 16 (j / 4) + 4 g + j % 4 = the accumulator layout of two score tiles,
//             so the normalised scores are the B operand of the second product as they stand.
// LDS image per wave: [hi | lo][key][channel] fp16, rows of 2 CG + 16 bytes (36 KiB per workgroup at K = 32: three
// workgroups = 3 waves / SIMD per CU, the 170 registers that two pass bodies and the prefetched window need; the 8 rows a 32-lane half of a transposed read touches start 36 banks apart).  Unused key tiles that a pass body reads hold zeros (their P is 0, but the product needs finite
// operands).  The caller guarantees the fp16 range of tokens and Qt (fused._attn_kv16_ok).
#define KVH_RS(cg) (2 * (cg) + 16)  // bytes per image row: 16-byte aligned, 36 banks at Cg = 64 (transposed reads: one 2-way pair per half)
__device__ __forceinline__ h16x4 lds_read_tr16(const char *p) {
    return __builtin_bit_cast(h16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16(
        (__attribute__((address_space(3))) fp16v4 *)(p)));
}
// QP: the hand-off rows hold Q' fragments (k_attn_q16<.., 2>) and Qt_h = (scale Wk_h)^T q'_h is formed here, per pass, from the
// Wk fragments of the pack blob staged into the LDS: one product per head with the columns of the other heads zeroed in
// the B operand, all accumulated into one tile -- NH x NT x 3 K = 16 instructions for 1 instead of 4 row loads per lane
template <int CG, int HD, int HP, int KT, bool QP>
__global__ void __launch_bounds__(ATTN_ROW_WAVES *MSSVT_WAVE, KT <= 2 ? (QP || CG >= 64 ? 3 : 4) : 2) k_attn_kvh(AttnPack pack) {
    static_assert(!QP || (HD == 16 && (CG / HD) % 2 == 0), "Q' hand-off: head = one 16-row tile, heads in pairs");
    static_assert(CG % 32 == 0 && KT % 2 == 0, "32-channel and 32-key steps");
    const AttnArgs &a = pack.g[blockIdx.y];
    constexpr int NT = CG / 16, NP = CG / 32, NH = CG / HD, QROW = HP * CG, QPP = 16 / HP;
    constexpr int RS = KVH_RS(CG), IMG = KT * 16 * RS;  // bytes: image row, one (hi or lo) image
    extern __shared__ float4 lds4[];
    const int lane = lane_id(), la = lane & 15, g = lane >> 4;
    const int wv = threadIdx.x / MSSVT_WAVE;
    // bytes of fragments in front of the images: the Wk pair fragments
    constexpr int WKB = QP ? AttnBlob<CG>::WV2 - AttnBlob<CG>::WK2 : 0;
    char *Ti = reinterpret_cast<char *>(lds4) + WKB + (size_t)wv * 2 * IMG;
    const h16x8 *WkF2 = reinterpret_cast<const h16x8 *>(lds4);
    // A zero the compiler cannot see through.  A word loaded at a wave-uniform address is otherwise fetched through the scalar
    // cache, or copied to a scalar register right behind its vector load -- either way with a wait at the place of the
    // load.  With `vz` in its byte offset the word is an ordinary vector load: it returns in issue order with the loads around
    // it and is waited for where readfirstlane uses it.
    unsigned vz = 0;
    asm volatile("" : "+v"(vz));
#define KVH_WORD(ptr_, idx_) \
    (*reinterpret_cast<const int *>(reinterpret_cast<const char *>(ptr_) + ((unsigned)(idx_) * 4u + vz)))
    // Prologue: four dependent round trips -- window count, work order, metadata, rows -- with the Wk staging in flight
    // under the first two (it was five: staging + barrier in front of the same four).  The count is asked for FIRST, as
    // a vector load, and the staging pieces leave behind it before it is waited for; the wave's first three work-order
    // entries leave as soon as the count is there and travel during the LDS stores and the barrier.  (Reading the order
    // ahead of the count would save one more trip, but the entry points carry no window capacity, so no index of `perm`
    // at or beyond *num_wins can be bounded by its allocation.)
    // PAIRS: a step may hold two one-tile windows -- window B's slots 0 .. 15 take key tile 1, the query lists are concatenated
    // and a column masks the other window's tile: exp2(-inf) = +0 in the softmax sum, token x (+0) in the second product, so
    // every window's rows have the bits of its run as a single
    constexpr bool PAIRS = KT == 2 && QP;
    const int sstr = a.step_stride;
    const int n_act_v = KVH_WORD(a.num_steps, 0);
    // positional MLP operand of this lane: A row la of tile u <-> channel (16 * u + la), input g: the weight of the
    // relative offset (g < 3) | bias + window-centre part (g = 3: summed over the three lanes that hold its weights)
    float wrel[NT], wctr[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int c = (16 * u + la);
        const float *wp = a.Wp + (size_t)(a.c0 + c) * 6;
        const float w_rel = wp[min(g, 2)], w_ctr = wp[3 + min(g, 2)], b_ = a.bp[a.c0 + c];  // (no lane-dependent branch)
        wrel[u] = g < 3 ? w_rel : b_;
        wctr[u] = g < 3 ? w_ctr : 0.f;
    }
    constexpr int WK16 = (WKB > 0 ? WKB : 16) / 16;
    float4 wk_v[(WK16 + ATTN_ROW_WAVES * MSSVT_WAVE - 1) / (ATTN_ROW_WAVES * MSSVT_WAVE)];
    if (QP)
        attn_stage16_load<WK16, ATTN_ROW_WAVES * MSSVT_WAVE>(
            wk_v, reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(a.packed) + AttnBlob<CG>::WK2));
    const int n_act = __builtin_amdgcn_readfirstlane(n_act_v);
    const int wstep = gridDim.x * ATTN_ROW_WAVES;
    const int K = a.K;
    int wi = __builtin_amdgcn_readfirstlane(blockIdx.x * ATTN_ROW_WAVES + wv);
    const int w_last = n_act - 1;
    // the wave's first three windows, loaded without a branch: indices <= w_last, inside the *num_wins entries that
    // mssvt_plan_order wrote; with no active window at all the three loads read the count word again instead
    const int *perm0 = n_act > 0 ? a.steps : a.num_steps;
    const int sst0 = n_act > 0 ? sstr : 0, sb0 = PAIRS && n_act > 0 ? sstr - 1 : 0;  // (window B: the step's last word)
    const int w_p0 = KVH_WORD(perm0, max(min(wi, w_last), 0) * sst0);
    const int w_p1 = KVH_WORD(perm0, max(min(wi + wstep, w_last), 0) * sst0);
    const int w_p2 = KVH_WORD(perm0, max(min(wi + 2 * wstep, w_last), 0) * sst0);
    const int w_pb0 = KVH_WORD(perm0, max(min(wi, w_last), 0) * sst0 + sb0);
    const int w_pb1 = KVH_WORD(perm0, max(min(wi + wstep, w_last), 0) * sst0 + sb0);
    const int w_pb2 = KVH_WORD(perm0, max(min(wi + 2 * wstep, w_last), 0) * sst0 + sb0);
    if (QP) {  // before any wave can leave: every wave of the workgroup meets at the barrier
        attn_stage16_store<WK16, ATTN_ROW_WAVES * MSSVT_WAVE>(lds4, wk_v);
        __syncthreads();
    }
    if (wi >= n_act) return;
    const __amdgpu_buffer_rsrc_t xr_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.xhat), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t km_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float4 *>(a.kmeta), 0, -1, 0x00020000);
    const unsigned row_bytes = (unsigned)a.C * 4u, lane_off = ((unsigned)a.c0 + 4u * g) * 4u;
    // piece S of a row: channels 16 S + 4 g + i (dense: the four g lanes of a key read 64 contiguous bytes)
#define KVH_ROW4(off_, S_) __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xr_rs, (off_) + 64u * (S_), 0, 0))
    // the software pipeline of k_attn_kv: window ids three steps ahead, metadata two, raw rows one; every load unconditional.
    // The window id and the two counts are wave-uniform words that the NEXT iteration consumes.  Left to the compiler they
    // cross the loop edge in scalar registers, and the copy out of the loaded vector register -- with the wait for every
    // load issued before it, the next window's rows among them -- lands right behind the load: one full round trip per
    // window, the pipeline undone.  Their byte offsets therefore carry a zero the compiler cannot see through (`vz`): the
    // words stay in vector registers until readfirstlane at the point of use, one iteration later.
    int w_p, w_pb;
    float4 wc_m, wcb_m, km_m[KT];
    int nqv_m, qbase_m, nqvb_m, qbaseb_m;
    bool pair_m = false;  // (wave-uniform) the step whose metadata is in flight holds two windows
#define KVH_LOAD_META()                                                                    \
    {                                                                                      \
        const int w_ = __builtin_amdgcn_readfirstlane(w_p);                                \
        int wb_ = w_;                                                                      \
        if (PAIRS) {                                                                       \
            const int b_ = __builtin_amdgcn_readfirstlane(w_pb);                           \
            pair_m = sstr == 2 && b_ >= 0;                                                 \
            wb_ = pair_m ? b_ : w_;                                                        \
        }                                                                                  \
        wc_m = a.wcentre[w_];                                                              \
        nqv_m = KVH_WORD(a.nq_valid, w_);                                                  \
        qbase_m = KVH_WORD(a.q_off, w_);                                                   \
        if (PAIRS) {                                                                       \
            wcb_m = a.wcentre[wb_];                                                        \
            nqvb_m = KVH_WORD(a.nq_valid, wb_);                                            \
            qbaseb_m = KVH_WORD(a.q_off, wb_);                                             \
        }                                                                                  \
        _Pragma("unroll") for (int t = 0; t < KT; ++t) {                                   \
            const int wt_ = PAIRS && t == 1 ? wb_ : w_;                                    \
            const int sl_ = PAIRS && t == 1 && pair_m ? la : 16 * t + la;                  \
            km_m[t] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(    \
                km_rs, ((unsigned)wt_ * (unsigned)K + (unsigned)min(sl_, K - 1)) * 16u, 0, 0)); \
        }                                                                                  \
    }
    float4 wc_r, wcb_r;
    int nqv_r, qbase_r, nqvb_r = 0, qbaseb_r = 0;
    bool pair_r = false;
    float rel_r[KT];
    unsigned vmask_r, used_r;
    f32x4 T1n[KT][NT];
    // The first pass's Q' piece travels with the rows, one window ahead: loaded where it is used it is the youngest load
    // in flight, and the wait for it drains the next window's rows.  (Round 6 measured this alone and saw no gain, 52.1 /
    // 26.0 against 51.4 / 25.6 us: the scalar copies above drained the queue all the same.)
    h16x8 qp8_n = h16x8{0, 0, 0, 0, 0, 0, 0, 0};
    const int hh = la % HP;
    const bool head_ok = hh < NH;
#define KVH_ISSUE_ROWS()                                                                   \
    {                                                                                      \
        wc_r = wc_m;                                                                       \
        nqv_r = __builtin_amdgcn_readfirstlane(nqv_m);                                     \
        qbase_r = __builtin_amdgcn_readfirstlane(qbase_m);                                 \
        if (PAIRS) {                                                                       \
            pair_r = pair_m;                                                               \
            wcb_r = wcb_m;                                                                 \
            nqvb_r = pair_m ? __builtin_amdgcn_readfirstlane(nqvb_m) : 0;                  \
            qbaseb_r = __builtin_amdgcn_readfirstlane(qbaseb_m);                           \
        }                                                                                  \
        if (QP) {                                                                          \
            const int nq_ = qbase_r + nqv_r <= a.row_capacity ? nqv_r : 0;                 \
            const int nb_ = PAIRS && qbaseb_r + nqvb_r <= a.row_capacity ? nqvb_r : 0;     \
            const int qc_ = max(min(la / HP, nq_ + nb_ - 1), 0);                           \
            const size_t row_ = nb_ > 0 && qc_ >= nq_ ? (size_t)qbaseb_r + (size_t)(qc_ - nq_) : (size_t)qbase_r + (size_t)qc_; \
            qp8_n = reinterpret_cast<const h16x8 *>(a.qbuf + row_ * QROW)[(head_ok ? hh : 0) * 4 + g]; \
        }                                                                                  \
        vmask_r = 0; used_r = 0;                                                           \
        _Pragma("unroll") for (int t = 0; t < KT; ++t) {                                   \
            const int r_ = __builtin_bit_cast(int, km_m[t].w);                             \
            const bool ok_ = (PAIRS && t == 1 && pair_m ? la : 16 * t + la) < K && r_ >= 0; \
            const unsigned long long bal_ = __ballot(ok_);                                 \
            vmask_r |= (unsigned)((bal_ >> (4 * g)) & 15ull) << (4 * t);                   \
            used_r |= (t == 0 || (bal_ & 0xFFFFull) != 0ull) ? 1u << t : 0u;               \
            rel_r[t] = lane_pick4(g, km_m[t].x, km_m[t].y, km_m[t].z, 1.0f); \
            const unsigned ro_ = (unsigned)__umul24((unsigned)(ok_ ? r_ : 0), row_bytes) + lane_off; \
            _Pragma("unroll") for (int S = 0; S < NT; ++S) T1n[t][S] = KVH_ROW4(ro_, S);   \
        }                                                                                  \
    }
    w_p = w_p0; w_pb = w_pb0;
    KVH_LOAD_META()
    w_p = w_p1; w_pb = w_pb1;
    KVH_ISSUE_ROWS()
    KVH_LOAD_META()
    w_p = w_p2; w_pb = w_pb2;
    // transposed reads: lane 4 q + p of a 16-lane group addresses row q, columns 4 p .. 4 p + 3 of its 4 x 16 block
    const char *tr_base = Ti + (4 * g + (la >> 2)) * RS + 8 * (la & 3);
    for (; wi < n_act; wi += wstep) {
        const float4 wc = wc_r, wcb = wcb_r;
        // each window of a pair is clipped against the row capacity on its own; the passes walk both query lists, A's first
        const int nqa = qbase_r + nqv_r <= a.row_capacity ? nqv_r : 0;
        const int nqb = PAIRS && qbaseb_r + nqvb_r <= a.row_capacity ? nqvb_r : 0;  // (a single: 0)
        const int nqv = nqa + nqb;
        const size_t qbase = (size_t)qbase_r, qbaseb = (size_t)qbaseb_r;
        const bool pair = PAIRS && pair_r;
        const unsigned vmask = vmask_r, used = used_r;
        // every live key in the first half of the list (wave-uniform): KT = 2 -- in tile 0; KT = 4 -- in its first 32-key step
        const bool front = (used >> (KT / 2)) == 0u;
        // key tokens = row + relu(positional MLP), split once, straight into the image (both products read it: the score
        // product row-wise, the second one transposed -- no token registers live across the passes)
        float wu[NT];  // A operand of the positional product: once per window (the window centre), not once per key tile
        const auto make_wu = [&](const float4 c) __attribute__((always_inline)) {
            const float ctrb = lane_pick4(g, c.x, c.y, c.z, c.z);  // wctr is 0 for g = 3
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                float cs = wctr[u] * ctrb;
                cs += lane_xor16(cs);
                cs += lane_xor32(cs);
                wu[u] = g == 3 ? wrel[u] + cs : wrel[u];
            }
        };
        make_wu(wc);
#pragma unroll
        for (int t = 0; t < KT; ++t) {
            // zeros only where a pass body reads them: a dead tile beside a live one in a 32-key step (none at KT = 2,
            // where a dead tile 1 means the `front` body, which reads tile 0 alone)
            if (!(used >> t & 1) && (KT == 2 || (front && t >= KT / 2))) continue;
            if (PAIRS && t == 1 && pair) make_wu(wcb);  // tile 1 holds window B's keys: its own centre
#pragma unroll
            for (int P = 0; P < NP; ++P) {
                h16x8 th = h16x8{0, 0, 0, 0, 0, 0, 0, 0}, tl = th;
                if (used >> t & 1) {
                    f32x4 tk[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int u = 2 * P + h;
                        f32x4 p1 = f32x4{0.f, 0.f, 0.f, 0.f};
                        MFMA4(p1, wu[u], rel_r[t]);
#pragma unroll
                        for (int i = 0; i < 4; ++i) tk[h][i] = T1n[t][u][i] + fmaxf(p1[i], 0.0f);
                    }
                    split8_rtz(tk[0], tk[1], th, tl);
                }
                char *dst = Ti + (16 * t + la) * RS + 64 * P + 16 * g;  // key row 16 t + la, the lane's 8 k slots of step P
                *reinterpret_cast<h16x8 *>(dst) = th;
                *reinterpret_cast<h16x8 *>(dst + IMG) = tl;
            }
        }
        h16x8 qh[NP], ql[NP];
        h16x8 qp8 = qp8_n;  // Q' mode: (hi x 4 | lo x 4) of this lane's column
        if (!QP) {
            const h16x8 *qr_ = reinterpret_cast<const h16x8 *>(a.qbuf + (qbase + max(min(la / HP, nqv - 1), 0)) * QROW + (head_ok ? hh : 0) * CG);
#pragma unroll
            for (int P = 0; P < NP; ++P) {
                qh[P] = qr_[(P * 4 + g) * 2];
                ql[P] = qr_[(P * 4 + g) * 2 + 1];
            }
        }
        KVH_ISSUE_ROWS()
        KVH_LOAD_META()
        w_p = KVH_WORD(a.steps, min(wi + 3 * wstep, w_last) * sstr);
        if (PAIRS) w_pb = KVH_WORD(a.steps, min(wi + 3 * wstep, w_last) * sstr + sstr - 1);
        wave_lds_sync();
        // One pass body per set of live 32-key steps, chosen ONCE per window (`front` is known before its passes start), so
        // that a pass is straight-line code: FRONT -- every live key in the first half of the list.  KT = 2: tile 0 alone
        // (9.6 of 32 slots are live on the flagship frame): the softmax runs over its 4 values per lane, and the second
        // product takes tile 1's half of both operands as zero registers -- the same K = 32 instruction on the same operand
        // values as with zeros read back from the image and P = exp2(-inf) = +0, and the softmax loses only exact +0 terms
        // and -inf candidates: the bits of the two-tile body.  KT = 4: the second step is left out whole (its products
        // are +0 added to sums that are never -0); tiles are not told apart inside a step.
        const auto passes = [&](auto front_c) __attribute__((always_inline)) {
            constexpr int LT = decltype(front_c)::value ? KT / 2 : KT, LS = (LT + 1) / 2;  // tiles, 32-key steps this body reads
            for (int q0 = 0; q0 < nqv; q0 += QPP) {
                const int q = q0 + la / HP, qc = min(q, nqv - 1);
                const bool q_ok = q < nqv && head_ok;
                // the column's query: A's list first, then B's (a single: nqb = 0)
                const bool inb = PAIRS && nqb > 0 && qc >= nqa;
                const size_t qrow_i = inb ? qbaseb + (size_t)(qc - nqa) : qbase + (size_t)qc;
                float *xrow = a.qbuf + qrow_i * QROW + (head_ok ? hh : 0) * CG;
                // a pair's column keeps its own window's tile (bits 4 t .. 4 t + 3 of vmask: tile t)
                const unsigned vmq = pair ? (inb ? vmask & 0xF0u : vmask & 0x0Fu) : vmask;
                if (q0 > 0) {
                    if (QP) {
                        qp8 = reinterpret_cast<const h16x8 *>(a.qbuf + qrow_i * QROW)[(head_ok ? hh : 0) * 4 + g];
                    } else {
                        const h16x8 *qrow = reinterpret_cast<const h16x8 *>(xrow);
#pragma unroll
                        for (int P = 0; P < NP; ++P) {
                            qh[P] = qrow[(P * 4 + g) * 2];
                            ql[P] = qrow[(P * 4 + g) * 2 + 1];
                        }
                    }
                }
                if (QP) {
                    // Qt^T[c][col] = sum_h sum_{k < 16} (scale Wk)[16 h + k][c] Q'[q(col)][16 h + k] [h == head(col)]
                    const h16x4 z4 = h16x4{0, 0, 0, 0};
                    const h16x4 bh = h16x4{qp8[0], qp8[1], qp8[2], qp8[3]}, bl = h16x4{qp8[4], qp8[5], qp8[6], qp8[7]};
                    __builtin_amdgcn_sched_barrier(0);  // (the scheduler would hoist all 32 fragment reads: 70 spilled registers)
#pragma unroll
                    for (int P = 0; P < NP; ++P) {
                        f32x4 qt[2];
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const int u = 2 * P + e;
                            f32x4 mm = f32x4{0.f, 0.f, 0.f, 0.f}, cr = mm;
#pragma unroll
                            for (int pr = 0; pr < NH / 2; ++pr) {  // heads 2 pr | 2 pr + 1 in the two halves of the k slots
                                const h16x8 wh = WkF2[((pr * NT + u) * 2) * 64 + lane], wl = WkF2[((pr * NT + u) * 2 + 1) * 64 + lane];
                                const h16x8 sh = split_cat(hh == 2 * pr ? bh : z4, hh == 2 * pr + 1 ? bh : z4),
                                            sl = split_cat(hh == 2 * pr ? bl : z4, hh == 2 * pr + 1 ? bl : z4);
                                MFMA_H(mm, wh, sh);
                                MFMA_H(cr, wh, sl);
                                MFMA_H(cr, wl, sh);
                            }
#pragma unroll
                            for (int i = 0; i < 4; ++i) qt[e][i] = __builtin_fmaf(cr[i], SPLIT_INV, mm[i]);
                        }
                        split8_rtz(qt[0], qt[1], qh[P], ql[P]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                // scores S[key][col] = sum_c T[key][c] Qt[col][c]
                f32x4 sc[LT];
#pragma unroll
                for (int t = 0; t < LT; ++t) {
                    sc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (KT > 2 && !(used >> t & 1)) continue;  // (KT = 2: the body says which tiles are live)
                    f32x4 mm = sc[t], cr = sc[t];
#pragma unroll
                    for (int P = 0; P < NP; ++P) {
                        const char *src = Ti + (16 * t + la) * RS + 64 * P + 16 * g;
                        const h16x8 th = *reinterpret_cast<const h16x8 *>(src), tl = *reinterpret_cast<const h16x8 *>(src + IMG);
                        MFMA_H(mm, th, qh[P]);
                        MFMA_H(cr, th, ql[P]);
                        MFMA_H(cr, tl, qh[P]);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) sc[t][i] = __builtin_fmaf(cr[i], SPLIT_INV, mm[i]);
                }
                // softmax over the unmasked keys in base 2 (QP: log2 e is folded into the Wk fragments): masked slots score -inf
                float mx = -INFINITY;
#pragma unroll
                for (int t = 0; t < LT; ++t)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float sv = QP ? sc[t][i] : sc[t][i] * 1.4426950408889634f;
                        sc[t][i] = (vmq >> (4 * t + i) & 1) ? sv : -INFINITY;
                        mx = fmaxf(mx, sc[t][i]);
                    }
                mx = fmaxf(mx, lane_xor16(mx));
                mx = fmaxf(mx, lane_xor32(mx));
                float sum = 0.f;
#pragma unroll
                for (int t = 0; t < LT; ++t)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float e = __builtin_amdgcn_exp2f(sc[t][i] - mx);  // slot 0 of a list is never masked: mx is finite
                        sc[t][i] = e;
                        sum += e;
                    }
                sum += lane_xor16(sum);
                sum += lane_xor32(sum);
                const float inv = __builtin_amdgcn_rcpf(sum);
                // Xbar^T[c][col] = sum_key T[key][c] P[key][col]
                const h16x4 z4 = h16x4{0, 0, 0, 0};
                h16x8 ph[LS], pl[LS];
                if constexpr (LT == 1) {  // the step's second tile: P = 0 and zero tokens, as registers
                    h16x4 h0, l0;
                    split4_rtz(sc[0] * inv, h0, l0);
                    ph[0] = split_cat(h0, z4);
                    pl[0] = split_cat(l0, z4);
                } else {
#pragma unroll
                    for (int s = 0; s < LS; ++s) split8_rtz(sc[2 * s] * inv, sc[2 * s + 1] * inv, ph[s], pl[s]);
                }
#pragma unroll
                for (int u = 0; u < NT; ++u) {
                    f32x4 mm = f32x4{0.f, 0.f, 0.f, 0.f}, cr = mm;
#pragma unroll
                    for (int s = 0; s < LS; ++s) {
                        const char *blk = tr_base + 32 * s * RS + 32 * u;
                        const h16x8 ah = split_cat(lds_read_tr16(blk), LT == 1 ? z4 : lds_read_tr16(blk + 16 * RS));
                        const h16x8 al = split_cat(lds_read_tr16(blk + IMG), LT == 1 ? z4 : lds_read_tr16(blk + IMG + 16 * RS));
                        MFMA_H(mm, ah, ph[s]);
                        MFMA_H(cr, ah, pl[s]);
                        MFMA_H(cr, al, ph[s]);
                    }
                    const f32x4 xt = f32x4{__builtin_fmaf(cr[0], SPLIT_INV, mm[0]), __builtin_fmaf(cr[1], SPLIT_INV, mm[1]),
                                           __builtin_fmaf(cr[2], SPLIT_INV, mm[2]), __builtin_fmaf(cr[3], SPLIT_INV, mm[3])};
                    if (q_ok) {  // xbar replaces qt in place (this lane's own bytes of the row)
                        // image column 16 u + 4 g + i is k slot (2 (u % 2) + g / 2, 4 (g % 2) + i) of step u / 2 (see above)
                        store_handoff(xrow + 32 * (u >> 1) + 16 * (g & 1) + 8 * (u & 1) + 4 * (g >> 1), xt);
                    }
                }
            }
        };
        if (front)
            passes(std::integral_constant<bool, true>());
        else
            passes(std::integral_constant<bool, false>());
        wave_lds_sync();  // the next window rewrites the image
    }
#undef KVH_WORD
#undef KVH_LOAD_META
#undef KVH_ISSUE_ROWS
#undef KVH_ROW4
}

template <int CG, int HD, int HP>
static int launch_block_attn(const AttnPack &pack, int ng, int row_capacity, bool kv16, bool paired, hipStream_t stream) {
    constexpr int CGP = (CG + 15) / 16 * 16, LS = CGP + 4;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        cus = 256;
    // A / C: persistent over 16-row tiles, one 16-wave workgroup per CU and head group at most
    const int tiles_cap = (row_capacity + 15) / 16;
    int row_grid = tiles_cap;
    if (row_grid > cus / ng) row_grid = cus / ng;
    if (row_grid < 1) row_grid = 1;
    const size_t lds_q = ((size_t)2 * CGP * LS + CGP * 8 + CGP) * 4, lds_o = ((size_t)2 * CGP * LS + 2 * CGP) * 4;
    const int K = pack.g[0].K;
    if constexpr (CG % 32 == 0) {
        if (kv16 && K > 16 && K <= 64) {  // split-fp16 operands in launch B (k_attn_kvh); A writes Qt pre-split
            constexpr int RS = KVH_RS(CG);
            // resident workgroups per CU.  (K <= 32 without blobs ran four at 128 registers and 6 spilled ones; with a pass body
            // per tile set it spilled 45 there -- 159 / 76 us for the three launches on the flagship tables -- and takes 99 / 47 at
            // three, against 106 / 48 before)
            const int wgs = K <= 32 ? (CG >= 64 ? 3 : 4) : 2;  // (Cg = 32 fits 128 registers: four, as before)
            const dim3 kv_grid(cus * wgs / ng > 0 ? cus * wgs / ng : 1, ng);
            const size_t img = (size_t)ATTN_ROW_WAVES * 2 * 16 * RS;  // per key tile of 16 slots, all waves, hi + lo
            bool packed = HD == 16;
            for (int g = 0; g < ng; ++g) packed = packed && pack.g[g].packed != nullptr;
            int grid16 = tiles_cap;  // 8-wave workgroups, two per CU
            if (grid16 > cus * 2 / ng) grid16 = cus * 2 / ng;
            if (grid16 < 1) grid16 = 1;
            // packed weights: A and C as k_attn_q16 / k_attn_o16, and at K <= 32 the Q' hand-off (Qt formed in the window launch)
            const bool qp = packed && K <= 32;
            if (paired && !(qp && HD == 16)) return MSSVT_E_TOOLARGE;  // only k_attn_kvh<.., 2, true> walks step pairs
            if constexpr (HD == 16) {
                if (qp) {
                    using L = AttnBlob<CG>;
                    const dim3 qp_grid(cus * 3 / ng > 0 ? cus * 3 / ng : 1, ng);
                    k_attn_q16<CG, HP, 2><<<dim3(grid16, ng), ATTN_QO16_WAVES * MSSVT_WAVE, L::WK + CG * 4, stream>>>(pack);
                    k_attn_kvh<CG, HD, HP, 2, true><<<qp_grid, ATTN_ROW_WAVES * MSSVT_WAVE, (L::WV2 - L::WK2) + 2 * img, stream>>>(pack);
                }
            }
            if constexpr (HD == 16) {
                if (packed && !qp)
                    k_attn_q16<CG, HP, 1><<<dim3(grid16, ng), ATTN_QO16_WAVES * MSSVT_WAVE, AttnBlob<CG>::WV + CG * 4, stream>>>(pack);
            }
            if (!packed)
                k_attn_q<CG, HD, HP, true><<<dim3(row_grid, ng), ATTN_QO_WAVES * MSSVT_WAVE, lds_q, stream>>>(pack);
            if (qp) {
            } else if (K <= 32)
                k_attn_kvh<CG, HD, HP, 2, false><<<kv_grid, ATTN_ROW_WAVES * MSSVT_WAVE, 2 * img, stream>>>(pack);
            else {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_attn_kvh<CG, HD, HP, 4, false>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * img));
                if (e != hipSuccess) return (int)e;
                k_attn_kvh<CG, HD, HP, 4, false><<<kv_grid, ATTN_ROW_WAVES * MSSVT_WAVE, 4 * img, stream>>>(pack);
            }
            if constexpr (HD == 16) {
                if (packed)
                    k_attn_o16<CG, HP><<<dim3(grid16, ng), ATTN_QO16_WAVES * MSSVT_WAVE, AttnBlob<CG>::WK2 - AttnBlob<CG>::WV + 2 * CG * 4, stream>>>(pack);
            }
            if (!packed)
                k_attn_o<CG, HD, HP><<<dim3(row_grid, ng), ATTN_QO_WAVES * MSSVT_WAVE, lds_o, stream>>>(pack);
            return mssvt_launch_status();
        }
    }
    if (paired) return MSSVT_E_TOOLARGE;
    k_attn_q<CG, HD, HP, false><<<dim3(row_grid, ng), ATTN_QO_WAVES * MSSVT_WAVE, lds_q, stream>>>(pack);
    // B: persistent over the work order with exactly the waves that are resident (3 workgroups of 4 waves per CU at the
    // 164 VGPRs of the K = 32 instantiation): every further workgroup would run in a later round and pay the prologue
    // (positional weights, three dependent metadata round trips: ~9 k cycles, as much as one window) again for its few
    // windows -- 8 per CU: 47.0 us mean per launch, 3 per CU: 42.9 us.  Measured and dropped (round 3): one wave per
    // window without a work list (the ~37 k empty workgroups of a capacity-sized grid cost 5 k cycles each: 92 us), and
    // the same pipeline squeezed under 128 VGPRs for 4 waves / SIMD (18 spilled registers, 63 us): per window the SIMD
    // is busy ~3.2 k of the wave's 9.7 k cycles, more than half of it fp32 matrix instructions -- not a latency problem.
    const dim3 kv_grid(cus * 3 / ng > 0 ? cus * 3 / ng : 1, ng);
    const size_t lds_tile = (size_t)ATTN_ROW_WAVES * 16 * LS * 4;  // per key tile of 16 slots, all waves
    if (K <= 16)
        k_attn_kv<CG, HD, HP, 1><<<kv_grid, ATTN_ROW_WAVES * MSSVT_WAVE, lds_tile, stream>>>(pack);
    else if (K <= 32)
        k_attn_kv<CG, HD, HP, 2><<<kv_grid, ATTN_ROW_WAVES * MSSVT_WAVE, 2 * lds_tile, stream>>>(pack);
    else {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_attn_kv<CG, HD, HP, 4>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)(4 * lds_tile));
        if (e != hipSuccess) return (int)e;
        k_attn_kv<CG, HD, HP, 4><<<kv_grid, ATTN_ROW_WAVES * MSSVT_WAVE, 4 * lds_tile, stream>>>(pack);
    }
    k_attn_o<CG, HD, HP><<<dim3(row_grid, ng), ATTN_QO_WAVES * MSSVT_WAVE, lds_o, stream>>>(pack);
    return mssvt_launch_status();
}

static int dispatch_block_attn(const AttnPack &pack, int ng, int Cg, int head_dim, int row_capacity, bool kv16, bool paired, hipStream_t st) {
#define MSSVT_ATTN_CASE(cg, hd)                                   \
    if (Cg == cg && head_dim == hd)                               \
        return launch_block_attn<cg, hd, ((cg / hd + 3) / 4) * 4>(pack, ng, row_capacity, kv16, paired, st);
    MSSVT_ATTN_CASE(8, 8)
    MSSVT_ATTN_CASE(16, 8)
    MSSVT_ATTN_CASE(16, 16)
    MSSVT_ATTN_CASE(24, 8)
    MSSVT_ATTN_CASE(32, 8)
    MSSVT_ATTN_CASE(32, 16)
    MSSVT_ATTN_CASE(32, 32)
    MSSVT_ATTN_CASE(48, 16)
    MSSVT_ATTN_CASE(64, 8)
    MSSVT_ATTN_CASE(64, 16)
    MSSVT_ATTN_CASE(64, 32)
    return MSSVT_E_TOOLARGE;  // shape not instantiated: the caller falls back to the operator path
#undef MSSVT_ATTN_CASE
}

static int block_attention_impl(
    int C, int num_groups, const int *host_c0, const int *host_cg, const int *host_heads, int head_dim, float scale,
    int nq, int key_num_sample, const float *xhat, const int *num_active_dev, const int *perm, const int *q_off,
    const int *nq_valid, const int *num_rows_dev, int row_capacity, const float *qrow_meta, const int *qrow_src,
    const float *const *host_kmeta, const float *wcentre, const float *const *host_Wq, const float *const *host_bq,
    const float *const *host_Wkv, const float *const *host_bkv, const float *const *host_Wo,
    const float *const *host_bo, const float *Wpos, const float *bpos, float *qbuf, float *attn, bool kv16,
    const void *const *host_packed, const int *const *host_steps, const int *const *host_num_steps, void *stream) {
    if ((host_steps == nullptr) != (host_num_steps == nullptr)) return MSSVT_E_BADARG;
    if (!host_c0 || !host_cg || !host_heads || !xhat || !num_active_dev || !perm || !q_off || !nq_valid ||
        !num_rows_dev || !qrow_meta || !qrow_src || !host_kmeta || !wcentre || !host_Wq || !host_bq || !host_Wkv ||
        !host_bkv || !host_Wo || !host_bo || !Wpos || !bpos || !qbuf || !attn || C <= 0 || num_groups <= 0 ||
        head_dim <= 0 || nq <= 0 || key_num_sample <= 0 || row_capacity <= 0)
        return MSSVT_E_BADARG;
    // 16-byte row segments: channel offsets must be float4 aligned
    if (C & 3) return MSSVT_E_BADARG;
    if (key_num_sample > MSSVT_WAVE || (head_dim & 3)) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    bool same = num_groups <= ATTN_MAX_GROUPS;
    for (int g = 0; g < num_groups; ++g) same = same && host_cg[g] == host_cg[0];
    AttnPack pack;
    size_t qoff = 0;  // each group's region of qbuf: row_capacity x 4*ceil(heads/4)*Cg floats
    for (int g = 0; g < num_groups; ++g) {
        const int c0 = host_c0[g], Cg = host_cg[g], heads = host_heads[g];
        if (!host_kmeta[g] || !host_Wq[g] || !host_bq[g] || !host_Wkv[g] || !host_bkv[g] || !host_Wo[g] || !host_bo[g])
            return MSSVT_E_BADARG;
        if (host_steps && (!host_steps[g] || !host_num_steps[g])) return MSSVT_E_BADARG;
        if (Cg <= 0 || heads <= 0 || Cg != heads * head_dim || c0 < 0 || c0 + Cg > C || (c0 & 3)) return MSSVT_E_BADARG;
        // one channel per lane, <= 8 heads per group
        if (Cg > MSSVT_WAVE || heads > 8) return MSSVT_E_TOOLARGE;
        AttnArgs a;
        a.C = C; a.c0 = c0; a.heads = heads; a.hd = head_dim; a.scale = scale;
        a.nq = nq; a.K = key_num_sample;
        a.xhat = xhat; a.num_wins = num_active_dev; a.perm = perm; a.q_off = q_off; a.nq_valid = nq_valid;
        a.num_rows = num_rows_dev;
        a.steps = host_steps ? host_steps[g] : perm;
        a.num_steps = host_steps ? host_num_steps[g] : num_active_dev;
        a.step_stride = host_steps ? 2 : 1;
        a.qrow_meta = reinterpret_cast<const float4 *>(qrow_meta);
        a.qrow_src = reinterpret_cast<const int2 *>(qrow_src);
        a.kmeta = reinterpret_cast<const float4 *>(host_kmeta[g]);
        a.wcentre = reinterpret_cast<const float4 *>(wcentre);
        a.Wq = host_Wq[g]; a.bq = host_bq[g]; a.Wkv = host_Wkv[g]; a.bkv = host_bkv[g];
        a.Wo = host_Wo[g]; a.bo = host_bo[g]; a.Wp = Wpos; a.bp = bpos;
        a.qbuf = qbuf + qoff;
        a.attn = attn;
        a.row_capacity = row_capacity;
        a.packed = host_packed ? host_packed[g] : nullptr;
        qoff += (size_t)row_capacity * (((heads + 3) / 4) * 4) * Cg;
        if (same) {
            pack.g[g] = a;
        } else {  // unequal group widths: one launch triple per group
            if (host_steps) return MSSVT_E_TOOLARGE;
            AttnPack one;
            for (int i = 0; i < ATTN_MAX_GROUPS; ++i) one.g[i] = a;
            const int rc = dispatch_block_attn(one, 1, Cg, head_dim, row_capacity, kv16, false, st);
            if (rc) return rc;
        }
    }
    if (!same) return MSSVT_OK;
    for (int g = num_groups; g < ATTN_MAX_GROUPS; ++g) pack.g[g] = pack.g[0];
    return dispatch_block_attn(pack, num_groups, host_cg[0], head_dim, row_capacity, kv16, host_steps != nullptr, st);
}

#define ATTN_ENTRY_PARAMS                                                                                              \
    int C, int num_groups, const int *host_c0, const int *host_cg, const int *host_heads, int head_dim, float scale,   \
    int nq, int key_num_sample, const float *xhat, const int *num_active_dev, const int *perm, const int *q_off,       \
    const int *nq_valid, const int *num_rows_dev, int row_capacity, const float *qrow_meta, const int *qrow_src,       \
    const float *const *host_kmeta, const float *wcentre, const float *const *host_Wq, const float *const *host_bq,    \
    const float *const *host_Wkv, const float *const *host_bkv, const float *const *host_Wo,                           \
    const float *const *host_bo, const float *Wpos, const float *bpos, float *qbuf, float *attn, void *stream
#define ATTN_ENTRY_ARGS                                                                                                \
    C, num_groups, host_c0, host_cg, host_heads, head_dim, scale, nq, key_num_sample, xhat, num_active_dev, perm,      \
    q_off, nq_valid, num_rows_dev, row_capacity, qrow_meta, qrow_src, host_kmeta, wcentre, host_Wq, host_bq, host_Wkv, \
    host_bkv, host_Wo, host_bo, Wpos, bpos, qbuf, attn
extern "C" int mssvt_block_attention(ATTN_ENTRY_PARAMS) { return block_attention_impl(ATTN_ENTRY_ARGS, false, nullptr, nullptr, nullptr, stream); }
// launch B with split-fp16 matrix operands (k_attn_kvh) where the shape allows (Cg % 32 == 0, 16 < K <= 64), the fp32
// form otherwise; with host_packed (one mssvt_attn_pack_weights blob per group; head_dim 16) launches A and C run on the
// pre-split fragments too.  The CALLER guarantees the fp16 range of key tokens, Q', Qt, Xbar and V
extern "C" int mssvt_block_attention_kv16(
    int C, int num_groups, const int *host_c0, const int *host_cg, const int *host_heads, int head_dim, float scale,
    int nq, int key_num_sample, const float *xhat, const int *num_active_dev, const int *perm, const int *q_off,
    const int *nq_valid, const int *num_rows_dev, int row_capacity, const float *qrow_meta, const int *qrow_src,
    const float *const *host_kmeta, const float *wcentre, const float *const *host_Wq, const float *const *host_bq,
    const float *const *host_Wkv, const float *const *host_bkv, const float *const *host_Wo,
    const float *const *host_bo, const float *Wpos, const float *bpos, float *qbuf, float *attn,
    const void *const *host_packed, void *stream) {
    return block_attention_impl(ATTN_ENTRY_ARGS, true, host_packed, nullptr, nullptr, stream);
}
// mssvt_block_attention_kv16 whose window launch walks one step list per head group (mssvt_plan_order_steps): two one-tile
// windows per wavefront step.  Only the Q' hand-off form takes pairs (blobs, head_dim 16, key_num_sample <= 32, equal group
// widths): MSSVT_E_TOOLARGE for every other launch form, before anything is launched.
extern "C" int mssvt_block_attention_kv16_steps(
    int C, int num_groups, const int *host_c0, const int *host_cg, const int *host_heads, int head_dim, float scale,
    int nq, int key_num_sample, const float *xhat, const int *num_active_dev, const int *perm, const int *q_off,
    const int *nq_valid, const int *num_rows_dev, int row_capacity, const float *qrow_meta, const int *qrow_src,
    const float *const *host_kmeta, const float *wcentre, const float *const *host_Wq, const float *const *host_bq,
    const float *const *host_Wkv, const float *const *host_bkv, const float *const *host_Wo,
    const float *const *host_bo, const float *Wpos, const float *bpos, float *qbuf, float *attn,
    const void *const *host_packed, const int *const *host_steps, const int *const *host_num_steps, void *stream) {
    if (!host_packed || !host_steps || !host_num_steps) return MSSVT_E_BADARG;
    return block_attention_impl(ATTN_ENTRY_ARGS, true, host_packed, host_steps, host_num_steps, stream);
}

extern "C" long long mssvt_attn_packed_bytes(int Cg, int head_dim) {
    if (head_dim != 16) return 0;
    if (Cg == 64) return AttnBlob<64>::BYTES;
    if (Cg == 32) return AttnBlob<32>::BYTES;
    return 0;
}

extern "C" int mssvt_attn_pack_weights(int Cg, int head_dim, float scale, const float *Wq, const float *Wkv, const float *Wo,
                                       void *packed, void *stream) {
    if (!Wq || !Wkv || !Wo || !packed) return MSSVT_E_BADARG;
    if (head_dim != 16) return MSSVT_E_TOOLARGE;
    hipStream_t st = (hipStream_t)stream;
    if (Cg == 64) k_attn_pack<64><<<dim3(16, 6), MSSVT_WAVE, 0, st>>>(Wq, Wkv, Wo, scale, reinterpret_cast<char *>(packed));
    else if (Cg == 32) k_attn_pack<32><<<dim3(4, 6), MSSVT_WAVE, 0, st>>>(Wq, Wkv, Wo, scale, reinterpret_cast<char *>(packed));
    else return MSSVT_E_TOOLARGE;
    return mssvt_launch_status();
}

// cell centre in metres, one rounding per op like the reference's torch expression
// (ref: with_coords, mssvt_backbone.py:132-137)
__device__ __forceinline__ float centre_of(int idx, float cell, float lo) {
    return __fadd_rn(__fmul_rn(__fadd_rn((float)idx, 0.5f), cell), lo);
}

// ---------------------------------------------------------------------------------
// interpolation (3-NN, inverse distance) + scatter + first residual
// ---------------------------------------------------------------------------------
struct ScatterArgs {
    int C, nq, n1, interp;
    const float *attn, *x_in;
    float *x_new;
    const int *indices, *win_ind, *num_wins, *win_vstart, *q_ind, *upd_ind, *owner;
    float vsx, vsy, vsz, minx, miny, minz;
    // table mode (tab_row != null): nothing is gathered; per owned voxel the three attention
    // rows and weights are recorded so that a consumer (the fused FFN) can apply them
    int4 *tab_row;
    float4 *tab_w;
    int zero_row;  // row of `attn` that holds zeros: target of empty slots / zero weights
};

#define SC_WPB 4
#define SC_MAXQ 256
#define SC_MAX_SETS 4
struct ScatterPack {
    ScatterArgs s[SC_MAX_SETS];
};

// blockIdx.y = set: the interpolation tables of all (cbs_pattern, interp) variants of a plan in one launch
__global__ void __launch_bounds__(SC_WPB *MSSVT_WAVE) k_block_scatter(ScatterPack pack) {
    const ScatterArgs &a = pack.s[blockIdx.y];
    __shared__ float kx[SC_WPB][SC_MAXQ], ky[SC_WPB][SC_MAXQ], kz[SC_WPB][SC_MAXQ];
    __shared__ int kvalid[SC_WPB][SC_MAXQ];
    const int wv = threadIdx.x / MSSVT_WAVE, lane = lane_id();
    const int nw = *a.num_wins;
    for (int w = blockIdx.x * SC_WPB + wv; w < nw; w += gridDim.x * SC_WPB) {
        const int vstart = a.win_vstart[w];
        if (!a.interp) {  // ref mssvt_backbone.py:327-330: only the query voxels are updated
            for (int i = 0; i < a.nq; ++i) {
                const int v = a.q_ind[(size_t)w * a.nq + i];
                if (v < 0 || a.owner[vstart + v] != w * a.nq + i) continue;
                if (a.tab_row) {
                    if (lane == 0) {
                        a.tab_row[vstart + v] = make_int4(w * a.nq + i, a.zero_row, a.zero_row, 0);
                        a.tab_w[vstart + v] = make_float4(1.f, 0.f, 0.f, 0.f);
                    }
                    continue;
                }
                const float *src = a.attn + ((size_t)w * a.nq + i) * a.C;
                const size_t row = (size_t)(vstart + v) * a.C;
                for (int c = lane; c < a.C; c += MSSVT_WAVE) a.x_new[row + c] = src[c] + a.x_in[row + c];
            }
            continue;
        }
        // known points = ALL nq query slots; empty slots sit at the world origin with zero
        // features (ref :302 gathers coordinates with -1 -> 0 fill) -- kept as is
        // Candidate list for the 3-NN search, in slot order: every valid slot, and of the EMPTY slots only the
        // first three -- all empty slots are the same point (the origin), the search keeps the first seen on
        // ties (strict <), so a fourth one can never enter the best three.  ~5 candidates instead of nq.
        int ncand = 0, nempty = 0;
        for (int i0 = 0; i0 < a.nq; i0 += MSSVT_WAVE) {
            const int i = i0 + lane;
            int v = -1;
            float x = 0.f, y = 0.f, z = 0.f;
            if (i < a.nq) {
                v = a.q_ind[(size_t)w * a.nq + i];
                if (v >= 0) {
                    const int4 vi = reinterpret_cast<const int4 *>(a.indices)[vstart + v];
                    x = centre_of(vi.w, a.vsx, a.minx);
                    y = centre_of(vi.z, a.vsy, a.miny);
                    z = centre_of(vi.y, a.vsz, a.minz);
                }
            }
            const bool empty = i < a.nq && v < 0;
            const unsigned long long me = __ballot(empty);
            const bool keep = i < a.nq && (v >= 0 || nempty + __popcll(me & ((1ull << lane) - 1ull)) < 3);
            const unsigned long long mk = __ballot(keep);
            if (keep) {
                const int p = ncand + __popcll(mk & ((1ull << lane) - 1ull));
                kx[wv][p] = x; ky[wv][p] = y; kz[wv][p] = z;
                kvalid[wv][p] = (i << 1) | (v >= 0 ? 1 : 0);  // original slot, valid bit
            }
            ncand += __popcll(mk);
            nempty += __popcll(me);
        }
        wave_lds_sync();
        for (int s0 = 0; s0 < a.n1; s0 += MSSVT_WAVE) {
            const int s = s0 + lane;
            int v = -1;
            if (s < a.n1) {
                v = a.upd_ind[(size_t)w * a.n1 + s];
                if (v >= 0 && a.owner[vstart + v] != w * a.n1 + s) v = -1;  // another slot owns this voxel
            }
            int i1 = 0, i2 = 0, i3 = 0;
            float w1 = 0.f, w2 = 0.f, w3 = 0.f;
            if (v >= 0) {  // K9 (ref interpolate_gpu.cu:16-59) + weights (ref mssvt_backbone.py:305-307)
                const int4 vi = reinterpret_cast<const int4 *>(a.indices)[vstart + v];
                const float ux = centre_of(vi.w, a.vsx, a.minx), uy = centre_of(vi.z, a.vsy, a.miny),
                            uz = centre_of(vi.y, a.vsz, a.minz);
                // the reference keeps the running bests in double (initial 1e40) and compares float distances
                // against them: the same order as float compares against +inf
                float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
                int c1 = -1, c2 = -1, c3 = -1;  // candidate positions
                for (int k = 0; k < ncand; ++k) {
                    const float dx = ux - kx[wv][k], dy = uy - ky[wv][k], dz = uz - kz[wv][k];
                    const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                    if (d < b1) { b3 = b2; c3 = c2; b2 = b1; c2 = c1; b1 = d; c1 = k; }
                    else if (d < b2) { b3 = b2; c3 = c2; b2 = d; c2 = k; }
                    else if (d < b3) { b3 = d; c3 = k; }
                }
                // fewer than three candidates (nq < 3): the reference leaves index 0 / distance 1e40 -> weight ~0
                const int m1 = c1 >= 0 ? kvalid[wv][c1] : 0, m2 = c2 >= 0 ? kvalid[wv][c2] : 0,
                          m3 = c3 >= 0 ? kvalid[wv][c3] : 0;
                i1 = m1 >> 1; i2 = m2 >> 1; i3 = m3 >> 1;
                const float d1 = fmaxf(c1 >= 0 ? sqrtf(b1) : INFINITY, 1e-10f), d2 = fmaxf(c2 >= 0 ? sqrtf(b2) : INFINITY, 1e-10f),
                            d3 = fmaxf(c3 >= 0 ? sqrtf(b3) : INFINITY, 1e-10f);
                w1 = 1.0f / d1; w2 = 1.0f / d2; w3 = 1.0f / d3;
                const float norm = (w1 + w2) + w3;
                w1 /= norm; w2 /= norm; w3 /= norm;
                if (!(m1 & 1) || c1 < 0) w1 = 0.f;  // empty slots carry zero features
                if (!(m2 & 1) || c2 < 0) w2 = 0.f;
                if (!(m3 & 1) || c3 < 0) w3 = 0.f;
            }
            if (a.tab_row) {
                if (v >= 0) {
                    a.tab_row[vstart + v] = make_int4(w1 != 0.f ? w * a.nq + i1 : a.zero_row,
                                                      w2 != 0.f ? w * a.nq + i2 : a.zero_row,
                                                      w3 != 0.f ? w * a.nq + i3 : a.zero_row, 0);
                    a.tab_w[vstart + v] = make_float4(w1, w2, w3, 0.f);
                }
                continue;
            }
            unsigned long long todo = __ballot(v >= 0);
            while (todo) {  // one covered voxel at a time, lanes sweep its channels
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int vv = __shfl(v, src);
                const int j1 = __shfl(i1, src), j2 = __shfl(i2, src), j3 = __shfl(i3, src);
                const float f1 = __shfl(w1, src), f2 = __shfl(w2, src), f3 = __shfl(w3, src);
                const float *r1 = a.attn + ((size_t)w * a.nq + j1) * a.C;
                const float *r2 = a.attn + ((size_t)w * a.nq + j2) * a.C;
                const float *r3 = a.attn + ((size_t)w * a.nq + j3) * a.C;
                const size_t row = (size_t)(vstart + vv) * a.C;
                for (int c = lane; c < a.C; c += MSSVT_WAVE) {
                    float acc = 0.f;  // a zero weight never touches the (unwritten) row of an empty slot
                    if (f1 != 0.f) acc = r1[c] * f1;
                    if (f2 != 0.f) acc += r2[c] * f2;
                    if (f3 != 0.f) acc += r3[c] * f3;
                    a.x_new[row + c] = acc + a.x_in[row + c];
                }
            }
        }
        wave_lds_sync();
    }
}

extern "C" int mssvt_block_interp_scatter(int C, int nq, int n_upd, int use_interpolation,
                                          const float *attn, const float *x_in, float *x_new,
                                          const int *indices, const int *win_ind,
                                          const int *num_wins_dev, int win_capacity,
                                          const int *win_vstart, const int *q_ind,
                                          const int *upd_ind, const int *owner,
                                          const float *host_voxel_size3,
                                          const float *host_range_min3, void *stream) {
    if (!attn || !x_in || !x_new || !indices || !win_ind || !num_wins_dev || !win_vstart || !q_ind ||
        !owner || !host_voxel_size3 || !host_range_min3 || C <= 0 || nq <= 0)
        return MSSVT_E_BADARG;
    if (use_interpolation && (!upd_ind || n_upd <= 0)) return MSSVT_E_BADARG;
    if (nq > SC_MAXQ) return MSSVT_E_TOOLARGE;
    if (win_capacity <= 0) return MSSVT_OK;
    ScatterArgs a;
    a.C = C; a.nq = nq; a.n1 = n_upd; a.interp = use_interpolation;
    a.attn = attn; a.x_in = x_in; a.x_new = x_new;
    a.indices = indices; a.win_ind = win_ind; a.num_wins = num_wins_dev; a.win_vstart = win_vstart;
    a.q_ind = q_ind; a.upd_ind = upd_ind; a.owner = owner;
    a.vsx = host_voxel_size3[0]; a.vsy = host_voxel_size3[1]; a.vsz = host_voxel_size3[2];
    a.minx = host_range_min3[0]; a.miny = host_range_min3[1]; a.minz = host_range_min3[2];
    a.tab_row = nullptr; a.tab_w = nullptr; a.zero_row = 0;
    int grid = divup(win_capacity, SC_WPB);
    if (grid > 4096) grid = 4096;  // grid-stride over the windows actually present
    ScatterPack pack;
    for (int i = 0; i < SC_MAX_SETS; ++i) pack.s[i] = a;
    k_block_scatter<<<grid, SC_WPB * MSSVT_WAVE, 0, (hipStream_t)stream>>>(pack);
    return mssvt_launch_status();
}

// Table form of mssvt_block_interp_scatter: records, per voxel owned by a list slot, the
// (up to) three attention rows and inverse-distance weights instead of applying them.
extern "C" int mssvt_block_interp_table_multi(int num_sets, const int *host_nq, const int *host_n_upd,
                                              const int *host_interp, const int *indices, const int *win_ind,
                                              const int *num_wins_dev, int win_capacity, const int *win_vstart,
                                              const int *const *host_q_ind, const int *const *host_upd_ind,
                                              const int *const *host_owner, const float *host_voxel_size3,
                                              const float *host_range_min3, const int *host_zero_row,
                                              int *const *host_tab_row, float *const *host_tab_w, void *stream) {
    if (num_sets <= 0 || num_sets > SC_MAX_SETS) return num_sets <= 0 ? MSSVT_E_BADARG : MSSVT_E_TOOLARGE;
    if (!host_nq || !host_n_upd || !host_interp || !indices || !win_ind || !num_wins_dev || !win_vstart ||
        !host_q_ind || !host_upd_ind || !host_owner || !host_voxel_size3 || !host_range_min3 || !host_zero_row ||
        !host_tab_row || !host_tab_w)
        return MSSVT_E_BADARG;
    if (win_capacity <= 0) return MSSVT_OK;
    ScatterPack pack;
    for (int i = 0; i < SC_MAX_SETS; ++i) {
        const int k = i < num_sets ? i : 0;
        if (!host_q_ind[k] || !host_owner[k] || !host_tab_row[k] || !host_tab_w[k] || host_nq[k] <= 0)
            return MSSVT_E_BADARG;
        if (host_interp[k] && (!host_upd_ind[k] || host_n_upd[k] <= 0)) return MSSVT_E_BADARG;
        if (host_nq[k] > SC_MAXQ) return MSSVT_E_TOOLARGE;
        ScatterArgs &a = pack.s[i];
        a.C = 0; a.nq = host_nq[k]; a.n1 = host_n_upd[k]; a.interp = host_interp[k];
        a.attn = nullptr; a.x_in = nullptr; a.x_new = nullptr;
        a.indices = indices; a.win_ind = win_ind; a.num_wins = num_wins_dev; a.win_vstart = win_vstart;
        a.q_ind = host_q_ind[k]; a.upd_ind = host_upd_ind[k]; a.owner = host_owner[k];
        a.vsx = host_voxel_size3[0]; a.vsy = host_voxel_size3[1]; a.vsz = host_voxel_size3[2];
        a.minx = host_range_min3[0]; a.miny = host_range_min3[1]; a.minz = host_range_min3[2];
        a.tab_row = reinterpret_cast<int4 *>(host_tab_row[k]);
        a.tab_w = reinterpret_cast<float4 *>(host_tab_w[k]);
        a.zero_row = host_zero_row[k];
    }
    int grid = divup(win_capacity, SC_WPB);
    if (grid > 16384 / num_sets) grid = 16384 / num_sets;  // ~1 window per wave: the per-window chain is 3 dependent round trips
    k_block_scatter<<<dim3(grid, num_sets), SC_WPB * MSSVT_WAVE, 0, (hipStream_t)stream>>>(pack);
    return mssvt_launch_status();
}

extern "C" int mssvt_block_interp_table(int nq, int n_upd, int use_interpolation, const int *indices,
                                        const int *win_ind, const int *num_wins_dev, int win_capacity,
                                        const int *win_vstart, const int *q_ind, const int *upd_ind,
                                        const int *owner, const float *host_voxel_size3,
                                        const float *host_range_min3, int zero_row, int *tab_row,
                                        float *tab_w, void *stream) {
    return mssvt_block_interp_table_multi(1, &nq, &n_upd, &use_interpolation, indices, win_ind, num_wins_dev,
                                          win_capacity, win_vstart, &q_ind, &upd_ind, &owner, host_voxel_size3,
                                          host_range_min3, &zero_row, &tab_row, &tab_w, stream);
}
