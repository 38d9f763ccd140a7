// center_loss.hip -- CenterHead's training loss of ONE head, forward and backward, without a host synchronisation.
//
// Replaces the torch composition of CenterHead.get_loss (ref: pcdet/models/dense_heads/center_head.py:220-250 with
// FocalLossCenterNet / RegLossCenterNet, pcdet/utils/loss_utils.py:264-386): a dozen elementwise / reduce launches over the
// heat map and their autograd replay, a (B, D, H, W) concatenation of the regression maps, a gather, a scatter_add backward
// with float atomics, and a Python branch on the device scalar num_pos.
//   forward   k_cl_focal_partials : one streaming pass over logits + target heat map (16-byte loads on the aligned body,
//                                   scalar loads on the <= 3 elements before and after it); pos / neg / num_pos per thread
//                                   in double, per wave by shuffles, per workgroup through LDS, one plain store per workgroup.
//             k_cl_finish         : one workgroup: the partials in index order, hm_loss with the num_pos branch on the
//                                   device, and the regression term (one thread per (b, j, d), ordered sums).
//   backward  k_cl_focal_grad     : one streaming pass that recomputes from the logits and the targets (the forward saves no
//                                   gradient buffer) and writes every element of d_hm once.
//             k_cl_fill           : zeroes the regression gradients (one launch for all maps).
//             k_cl_reg_grad       : one workgroup per sample; the sample's cells staged in LDS; the FIRST unmasked slot of a
//                                   cell owns it and stores the sum of all its slots in ascending j.
// No float atomics: every sum has a fixed order, results are bit-identical run to run and across streams.
//
// Arithmetic.  With a = |x|, e = exp(-a): the larger of (p, 1 - p) is 1 / (1 + e) with logarithm -log1p(e), the smaller is
// e / (1 + e) with logarithm -a - log1p(e): both probabilities and both logarithms carry float32 RELATIVE accuracy at every
// x (log(1 - p) from a rounded p would lose it at either end).  The clamp of the reference acts on float32 sigmoids with the
// float32 bounds 1e-4f and (float)(1 - 1e-4); clamped elements use the constants below (folded in double on the host).
// Products and sums of the loss are double from the first operation and rounded to float once.
#include "common.hip.h"

#define CL_THREADS 256
#define CL_WAVES (CL_THREADS / MSSVT_WAVE)
#define CL_SWEEP MSSVT_CENTER_LOSS_SWEEP            // elements one workgroup covers per step of its grid-stride loop
#define CL_MAX_BLOCKS MSSVT_CENTER_LOSS_MAX_BLOCKS  // 256 CUs x 8 workgroups
#define CL_FIN_THREADS 1024
#define CL_FIN_WAVES (CL_FIN_THREADS / MSSVT_WAVE)
#define CL_FIN_UNROLL 8  // slots in flight per thread of k_cl_finish
#define CL_MAX_M MSSVT_CENTER_LOSS_MAX_OBJS
#define CL_MAX_D MSSVT_CENTER_LOSS_MAX_CODE
#define CL_MAX_MAPS 6
// out[]: hm_loss, loc_loss (f32), num_pos, num (int32 bit patterns), per_dim[D] (f32)
#define CL_OUT_HM 0
#define CL_OUT_LOC 1
#define CL_OUT_NUM_POS 2
#define CL_OUT_NUM 3
#define CL_OUT_PER_DIM 4

static_assert(CL_SWEEP == CL_THREADS * 4, "a workgroup sweeps one float4 per thread");
static_assert(CL_MAX_D == 16, "k_cl_finish gives 16 lanes to a slot");

struct ClMaps { const float *p[CL_MAX_MAPS]; int ch[CL_MAX_MAPS]; };
struct ClGrads { float *p[CL_MAX_MAPS]; int ch[CL_MAX_MAPS]; };
struct ClConst { float lo, hi, q_lo, q_hi, log_lo, log_hi, log_q_lo, log_q_hi; };

struct ClProb {
    float p, q, lp, lq;  // clamped sigmoid, 1 - p, their logarithms
    bool inside;         // the sigmoid lies inside the clamp: the gradient passes
};

__device__ __forceinline__ ClProb cl_prob(float x, const ClConst &c) {
    const float a = fabsf(x), e = expf(-a), l1 = log1pf(e);
    const float big = 1.0f / (1.0f + e), small = e * big;
    const bool neg = x < 0.f;
    ClProb r;
    r.p = neg ? small : big;
    r.q = neg ? big : small;
    r.lp = neg ? -a - l1 : -l1;
    r.lq = neg ? -l1 : -a - l1;
    r.inside = r.p >= c.lo && r.p <= c.hi;
    if (r.p < c.lo) { r.p = c.lo; r.q = c.q_lo; r.lp = c.log_lo; r.lq = c.log_q_lo; }
    else if (r.p > c.hi) { r.p = c.hi; r.q = c.q_hi; r.lp = c.log_hi; r.lq = c.log_q_hi; }
    return r;
}

__device__ __forceinline__ void cl_accum(float x, float g, const ClConst &c, double &pos, double &neg, int &npos) {
    const ClProb v = cl_prob(x, c);
    if (g == 1.f) {
        pos += (double)v.lp * ((double)v.q * (double)v.q);
        npos += 1;
    } else if (g < 1.f) {
        const double w = 1.0 - (double)g, w2 = w * w;
        neg += ((double)v.lq * ((double)v.p * (double)v.p)) * (w2 * w2);
    }
}

// d/dx of the element's term of -(pos + neg), times `scale` (= g_hm / num_pos, or g_hm without positives)
__device__ __forceinline__ float cl_grad(float x, float g, float scale, const ClConst &c) {
    const ClProb v = cl_prob(x, c);
    if (!v.inside) return 0.f;
    float t;
    if (g == 1.f) {  // (d/dp log(p) q^2) p q = q^3 - 2 q^2 p log(p): both terms >= 0
        t = v.q * v.q * v.q - 2.f * (v.q * v.q) * (v.p * v.lp);
    } else if (g < 1.f) {  // (d/dp log(q) p^2) p q = -p^3 + 2 p^2 q log(q): both terms <= 0
        const float w = 1.f - g, w2 = w * w;
        t = (2.f * (v.p * v.p) * (v.q * v.lq) - v.p * v.p * v.p) * (w2 * w2);
    } else {
        return 0.f;
    }
    return -(scale * t);
}

// elements in front of the first 16-byte boundary of `p`, at most n
static inline int cl_head(const void *p, long long n) {
    const long long h = (long long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
    return (int)(h < n ? h : n);
}

static inline int cl_grid(long long n) {
    const long long g = (n + CL_SWEEP - 1) / CL_SWEEP;
    return (int)(g < CL_MAX_BLOCKS ? g : CL_MAX_BLOCKS);
}

__device__ __forceinline__ double cl_wave_sum(double v) {
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// VEC: hm + head and gt + head are 16-byte aligned
template <bool VEC>
__global__ void __launch_bounds__(CL_THREADS) k_cl_focal_partials(const float *hm, const float *gt, int n, int head, ClConst c,
                                                                   double *partials) {
    __shared__ double sh[3][CL_WAVES];
    const int tid = threadIdx.x;
    double pos = 0.0, neg = 0.0;
    int npos = 0;
    if (VEC) {
        const int nb = (n - head) >> 2;
        const float4 *x4 = reinterpret_cast<const float4 *>(hm + head), *g4 = reinterpret_cast<const float4 *>(gt + head);
        for (long long i = (long long)blockIdx.x * CL_THREADS + tid; i < nb; i += (long long)gridDim.x * CL_THREADS) {
            const float4 x = x4[i], g = g4[i];
            cl_accum(x.x, g.x, c, pos, neg, npos);
            cl_accum(x.y, g.y, c, pos, neg, npos);
            cl_accum(x.z, g.z, c, pos, neg, npos);
            cl_accum(x.w, g.w, c, pos, neg, npos);
        }
        if (blockIdx.x == 0) {  // the <= 3 elements before and after the body
            if (tid < head) cl_accum(hm[tid], gt[tid], c, pos, neg, npos);
            const long long t = (long long)head + 4ll * nb + tid;
            if (t < n) cl_accum(hm[t], gt[t], c, pos, neg, npos);
        }
    } else {
        for (long long base = (long long)blockIdx.x * CL_SWEEP; base < n; base += (long long)gridDim.x * CL_SWEEP)
            for (int k = 0; k < 4; ++k) {
                const long long i = base + k * CL_THREADS + tid;
                if (i < n) cl_accum(hm[i], gt[i], c, pos, neg, npos);
            }
    }
    pos = cl_wave_sum(pos);
    neg = cl_wave_sum(neg);
    npos = wave_sum_i(npos);
    if (lane_id() == 0) {
        const int w = tid / MSSVT_WAVE;
        sh[0][w] = pos; sh[1][w] = neg; sh[2][w] = (double)npos;
    }
    __syncthreads();
    if (tid < 3) {
        double s = 0.0;
        for (int w = 0; w < CL_WAVES; ++w) s += sh[tid][w];
        partials[(size_t)blockIdx.x * 3 + tid] = s;
    }
}

// the map and the channel inside it of code dimension d (d < sum of ch[])
__device__ __forceinline__ void cl_locate(const int *ch, int d, int &k, int &cc) {
    k = 0; cc = d;
    while (k < CL_MAX_MAPS - 1 && cc >= ch[k]) { cc -= ch[k]; ++k; }
}

__global__ void __launch_bounds__(CL_FIN_THREADS) k_cl_finish(const double *partials, int nparts, ClMaps maps, int B, int M, int D,
                                                               int DT, long long HW, const float *target, const long long *inds,
                                                               const long long *masks, const float *cw, float loc_weight,
                                                               float *out) {
    __shared__ double sh[3][CL_FIN_WAVES];
    __shared__ double reg[CL_FIN_WAVES][CL_MAX_D];
    __shared__ int cnt[CL_FIN_WAVES];
    __shared__ double term[CL_MAX_D];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / MSSVT_WAVE;

    // ---- the heat-map term: thread t owns partials [t chunk, (t + 1) chunk), all sums in index order
    {
        const int chunk = (nparts + CL_FIN_THREADS - 1) / CL_FIN_THREADS;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int k = tid * chunk; k < (tid + 1) * chunk && k < nparts; ++k) {
            s0 += partials[(size_t)k * 3];
            s1 += partials[(size_t)k * 3 + 1];
            s2 += partials[(size_t)k * 3 + 2];
        }
        s0 = cl_wave_sum(s0); s1 = cl_wave_sum(s1); s2 = cl_wave_sum(s2);
        if (lane == 0) { sh[0][wave] = s0; sh[1][wave] = s1; sh[2][wave] = s2; }
    }

    // ---- the regression term: 16 lanes per slot, lane d of them owns code dimension d
    const int d = tid & (CL_MAX_D - 1);
    int k, cc;
    cl_locate(maps.ch, d < D ? d : 0, k, cc);
    const float *map = maps.p[k];
    const int chs = maps.ch[k];
    double acc = 0.0;
    int unmasked = 0;
    const long long slots = (long long)B * M;
    // CL_FIN_UNROLL slots per thread and step, each level of the dependent chain (mask -> index -> map / target) loaded for
    // all of them before the next one is touched: the loop is latency bound, not bandwidth bound
    constexpr int SPP = CL_FIN_THREADS / CL_MAX_D;  // slots per pass of the workgroup
    for (long long s0 = tid / CL_MAX_D; s0 < slots; s0 += (long long)SPP * CL_FIN_UNROLL) {
        long long ind[CL_FIN_UNROLL];
        bool live[CL_FIN_UNROLL];
        float pred[CL_FIN_UNROLL], tgt[CL_FIN_UNROLL];
#pragma unroll
        for (int u = 0; u < CL_FIN_UNROLL; ++u) {
            const long long s = s0 + (long long)u * SPP;
            live[u] = s < slots && masks[s] != 0;
        }
#pragma unroll
        for (int u = 0; u < CL_FIN_UNROLL; ++u) {  // a masked-out slot is not read
            ind[u] = live[u] ? inds[s0 + (long long)u * SPP] : -1;
            if (live[u] && d == 0) ++unmasked;
            // an index outside the map counts in num and is never dereferenced
            live[u] = live[u] && d < D && ind[u] >= 0 && ind[u] < HW;
        }
#pragma unroll
        for (int u = 0; u < CL_FIN_UNROLL; ++u) {
            const long long s = s0 + (long long)u * SPP;
            pred[u] = live[u] ? map[((s / M) * chs + cc) * HW + ind[u]] : 0.f;
            tgt[u] = live[u] ? target[s * DT + d] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < CL_FIN_UNROLL; ++u)
            if (live[u]) acc += fabs((double)pred[u] - (double)tgt[u]);
    }
    acc += __shfl_xor(acc, 16);
    acc += __shfl_xor(acc, 32);
    unmasked += __shfl_xor(unmasked, 16);
    unmasked += __shfl_xor(unmasked, 32);
    if (lane < CL_MAX_D) reg[wave][lane] = acc;
    if (lane == 0) cnt[wave] = unmasked;
    __syncthreads();

    int num = 0;
    for (int w = 0; w < CL_FIN_WAVES; ++w) num += cnt[w];
    if (tid < D) {
        double s = 0.0;
        for (int w = 0; w < CL_FIN_WAVES; ++w) s += reg[w][tid];
        const double per_dim = s / (double)(num > 1 ? num : 1);
        out[CL_OUT_PER_DIM + tid] = (float)per_dim;
        term[tid] = (double)cw[tid] * per_dim;
    }
    __syncthreads();
    if (tid == 0) {
        double pos = 0.0, neg = 0.0, np = 0.0, loc = 0.0;
        for (int w = 0; w < CL_FIN_WAVES; ++w) { pos += sh[0][w]; neg += sh[1][w]; np += sh[2][w]; }
        for (int j = 0; j < D; ++j) loc += term[j];
        out[CL_OUT_HM] = (float)(np > 0.0 ? -(pos + neg) / np : -neg);
        out[CL_OUT_LOC] = (float)((double)loc_weight * loc);
        out[CL_OUT_NUM_POS] = __int_as_float((int)np);
        out[CL_OUT_NUM] = __int_as_float(num);
    }
}

// VEC: hm + head, gt + head and d_hm + head are 16-byte aligned
template <bool VEC>
__global__ void __launch_bounds__(CL_THREADS) k_cl_focal_grad(const float *hm, const float *gt, int n, int head, ClConst c,
                                                               const float *out, const float *g_hm, float *d_hm) {
    const int tid = threadIdx.x;
    const int npos = __float_as_int(out[CL_OUT_NUM_POS]);
    const float g = g_hm ? *g_hm : 0.f;
    const float scale = npos > 0 ? g / (float)npos : g;
    if (VEC) {
        const int nb = (n - head) >> 2;
        const float4 *x4 = reinterpret_cast<const float4 *>(hm + head), *g4 = reinterpret_cast<const float4 *>(gt + head);
        float4 *o4 = reinterpret_cast<float4 *>(d_hm + head);
        for (long long i = (long long)blockIdx.x * CL_THREADS + tid; i < nb; i += (long long)gridDim.x * CL_THREADS) {
            const float4 x = x4[i], t = g4[i];
            o4[i] = make_float4(cl_grad(x.x, t.x, scale, c), cl_grad(x.y, t.y, scale, c), cl_grad(x.z, t.z, scale, c),
                                cl_grad(x.w, t.w, scale, c));
        }
        if (blockIdx.x == 0) {
            if (tid < head) d_hm[tid] = cl_grad(hm[tid], gt[tid], scale, c);
            const long long t = (long long)head + 4ll * nb + tid;
            if (t < n && tid < 4) d_hm[t] = cl_grad(hm[t], gt[t], scale, c);
        }
    } else {
        for (long long base = (long long)blockIdx.x * CL_SWEEP; base < n; base += (long long)gridDim.x * CL_SWEEP)
            for (int k = 0; k < 4; ++k) {
                const long long i = base + k * CL_THREADS + tid;
                if (i < n) d_hm[i] = cl_grad(hm[i], gt[i], scale, c);
            }
    }
}

// blockIdx.y = map; per_channel = B H W floats
__global__ void __launch_bounds__(CL_THREADS) k_cl_fill(ClGrads grads, long long per_channel) {
    float *p = grads.p[blockIdx.y];
    if (!p) return;
    const long long len = per_channel * grads.ch[blockIdx.y];
    long long head = (long long)(((16 - ((uintptr_t)p & 15)) & 15) >> 2);
    head = head < len ? head : len;
    const long long nb = (len - head) >> 2;
    float4 *o4 = reinterpret_cast<float4 *>(p + head);
    for (long long i = (long long)blockIdx.x * CL_THREADS + threadIdx.x; i < nb; i += (long long)gridDim.x * CL_THREADS)
        o4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) p[threadIdx.x] = 0.f;
        const long long t = head + 4 * nb + threadIdx.x;
        if (t < len) p[t] = 0.f;  // < 4 elements
    }
}

__global__ void __launch_bounds__(CL_THREADS) k_cl_reg_grad(ClMaps maps, ClGrads grads, int M, int D, int DT, long long HW,
                                                             const float *target, const long long *inds, const long long *masks,
                                                             const float *cw, float loc_weight, const float *out,
                                                             const float *g_loc) {
    __shared__ int cell[CL_MAX_M];  // the slot's cell, -1: masked out or outside the map
    __shared__ const float *src[CL_MAX_D];
    __shared__ float *dst[CL_MAX_D];
    __shared__ float coef[CL_MAX_D];
    const int tid = threadIdx.x;
    const long long b = blockIdx.x;
    for (int j = tid; j < M; j += CL_THREADS) {
        const long long s = b * M + j;
        long long ind = -1;
        if (masks[s] != 0) ind = inds[s];
        cell[j] = ind >= 0 && ind < HW ? (int)ind : -1;  // H W < 2^31
    }
    if (tid < D) {
        int k, cc;
        cl_locate(maps.ch, tid, k, cc);
        const long long off = (b * maps.ch[k] + cc) * HW;
        src[tid] = maps.p[k] + off;
        dst[tid] = grads.p[k] ? grads.p[k] + off : nullptr;
        const int num = __float_as_int(out[CL_OUT_NUM]);
        coef[tid] = ((*g_loc * loc_weight) * cw[tid]) / (float)(num > 1 ? num : 1);
    }
    __syncthreads();
    for (int j = tid; j < M; j += CL_THREADS) {
        const int c = cell[j];
        if (c < 0) continue;
        bool owner = true;
        for (int e = 0; e < j; ++e)
            if (cell[e] == c) { owner = false; break; }
        if (!owner) continue;
        float pred[CL_MAX_D];
        int sgn[CL_MAX_D];
#pragma unroll
        for (int d = 0; d < CL_MAX_D; ++d) {
            pred[d] = d < D ? src[d][c] : 0.f;
            sgn[d] = 0;
        }
        for (int e = j; e < M; ++e) {  // every slot of this cell, ascending
            if (cell[e] != c) continue;
            const float *row = target + (size_t)(b * M + e) * (size_t)DT;
#pragma unroll
            for (int d = 0; d < CL_MAX_D; ++d)
                if (d < D) {
                    const float v = pred[d] - row[d];
                    sgn[d] += (v > 0.f) - (v < 0.f);
                }
        }
#pragma unroll
        for (int d = 0; d < CL_MAX_D; ++d)
            if (d < D && dst[d]) dst[d][c] = coef[d] * (float)sgn[d];
    }
}

static ClConst cl_constants() {
    ClConst c;
    c.lo = 1e-4f;
    c.hi = (float)(1.0 - 1e-4);
    c.q_lo = (float)(1.0 - (double)c.lo);
    c.q_hi = (float)(1.0 - (double)c.hi);
    c.log_lo = (float)log((double)c.lo);
    c.log_hi = (float)log((double)c.hi);
    c.log_q_lo = (float)log(1.0 - (double)c.lo);
    c.log_q_hi = (float)log(1.0 - (double)c.hi);
    return c;
}

// 0: fine, else the status to return
static int cl_check_shape(int B, int C, int H, int W, int M, int D, int DT, long long *n_out) {
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || M <= 0 || D <= 0 || DT < D) return MSSVT_E_BADARG;
    if (M > CL_MAX_M || D > CL_MAX_D) return MSSVT_E_TOOLARGE;
    const long long lim = 0x7FFFFFFFll;
    const long long hw = (long long)H * W;  // < 2^62
    if (hw > lim || hw * C > lim || hw * C * B > lim || (long long)B * M > lim) return MSSVT_E_TOOLARGE;
    *n_out = hw * C * B;
    return 0;
}

static int cl_check_maps(const ClMaps &m, int D) {
    int sum = 0;
    for (int k = 0; k < CL_MAX_MAPS; ++k) {
        if (m.ch[k] < 0 || m.ch[k] > CL_MAX_D) return MSSVT_E_BADARG;
        if (m.ch[k] > 0 && !m.p[k]) return MSSVT_E_BADARG;
        sum += m.ch[k];
    }
    return sum == D ? 0 : MSSVT_E_BADARG;
}

extern "C" long long mssvt_center_loss_workspace_bytes(int batch_size, int num_classes, int H, int W, int num_max_objs,
                                                       int code_size) {
    long long n = 0;
    if (cl_check_shape(batch_size, num_classes, H, W, num_max_objs, code_size, code_size, &n) != 0) return 0;
    return (long long)cl_grid(n) * 3 * (long long)sizeof(double);
}

extern "C" int mssvt_center_loss_forward(int batch_size, int num_classes, int H, int W, int num_max_objs, int code_size,
                                         int target_stride, const float *hm, const float *heatmap, const float *map0, int ch0,
                                         const float *map1, int ch1, const float *map2, int ch2, const float *map3, int ch3,
                                         const float *map4, int ch4, const float *map5, int ch5, const float *target_boxes,
                                         const long long *inds, const long long *masks, const float *code_weights,
                                         float loc_weight, void *workspace, float *out, void *stream) {
    if (!hm || !heatmap || !target_boxes || !inds || !masks || !code_weights || !workspace || !out) return MSSVT_E_BADARG;
    long long n = 0;
    int st = cl_check_shape(batch_size, num_classes, H, W, num_max_objs, code_size, target_stride, &n);
    if (st != 0) return st;
    const ClMaps maps = {{map0, map1, map2, map3, map4, map5}, {ch0, ch1, ch2, ch3, ch4, ch5}};
    st = cl_check_maps(maps, code_size);
    if (st != 0) return st;
    if (((uintptr_t)workspace & 7) != 0) return MSSVT_E_BADARG;
    const ClConst c = cl_constants();
    const int grid = cl_grid(n), head = cl_head(hm, n);
    double *partials = (double *)workspace;
    hipStream_t s = (hipStream_t)stream;
    if ((((uintptr_t)hm ^ (uintptr_t)heatmap) & 15) == 0)
        k_cl_focal_partials<true><<<grid, CL_THREADS, 0, s>>>(hm, heatmap, (int)n, head, c, partials);
    else
        k_cl_focal_partials<false><<<grid, CL_THREADS, 0, s>>>(hm, heatmap, (int)n, head, c, partials);
    k_cl_finish<<<1, CL_FIN_THREADS, 0, s>>>(partials, grid, maps, batch_size, num_max_objs, code_size, target_stride,
                                             (long long)H * W, target_boxes, inds, masks, code_weights, loc_weight, out);
    return mssvt_launch_status();
}

extern "C" int mssvt_center_loss_backward(int batch_size, int num_classes, int H, int W, int num_max_objs, int code_size,
                                          int target_stride, const float *hm, const float *heatmap, const float *map0, int ch0,
                                          const float *map1, int ch1, const float *map2, int ch2, const float *map3, int ch3,
                                          const float *map4, int ch4, const float *map5, int ch5, const float *target_boxes,
                                          const long long *inds, const long long *masks, const float *code_weights,
                                          float loc_weight, const float *out, const float *g_hm, const float *g_loc,
                                          float *d_hm, float *d_map0, float *d_map1, float *d_map2, float *d_map3,
                                          float *d_map4, float *d_map5, void *stream) {
    if (!hm || !heatmap || !target_boxes || !inds || !masks || !code_weights || !out) return MSSVT_E_BADARG;
    long long n = 0;
    int st = cl_check_shape(batch_size, num_classes, H, W, num_max_objs, code_size, target_stride, &n);
    if (st != 0) return st;
    const ClMaps maps = {{map0, map1, map2, map3, map4, map5}, {ch0, ch1, ch2, ch3, ch4, ch5}};
    st = cl_check_maps(maps, code_size);
    if (st != 0) return st;
    ClGrads grads = {{d_map0, d_map1, d_map2, d_map3, d_map4, d_map5}, {ch0, ch1, ch2, ch3, ch4, ch5}};
    bool any = false;
    int max_ch = 0;
    for (int k = 0; k < CL_MAX_MAPS; ++k) {
        if (grads.ch[k] == 0) grads.p[k] = nullptr;
        if (grads.p[k]) { any = true; max_ch = grads.ch[k] > max_ch ? grads.ch[k] : max_ch; }
    }
    const ClConst c = cl_constants();
    const long long HW = (long long)H * W;
    hipStream_t s = (hipStream_t)stream;
    if (d_hm) {
        const int grid = cl_grid(n), head = cl_head(hm, n);
        if (((((uintptr_t)hm ^ (uintptr_t)heatmap) | ((uintptr_t)hm ^ (uintptr_t)d_hm)) & 15) == 0)
            k_cl_focal_grad<true><<<grid, CL_THREADS, 0, s>>>(hm, heatmap, (int)n, head, c, out, g_hm, d_hm);
        else
            k_cl_focal_grad<false><<<grid, CL_THREADS, 0, s>>>(hm, heatmap, (int)n, head, c, out, g_hm, d_hm);
    }
    if (any) {
        const long long per_channel = (long long)batch_size * HW;
        k_cl_fill<<<dim3(cl_grid(per_channel * max_ch), CL_MAX_MAPS), CL_THREADS, 0, s>>>(grads, per_channel);
        if (g_loc)  // an absent upstream gradient is zero: the fill is the whole answer
            k_cl_reg_grad<<<batch_size, CL_THREADS, 0, s>>>(maps, grads, num_max_objs, code_size, target_stride, HW,
                                                            target_boxes, inds, masks, code_weights, loc_weight, out, g_loc);
    }
    return mssvt_launch_status();
}
