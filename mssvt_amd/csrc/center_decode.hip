// center_decode.hip -- CenterHead's inference decode for one head and the whole batch: exact top-K peaks of the heat map,
// box decode, centre-range / score filter and rank-ordered compaction, with nothing read back.
//
// Replaces, on the padded path, decode_bbox_from_heatmap (ref: pcdet/models/model_utils/centernet_utils.py:136-216:
// torch.topk over sigmoid(hm), five permute / reshape / gather chains, a boolean mask per sample).
//
// Selection: per sample the N = C H W cells are ranked by (logit descending, flat index ascending) and the first
// K' = min(K, N) are taken.  Every cell gets a UNIQUE 56-bit key
//     (order-preserving bits of the logit) << 24 | (2^24 - 1 - flat index)
// (-0.0 counts as +0.0; a NaN gets logit bits 0, below -inf, and never yields a box), so the K'-th largest key has no ties
// and a radix select finds it exactly for ANY input -- a constant map included:
//   k_cd_pass x 5 : 12-bit digit histograms of the keys that share the prefix found so far (LDS histogram per
//                   workgroup, flushed with integer atomics: the sums do not depend on arrival order).  Every workgroup of
//                   pass p first derives the digit of pass p - 1 from that pass's finished histogram (a 4096-bin scan from
//                   the top: cheaper than a launch of its own); workgroup 0 of each sample records it for pass p + 1.
//   k_cd_collect  : derives the last digit -- the K'-th key itself -- and appends every key >= it (exactly K' of them) to
//                   the sample's list through an atomic cursor: the list's ORDER is arbitrary, its content is not.
//   k_cd_decode   : one workgroup per sample sorts the list (bitonic, LDS), decodes the cells in rank order, filters and
//                   compacts the survivors in rank order, and zeroes the tails: every output element is written.
// 8 launches per head (one fill of the workspace, 5 + 1 + 1 kernels) whatever B is; no static device state (the workspace
// is the caller's, cleared here on the caller's stream), so concurrent frames on different streams do not meet.
//
// Arithmetic: one correctly rounded float32 operation per step in the order of the reference's torch expressions (no
// contraction); exp / atan2 are the device library's.
#include "common.hip.h"

#define CD_THREADS 256
#define CD_WAVES (CD_THREADS / MSSVT_WAVE)
#define CD_ITEMS 16
#define CD_BLOCK_CELLS (CD_THREADS * CD_ITEMS)  // cells per workgroup of a select pass
#define CD_BITS 12
#define CD_BINS (1 << CD_BITS)
#define CD_PASSES 5                             // 5 x 12 = 60 bits >= 56 (the key is shifted left by 4)
#define CD_MAX_K MSSVT_CENTER_DECODE_MAX_K
#define CD_MAX_CELLS (1 << 24)

typedef unsigned long long cd_key_t;

struct CdState {  // after a pass: the digits found so far and the rank still to find among the keys that share them
    cd_key_t prefix;
    unsigned int k, pad;
};

struct CdLayout {  // byte offsets into the workspace
    size_t hist, state, cursor, sel, total;
};

static CdLayout cd_layout(long long B, long long K) {
    CdLayout l;
    l.hist = 0;
    l.state = l.hist + (size_t)B * CD_PASSES * CD_BINS * sizeof(unsigned int);
    l.cursor = l.state + (size_t)B * CD_PASSES * sizeof(CdState);
    l.sel = l.cursor + (((size_t)B * sizeof(unsigned int) + 15) & ~(size_t)15);
    l.total = l.sel + (size_t)B * (size_t)K * sizeof(cd_key_t);
    return l;
}

// the 60-bit ranking key of cell `idx` (< 2^24 - 1) with logit l
__device__ __forceinline__ cd_key_t cd_key(float l, unsigned int idx) {
    unsigned int ord = 0u;  // NaN: below everything
    if (l == l) {
        const unsigned int u = l == 0.f ? 0u : __float_as_uint(l);  // -0.0 and +0.0 compare equal: the index decides
        ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);          // >= 0x007FFFFF (-inf)
    }
    return (((cd_key_t)ord << 24) | (cd_key_t)(0xFFFFFFu - idx)) << 4;
}

// The digit of one finished pass: walks `hist` (CD_BINS counts, global) from the top bin down to the bin that holds the
// k-th key.  All CD_THREADS threads call it; returns the extended prefix and the rank inside that bin (both uniform).
// 1 <= k <= sum(hist) by construction (K' <= N and every pass keeps k inside its bin).
__device__ __forceinline__ void cd_next_digit(const unsigned int *hist, cd_key_t &prefix, unsigned int &k,
                                              unsigned int *scan, unsigned int *res) {
    const int tid = threadIdx.x;
    // thread t owns the t-th group of 16 bins from the top
    const unsigned int *g = hist + (CD_BINS - 16 * (tid + 1));
    unsigned int c[16], s = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 v = *reinterpret_cast<const uint4 *>(g + 4 * q);
        c[4 * q] = v.x; c[4 * q + 1] = v.y; c[4 * q + 2] = v.z; c[4 * q + 3] = v.w;
        s += v.x + v.y + v.z + v.w;
    }
    scan[tid] = s;
    if (tid == 0) { res[0] = 0u; res[1] = 1u; }
    __syncthreads();
    for (int off = 1; off < CD_THREADS; off <<= 1) {
        const unsigned int v = tid >= off ? scan[tid - off] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const unsigned int incl = scan[tid], excl = incl - s;
    if (excl < k && k <= incl) {  // exactly one thread
        unsigned int acc = excl;
#pragma unroll
        for (int q = 15; q >= 0; --q) {
            if (acc < k && k <= acc + c[q]) {
                res[0] = (unsigned int)(CD_BINS - 16 * (tid + 1) + q);
                res[1] = k - acc;
            }
            acc += c[q];
        }
    }
    __syncthreads();
    prefix = (prefix << CD_BITS) | (cd_key_t)res[0];
    k = res[1];
    __syncthreads();  // scan / res may be reused
}

// the state before pass `pass` (1..CD_PASSES; CD_PASSES = the collect launch): state after pass - 2 plus the histogram
// of pass - 1; workgroup 0 of the sample records it
__device__ __forceinline__ void cd_enter_pass(int pass, int b, unsigned int k_first, const unsigned int *hist,
                                              CdState *state, cd_key_t &prefix, unsigned int &k, unsigned int *scan,
                                              unsigned int *res) {
    prefix = 0ull;
    k = k_first;
    if (pass == 0) return;
    if (pass > 1) {
        const CdState st = state[(size_t)b * CD_PASSES + (pass - 2)];
        prefix = st.prefix;
        k = st.k;
    }
    cd_next_digit(hist + ((size_t)b * CD_PASSES + (pass - 1)) * CD_BINS, prefix, k, scan, res);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        CdState st;
        st.prefix = prefix; st.k = k; st.pad = 0u;
        state[(size_t)b * CD_PASSES + (pass - 1)] = st;
    }
}

// grid (ceil(N / CD_BLOCK_CELLS), B)
__global__ void __launch_bounds__(CD_THREADS) k_cd_pass(int pass, int N, unsigned int k_first, const float *hm,
                                                         unsigned int *hist, CdState *state) {
    __shared__ unsigned int h[CD_BINS];
    __shared__ unsigned int scan[CD_THREADS];
    __shared__ unsigned int res[2];
    const int tid = threadIdx.x, b = blockIdx.y;
    for (int i = tid; i < CD_BINS; i += CD_THREADS) h[i] = 0u;
    cd_key_t prefix;
    unsigned int k;
    cd_enter_pass(pass, b, k_first, hist, state, prefix, k, scan, res);
    __syncthreads();
    const int shift = CD_BITS * (CD_PASSES - 1 - pass);
    const float *src = hm + (size_t)b * (size_t)N;
    const long long base = (long long)blockIdx.x * CD_BLOCK_CELLS;
#pragma unroll 4
    for (int it = 0; it < CD_ITEMS; ++it) {
        const long long i = base + it * CD_THREADS + tid;
        if (i < N) {
            const cd_key_t key = cd_key(src[i], (unsigned int)i);
            if ((key >> (shift + CD_BITS)) == prefix) atomicAdd(&h[(unsigned int)(key >> shift) & (CD_BINS - 1)], 1u);
        }
    }
    __syncthreads();
    unsigned int *dst = hist + ((size_t)b * CD_PASSES + pass) * CD_BINS;
    for (int i = tid; i < CD_BINS; i += CD_THREADS)
        if (h[i]) atomicAdd(dst + i, h[i]);
}

// grid (ceil(N / CD_BLOCK_CELLS), B): every key >= the K'-th key goes to sel[b] (exactly K' keys, any order)
__global__ void __launch_bounds__(CD_THREADS) k_cd_collect(int N, int K, unsigned int k_first, const float *hm,
                                                            const unsigned int *hist, CdState *state, unsigned int *cursor,
                                                            cd_key_t *sel) {
    __shared__ unsigned int scan[CD_THREADS];
    __shared__ unsigned int res[2];
    const int tid = threadIdx.x, b = blockIdx.y;
    cd_key_t kth;
    unsigned int k;
    cd_enter_pass(CD_PASSES, b, k_first, hist, state, kth, k, scan, res);
    const float *src = hm + (size_t)b * (size_t)N;
    const long long base = (long long)blockIdx.x * CD_BLOCK_CELLS;
    for (int it = 0; it < CD_ITEMS; ++it) {
        const long long i = base + it * CD_THREADS + tid;
        if (i < N) {
            const cd_key_t key = cd_key(src[i], (unsigned int)i);
            if (key >= kth) {
                const unsigned int pos = atomicAdd(cursor + b, 1u);
                if (pos < (unsigned int)K) sel[(size_t)b * (size_t)K + pos] = key;  // always: the keys are unique
            }
        }
    }
}

struct CdParams {
    int C, H, W, V, K, has_thresh;
    float stride, voxel_x, voxel_y, x_min, y_min, thresh;
    float lim[6];
};

// grid (B): sort, decode, filter, compact
__global__ void __launch_bounds__(CD_THREADS) k_cd_decode(CdParams p, const float *hm, const float *center,
                                                           const float *center_z, const float *dim, const float *rot,
                                                           const float *vel, const unsigned int *cursor, const cd_key_t *sel,
                                                           float *cand_boxes, float *cand_scores, int *cand_labels,
                                                           int *cand_num) {
#pragma clang fp contract(off)
    __shared__ cd_key_t keys[CD_MAX_K];
    __shared__ int wave_count[2][CD_WAVES];
    const int tid = threadIdx.x, lane = lane_id(), wave = tid / MSSVT_WAVE, b = blockIdx.x;
    const int HW = p.H * p.W, N = p.C * HW, D = 7 + p.V;
    const int want = p.K < N ? p.K : N;
    const int have = (int)min(cursor[b], (unsigned int)want);  // = want
    int n2 = 1;
    while (n2 < have) n2 <<= 1;  // <= CD_MAX_K (a power of two)
    for (int i = tid; i < n2; i += CD_THREADS) keys[i] = i < have ? sel[(size_t)b * (size_t)p.K + i] : 0ull;  // 0 < every key
    __syncthreads();
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += CD_THREADS) {
                const int o = i ^ j;
                if (o > i) {
                    const cd_key_t a = keys[i], c = keys[o];
                    if ((i & k) == 0 ? a < c : a > c) { keys[i] = c; keys[o] = a; }  // descending overall
                }
            }
            __syncthreads();
        }

    float *boxes = cand_boxes + (size_t)b * (size_t)p.K * (size_t)D;
    float *scores = cand_scores + (size_t)b * (size_t)p.K;
    int *labels = cand_labels + (size_t)b * (size_t)p.K;
    const size_t hw = (size_t)HW;
    int running = 0;  // survivors before this chunk (uniform)
    for (int chunk = 0, par = 0; chunk < have; chunk += CD_THREADS, par ^= 1) {
        const int r = chunk + tid;
        bool ok = false;
        float row[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, score = 0.f;
        int cls = 0;
        size_t cell = 0;
        if (r < have) {
            const cd_key_t key = keys[r];
            const unsigned int idx = 0xFFFFFFu - (unsigned int)((key >> 4) & 0xFFFFFFull);
            if ((key >> 28) != 0ull && idx < (unsigned int)N) {  // not a NaN logit
                cls = (int)(idx / (unsigned int)HW);
                cell = (size_t)(idx % (unsigned int)HW);
                const int y = (int)(cell / (size_t)p.W), x = (int)(cell % (size_t)p.W);
                const float l = hm[(size_t)b * (size_t)N + idx];
                score = 1.0f / (1.0f + expf(-l));
                const float *ctr = center + (size_t)b * 2 * hw + cell;
                row[0] = (((float)x + ctr[0]) * p.stride) * p.voxel_x + p.x_min;
                row[1] = (((float)y + ctr[hw]) * p.stride) * p.voxel_y + p.y_min;
                row[2] = center_z[(size_t)b * hw + cell];
                const float *dm = dim + (size_t)b * 3 * hw + cell;
                row[3] = expf(dm[0]);
                row[4] = expf(dm[hw]);
                row[5] = expf(dm[2 * hw]);
                const float *rt = rot + (size_t)b * 2 * hw + cell;
                row[6] = atan2f(rt[hw], rt[0]);
                ok = row[0] >= p.lim[0] && row[1] >= p.lim[1] && row[2] >= p.lim[2] && row[0] <= p.lim[3] &&
                     row[1] <= p.lim[4] && row[2] <= p.lim[5] && (!p.has_thresh || score > p.thresh);
            }
        }
        const unsigned long long m = __ballot(ok);
        const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0) wave_count[par][wave] = __popcll(m);
        __syncthreads();  // the other parity's readers passed this barrier one chunk ago
        int slot = running + before, total = 0;
        for (int w = 0; w < CD_WAVES; ++w) {
            const int c = wave_count[par][w];
            slot += w < wave ? c : 0;
            total += c;
        }
        running += total;
        if (ok) {  // slot < have <= K
            float *o = boxes + (size_t)slot * (size_t)D;
#pragma unroll
            for (int q = 0; q < 7; ++q) o[q] = row[q];
            for (int q = 0; q < p.V; ++q) o[7 + q] = vel[((size_t)b * p.V + q) * hw + cell];
            scores[slot] = score;
            labels[slot] = cls;
        }
    }
    for (int s = running + tid; s < p.K; s += CD_THREADS) {  // the tails
        float *o = boxes + (size_t)s * (size_t)D;
        for (int q = 0; q < D; ++q) o[q] = 0.f;
        scores[s] = 0.f;
        labels[s] = 0;
    }
    if (tid == 0) cand_num[b] = running;
}

static bool cd_too_large(long long B, long long C, long long H, long long W, long long K) {
    return B > 65535 || C > 255 || H > CD_MAX_CELLS || W > CD_MAX_CELLS || H * W >= CD_MAX_CELLS ||
           C * H * W >= CD_MAX_CELLS || K > CD_MAX_K;
}

extern "C" long long mssvt_center_decode_workspace_bytes(int batch_size, int num_classes, int H, int W, int K) {
    if (batch_size <= 0 || num_classes <= 0 || H <= 0 || W <= 0 || K <= 0) return 0;
    if (cd_too_large(batch_size, num_classes, H, W, K)) return 0;
    return (long long)cd_layout(batch_size, K).total;
}

extern "C" int mssvt_center_decode(int batch_size, int num_classes, int H, int W, int num_vel, const float *hm,
                                   const float *center, const float *center_z, const float *dim, const float *rot,
                                   const float *vel, int K, float stride, float voxel_x, float voxel_y, float x_min,
                                   float y_min, float limit_x_min, float limit_y_min, float limit_z_min, float limit_x_max,
                                   float limit_y_max, float limit_z_max, int has_score_thresh, float score_thresh,
                                   void *workspace, float *cand_boxes, float *cand_scores, int *cand_labels, int *cand_num,
                                   void *stream) {
    if (batch_size <= 0 || num_classes <= 0 || H <= 0 || W <= 0 || K <= 0 || num_vel < 0) return MSSVT_E_BADARG;
    if (!hm || !center || !center_z || !dim || !rot || (num_vel > 0 && !vel) || !workspace || !cand_boxes || !cand_scores ||
        !cand_labels || !cand_num)
        return MSSVT_E_BADARG;
    if (cd_too_large(batch_size, num_classes, H, W, K) || num_vel > 64) return MSSVT_E_TOOLARGE;
    const int N = num_classes * H * W;
    const CdLayout lay = cd_layout(batch_size, K);
    char *ws = reinterpret_cast<char *>(workspace);
    unsigned int *hist = reinterpret_cast<unsigned int *>(ws + lay.hist);
    CdState *state = reinterpret_cast<CdState *>(ws + lay.state);
    unsigned int *cursor = reinterpret_cast<unsigned int *>(ws + lay.cursor);
    cd_key_t *sel = reinterpret_cast<cd_key_t *>(ws + lay.sel);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(workspace, 0, lay.total, st);
    if (e != hipSuccess) return (int)e;
    const unsigned int k_first = (unsigned int)(K < N ? K : N);
    const dim3 grid(divup(N, CD_BLOCK_CELLS), batch_size);
    for (int pass = 0; pass < CD_PASSES; ++pass)
        k_cd_pass<<<grid, CD_THREADS, 0, st>>>(pass, N, k_first, hm, hist, state);
    k_cd_collect<<<grid, CD_THREADS, 0, st>>>(N, K, k_first, hm, hist, state, cursor, sel);
    CdParams p;
    p.C = num_classes; p.H = H; p.W = W; p.V = num_vel; p.K = K; p.has_thresh = has_score_thresh ? 1 : 0;
    p.stride = stride; p.voxel_x = voxel_x; p.voxel_y = voxel_y; p.x_min = x_min; p.y_min = y_min; p.thresh = score_thresh;
    p.lim[0] = limit_x_min; p.lim[1] = limit_y_min; p.lim[2] = limit_z_min;
    p.lim[3] = limit_x_max; p.lim[4] = limit_y_max; p.lim[5] = limit_z_max;
    k_cd_decode<<<batch_size, CD_THREADS, 0, st>>>(p, hm, center, center_z, dim, rot, vel, cursor, sel, cand_boxes,
                                                   cand_scores, cand_labels, cand_num);
    return mssvt_launch_status();
}
