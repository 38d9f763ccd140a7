// nms_bev_batched.hip -- the NMS of nms_bev.hip for a whole batch of padded candidate lists whose lengths live on the
// device: CenterHead's padded path (center_decode.hip -> here), one call per head, nothing read back.
//
// Per sample b: n = min(cand_num[b], pre_max) rows of cand_boxes[b] (already in descending score order);
//   k_nmsb_mask : grid (rows / 4, 64-column blocks, B) sized by min(K, pre_max) -- never by a device value; a wavefront
//                 owns one row i and 64 columns, one `__ballot` is the row's mask word ("j > i and IoU(i, j) > thresh").
//                 Wavefronts beyond n[b] leave at once.  Every word the walk reads is written: no clearing.
//   k_nmsb_walk : one wavefront per sample, the greedy walk of k_nms_scan (removed-bits word w in lane w, 16 mask rows in
//                 flight); a kept row goes straight to out_*[b][out_num[b] + j] with its label mapped through class_map,
//                 until post_max rows are out; out_num[b] += their number.  Heads run one after another on one stream,
//                 so each appends behind the one before it.
// The pair geometry is box_geom.hip.h's, as in nms_bev.hip.  Rotated pairs whose centres are further apart than their
// half-diagonals (+ 5 cm each, five times the in-box margin) allow cannot cross or contain a corner: their overlap is
// exactly 0 and the polygon clipping is skipped.
#include "box_geom.hip.h"

#define NMSB_MAX_N 4096  // 64 words of 64 columns: one removed-bits word per lane
#define NMSB_ROWS 4      // wavefronts (rows) per workgroup of the mask kernel

template <bool NORMAL>
__global__ void __launch_bounds__(NMSB_ROWS * MSSVT_WAVE) k_nmsb_mask(int K, int D, int n_cap, int pre_max, float thresh,
                                                                       const float *cand_boxes, const int *cand_num,
                                                                       unsigned long long *mask) {
    const int lane = lane_id(), b = blockIdx.z, cb = blockIdx.y;
    const int i = blockIdx.x * NMSB_ROWS + threadIdx.x / MSSVT_WAVE;
    const int words = (n_cap + MSSVT_WAVE - 1) / MSSVT_WAVE;
    int n = cand_num[b];
    n = n < 0 ? 0 : n;
    n = n < K ? n : K;
    n = n < pre_max ? n : pre_max;  // <= n_cap
    if (i >= n || cb * MSSVT_WAVE >= n) return;  // wave-uniform
    unsigned long long word = 0ull;
    if (cb * MSSVT_WAVE + MSSVT_WAVE - 1 > i) {  // the block holds later boxes
        const float *boxes = cand_boxes + (size_t)b * (size_t)K * (size_t)D;
        const int j = cb * MSSVT_WAVE + lane;
        const bool col_ok = j < n && j > i;
        const Box7 bi = load_box(boxes, i, D), bj = load_box(boxes, col_ok ? j : i, D);
        bool hit = false;
        if (col_ok) {
            if (NORMAL) {
                hit = iou_normal(bi, bj) > thresh;
            } else {
                const float ri = 0.5f * sqrtf(bi.dx * bi.dx + bi.dy * bi.dy) * 1.001f + 0.05f;
                const float rj = 0.5f * sqrtf(bj.dx * bj.dx + bj.dy * bj.dy) * 1.001f + 0.05f;
                const float ux = bi.x - bj.x, uy = bi.y - bj.y, reach = ri + rj;
                // (a NaN anywhere fails the comparison and takes the full procedure)
                hit = (ux * ux + uy * uy > reach * reach * 1.001f) ? 0.f > thresh : iou_bev(bi, bj) > thresh;
            }
        }
        word = __ballot(hit);
    }
    if (lane == 0) mask[((size_t)b * (size_t)n_cap + (size_t)i) * (size_t)words + cb] = word;
}

__global__ void __launch_bounds__(MSSVT_WAVE) k_nmsb_walk(int K, int D, int n_cap, int pre_max, int post_max,
                                                          const float *cand_boxes, const float *cand_scores,
                                                          const int *cand_labels, const int *cand_num,
                                                          const long long *class_map, int num_classes,
                                                          const unsigned long long *mask, int P, float *out_boxes,
                                                          float *out_scores, long long *out_labels, int *out_num) {
    const int lane = lane_id(), b = blockIdx.x;
    const int words = (n_cap + MSSVT_WAVE - 1) / MSSVT_WAVE;  // <= 64
    int n = cand_num[b];
    n = n < 0 ? 0 : n;
    n = n < K ? n : K;
    n = n < pre_max ? n : pre_max;
    int base = out_num[b];
    base = base < 0 ? 0 : (base > P ? P : base);
    const int room = post_max < P - base ? post_max : P - base;  // rows this call may write
    const int live_words = (n + MSSVT_WAVE - 1) / MSSVT_WAVE;
    const float *boxes = cand_boxes + (size_t)b * (size_t)K * (size_t)D;
    const unsigned long long *rows_of = mask + (size_t)b * (size_t)n_cap * (size_t)words;
    unsigned long long remv = 0ull;  // removed bits of columns 64 lane .. 64 lane + 63
    int cnt = 0;
    for (int i0 = 0; i0 < n && cnt < room; i0 += 16) {
        unsigned long long rows[16];
#pragma unroll
        for (int r = 0; r < 16; ++r)
            rows[r] = (i0 + r < n && lane < live_words) ? rows_of[(size_t)(i0 + r) * (size_t)words + lane] : 0ull;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + r;
            if (i >= n || cnt >= room) continue;  // wave-uniform
            const int w = i >> 6;
            const unsigned lo = __shfl((unsigned)(remv & 0xFFFFFFFFull), w);
            const unsigned hi = __shfl((unsigned)(remv >> 32), w);
            const unsigned long long word = ((unsigned long long)hi << 32) | lo;
            if (!((word >> (i & 63)) & 1ull)) {  // wave-uniform
                const size_t o = (size_t)b * (size_t)P + (size_t)(base + cnt);
                for (int q = lane; q < D; q += MSSVT_WAVE) out_boxes[o * (size_t)D + q] = boxes[(size_t)i * (size_t)D + q];
                if (lane == 0) {
                    out_scores[o] = cand_scores[(size_t)b * (size_t)K + i];
                    const int c = cand_labels[(size_t)b * (size_t)K + i];
                    out_labels[o] = (c >= 0 && c < num_classes) ? class_map[c] + 1ll : 0ll;
                }
                ++cnt;
                remv |= rows[r];
            }
        }
    }
    if (lane == 0) out_num[b] = base + cnt;
}

static bool nmsb_bad(int batch_size, int K, int row_floats, int pre_max, int post_max, int num_classes, int P) {
    return batch_size <= 0 || K <= 0 || row_floats < 7 || pre_max <= 0 || post_max <= 0 || num_classes <= 0 || P <= 0;
}

extern "C" long long mssvt_nms_bev_batched_workspace_bytes(int batch_size, int K, int pre_max) {
    if (batch_size <= 0 || K <= 0 || pre_max <= 0 || batch_size > 65535 || K > NMSB_MAX_N) return 0;
    const long long n_cap = K < pre_max ? K : pre_max;
    return (long long)batch_size * n_cap * ((n_cap + MSSVT_WAVE - 1) / MSSVT_WAVE) * 8;
}

extern "C" int mssvt_nms_bev_batched(int batch_size, int K, int row_floats, const float *cand_boxes,
                                     const float *cand_scores, const int *cand_labels, const int *cand_num,
                                     const long long *class_map, int num_classes, int pre_max, int post_max, float thresh,
                                     int normal, void *workspace, int out_rows, float *out_boxes, float *out_scores,
                                     long long *out_labels, int *out_num, void *stream) {
    if (nmsb_bad(batch_size, K, row_floats, pre_max, post_max, num_classes, out_rows)) return MSSVT_E_BADARG;
    if (!cand_boxes || !cand_scores || !cand_labels || !cand_num || !class_map || !workspace || !out_boxes || !out_scores ||
        !out_labels || !out_num)
        return MSSVT_E_BADARG;
    if (batch_size > 65535 || K > NMSB_MAX_N) return MSSVT_E_TOOLARGE;
    const int n_cap = K < pre_max ? K : pre_max;
    const dim3 grid(divup(n_cap, NMSB_ROWS), divup(n_cap, MSSVT_WAVE), batch_size);
    unsigned long long *mask = reinterpret_cast<unsigned long long *>(workspace);
    hipStream_t st = (hipStream_t)stream;
    if (normal)
        k_nmsb_mask<true><<<grid, NMSB_ROWS * MSSVT_WAVE, 0, st>>>(K, row_floats, n_cap, pre_max, thresh, cand_boxes, cand_num, mask);
    else
        k_nmsb_mask<false><<<grid, NMSB_ROWS * MSSVT_WAVE, 0, st>>>(K, row_floats, n_cap, pre_max, thresh, cand_boxes, cand_num, mask);
    k_nmsb_walk<<<batch_size, MSSVT_WAVE, 0, st>>>(K, row_floats, n_cap, pre_max, post_max, cand_boxes, cand_scores, cand_labels,
                                                   cand_num, class_map, num_classes, mask, out_rows, out_boxes, out_scores,
                                                   out_labels, out_num);
    return mssvt_launch_status();
}
