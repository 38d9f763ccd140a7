// nms_bev.hip -- rotated bird's-eye-view NMS behind CenterHead's post-processing.
//
// Replaces iou3d_nms_cuda.nms_gpu (ref: pcdet/ops/iou3d_nms/src/iou3d_nms.cpp:90-135 + iou3d_nms_kernel.cu:236-278):
// the reference computes a suppression bit matrix on the GPU (one THREAD per row and 64-column block, a serial loop over
// the 64 columns), copies it to the host and walks it on the CPU.  Here
//   k_nms_mask : one WAVEFRONT per (64-row block, 64-column block); lane = column, the row loop is wave-uniform, so one
//                `__ballot` IS the 64-bit mask word of a row -- no per-thread bit assembly;
//   k_nms_scan : the greedy walk on the device (one wavefront, the removed-bits words live in its lanes, 16 mask rows
//                in flight at a time); only the kept indices and their count are read back.
// The pair geometry (rect_overlap / iou_bev, the reference's procedure, and the axis-aligned iou_normal) lives in
// box_geom.hip.h, shared with box_iou.hip; a box suppresses LATER boxes with IoU > thresh (strict).  mssvt_nms_normal is
// the same two kernels over iou_normal (ref nms_normal_kernel, iou3d_nms_kernel.cu:328-372; iou3d_nms.cpp:138-188).
#include "box_geom.hip.h"

// grid (column blocks, row blocks), one wavefront each; mask (n, col_blocks) words; NORMAL: the axis-aligned measure
template <bool NORMAL>
__global__ void __launch_bounds__(MSSVT_WAVE) k_nms_mask(int n, float thresh, const float *boxes, unsigned long long *mask) {
    const int cb = blockIdx.x, rb = blockIdx.y, lane = lane_id();
    const int col_blocks = gridDim.x;
    const int j = cb * MSSVT_WAVE + lane;
    const bool col_ok = j < n;
    const Box7 bj = load_box(boxes, col_ok ? j : 0);
    const int r_end = min(n, (rb + 1) * MSSVT_WAVE);
    for (int i = rb * MSSVT_WAVE; i < r_end; ++i) {
        unsigned long long word = 0ull;
        if (cb >= rb) {  // only later boxes can be suppressed (blocks left of the diagonal stay empty)
            const Box7 bi = load_box(boxes, i);
            const bool hit = col_ok && j > i && (NORMAL ? iou_normal(bi, bj) : iou_bev(bi, bj)) > thresh;
            word = __ballot(hit);
        }
        if (lane == 0) mask[(size_t)i * col_blocks + cb] = word;
    }
}

// one wavefront; lane l owns the removed-bits words l, l + 64, ... (NMS_WPL per lane)
#define NMS_WPL 4
__global__ void __launch_bounds__(MSSVT_WAVE) k_nms_scan(int n, int col_blocks, const unsigned long long *mask, int *keep,
                                                         int *num_keep) {
    const int lane = lane_id();
    unsigned long long remv[NMS_WPL];
#pragma unroll
    for (int k = 0; k < NMS_WPL; ++k) remv[k] = 0ull;
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += 16) {
        // the mask rows of the next 16 boxes travel together (they do not depend on the decisions)
        unsigned long long rows[16][NMS_WPL];
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int k = 0; k < NMS_WPL; ++k) {
                const int w = lane + MSSVT_WAVE * k;
                rows[r][k] = (i0 + r < n && w < col_blocks) ? mask[(size_t)(i0 + r) * col_blocks + w] : 0ull;
            }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = i0 + r;
            if (i >= n) continue;
            const int w = i >> 6;  // word of box i: lane w % 64, register w / 64
            unsigned long long mine = 0ull;
#pragma unroll
            for (int k = 0; k < NMS_WPL; ++k) mine = (w / MSSVT_WAVE) == k ? remv[k] : mine;
            const unsigned lo = __shfl((unsigned)(mine & 0xFFFFFFFFull), w % MSSVT_WAVE);
            const unsigned hi = __shfl((unsigned)(mine >> 32), w % MSSVT_WAVE);
            const unsigned long long word = ((unsigned long long)hi << 32) | lo;
            if (!((word >> (i & 63)) & 1ull)) {  // wave-uniform
                if (lane == 0) keep[cnt] = i;
                ++cnt;
#pragma unroll
                for (int k = 0; k < NMS_WPL; ++k) remv[k] |= rows[r][k];
            }
        }
    }
    if (lane == 0) *num_keep = cnt;
}

extern "C" long long mssvt_nms_workspace_bytes(int num_boxes) {
    const long long cbk = (num_boxes + MSSVT_WAVE - 1) / MSSVT_WAVE;
    return (long long)num_boxes * cbk * 8;
}

template <bool NORMAL>
static int nms_launch(int num_boxes, const float *boxes_sorted, float thresh, void *workspace, int *keep, int *num_keep_dev,
                      void *stream) {
    if (num_boxes < 0 || !keep || !num_keep_dev) return MSSVT_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (num_boxes == 0) return (int)hipMemsetAsync(num_keep_dev, 0, sizeof(int), st);
    if (!boxes_sorted || !workspace) return MSSVT_E_BADARG;
    const int cbk = divup(num_boxes, MSSVT_WAVE);
    if (cbk > MSSVT_WAVE * NMS_WPL) return MSSVT_E_TOOLARGE;  // 16384 boxes
    unsigned long long *mask = reinterpret_cast<unsigned long long *>(workspace);
    k_nms_mask<NORMAL><<<dim3(cbk, cbk), MSSVT_WAVE, 0, st>>>(num_boxes, thresh, boxes_sorted, mask);
    k_nms_scan<<<1, MSSVT_WAVE, 0, st>>>(num_boxes, cbk, mask, keep, num_keep_dev);
    return mssvt_launch_status();
}

extern "C" int mssvt_nms_bev(int num_boxes, const float *boxes_sorted, float thresh, void *workspace, int *keep,
                             int *num_keep_dev, void *stream) {
    return nms_launch<false>(num_boxes, boxes_sorted, thresh, workspace, keep, num_keep_dev, stream);
}

extern "C" int mssvt_nms_normal(int num_boxes, const float *boxes_sorted, float thresh, void *workspace, int *keep,
                                int *num_keep_dev, void *stream) {
    return nms_launch<true>(num_boxes, boxes_sorted, thresh, workspace, keep, num_keep_dev, stream);
}
