// box_iou.hip -- pairwise box measures: the (num_a, num_b) matrices behind boxes_iou_bev / boxes_iou3d_gpu of
// iou3d_nms_utils (recall bookkeeping of the detector, target assigners).
//
// Replaces boxes_overlap_kernel / boxes_iou_bev_kernel (ref: pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu:236-265, one
// thread per pair in 16 x 16 tiles) and, for the 3-D IoU, the torch composition around the overlap kernel
// (iou3d_nms_utils.py:48-81: one kernel, ~12 elementwise launches, six (N, M) temporaries) with ONE launch:
//   k_box_pairs<MODE> : lane = column j (the b-box stays in registers for the whole row loop), the row loop over a tile of
//                       a-boxes is wave-uniform (the a-box is read once per wave, through the scalar cache), each row's
//                       results leave as one coalesced 256-byte store.  Every element of `out` is written, once.
// Exact rejection (modes 0-2): the reference procedure finds a point of the intersection polygon only from an edge crossing
// or from a corner of one box within the other box grown by the 1e-2 margin.  Both need a point of one rectangle within
// 1e-2 * sqrt(2) of the other, i.e. a centre distance <= half-diagonal(a) + half-diagonal(b) + 0.0142 (+ fp32 rounding of
// the corners, ~1e-5 at 75 m).  Beyond half-diagonals + 2 * BOX_SLACK the procedure therefore returns exactly 0.0f, which
// is the overlap a rejected pair is given without running it; the survivors are compacted so that it runs with full lanes.
#include "box_geom.hip.h"

#define BOX_SLACK 0.02f     // per box, metres
#define BOX_ROWS_PER_WAVE 16  // sized for sparse survivors (anchor-scale calls); a 500 x 200 call is 32 workgroups: DESIGN.md 4
#define BOX_WAVES 4         // per workgroup: a workgroup covers 64 rows x 64 columns

// the torch composition of iou3d_nms_utils.py:59-79 around the BEV overlap, rounding for rounding: every product and sum
// rounded on its own (no fused multiply-add), the operands in its order.  (The whole library is compiled with
// -ffp-contract=off, mssvt_amd/build.py, so nothing in this file is contracted; the pragma keeps this function so under any flags.)
__device__ __forceinline__ float iou3d_value(const Box7 &a, const Box7 &b, float ov) {
#pragma clang fp contract(off)
    const float a_max = a.z + a.dz / 2, a_min = a.z - a.dz / 2;
    const float b_max = b.z + b.dz / 2, b_min = b.z - b.dz / 2;
    const float h = fmaxf(fminf(a_max, b_max) - fmaxf(a_min, b_min), 0.f);
    const float ov3 = ov * h;
    const float va = a.dx * a.dy * a.dz, vb = b.dx * b.dy * b.dz;
    return ov3 / fmaxf(va + vb - ov3, 1e-6f);
}

// the measure of a pair from the overlap area of its rectangles (modes 0 - 2)
template <int MODE>
__device__ __forceinline__ float pair_value(const Box7 &a, const Box7 &b, float ov) {
    if (MODE == MSSVT_BOX_OVERLAP_BEV) return ov;
    if (MODE == MSSVT_BOX_IOU_3D) return iou3d_value(a, b, ov);
    const float sa = a.dx * a.dy, sb = b.dx * b.dy;
    return ov / fmaxf(sa + sb - ov, NMS_EPS);
}

// A wavefront owns BOX_ROWS_PER_WAVE rows x 64 columns.  Pass 1 (lane = column, wave-uniform row loop): the rejection test;
// a rejected pair's value (overlap 0) leaves with the row's coalesced store, a surviving pair is appended to the wave's queue
// in LDS (`__ballot` + prefix popcount: row-major order).  Pass 2: the queue 64 pairs at a time, one pair per lane, so that
// rect_overlap -- ~150 VGPRs, 208 B of scratch, data-dependent loops -- runs with full lanes however sparse the survivors
// are (an anchor-scale call keeps 0.15 % of its pairs: one lane in 9 % of the rows).
template <int MODE>
__global__ void __launch_bounds__(MSSVT_WAVE *BOX_WAVES) k_box_pairs(int num_a, const float *boxes_a, int stride_a, int num_b,
                                                                      const float *boxes_b, int stride_b, float *out) {
    __shared__ unsigned short queue_all[BOX_WAVES][BOX_ROWS_PER_WAVE * MSSVT_WAVE];
    const int lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / MSSVT_WAVE);
    unsigned short *queue = queue_all[wave];
    const int j0 = blockIdx.x * MSSVT_WAVE, j = j0 + lane;
    const bool col_ok = j < num_b;
    const Box7 bj = load_box(boxes_b, col_ok ? j : 0, stride_b);
    const float reach_b = 0.5f * sqrtf(bj.dx * bj.dx + bj.dy * bj.dy) + BOX_SLACK;
    constexpr int TILE = BOX_ROWS_PER_WAVE * BOX_WAVES;
    // 64-bit row index: gridDim.y is capped by the launcher, the tiles beyond it are taken in further rounds
    for (long long r0 = (long long)blockIdx.y * TILE + wave * BOX_ROWS_PER_WAVE; r0 < num_a; r0 += (long long)gridDim.y * TILE) {
        const int r_begin = (int)r0, r_end = (int)min((long long)num_a, r0 + BOX_ROWS_PER_WAVE);
        int queued = 0;  // wave-uniform
        for (int i = r_begin; i < r_end; ++i) {
            const Box7 ai = load_box(boxes_a, i, stride_a);
            bool near = false;
            if (MODE != MSSVT_BOX_IOU_NORMAL) {
                const float reach = 0.5f * sqrtf(ai.dx * ai.dx + ai.dy * ai.dy) + BOX_SLACK + reach_b;
                const float ddx = ai.x - bj.x, ddy = ai.y - bj.y;
                near = col_ok && !(ddx * ddx + ddy * ddy > reach * reach);  // NaN boxes take the full procedure
                const unsigned long long m = __ballot(near);
                if (near)
                    queue[queued + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] =
                        (unsigned short)(((i - r_begin) << 6) | lane);
                queued += __popcll(m);
            }
            if (col_ok && !near)
                out[(size_t)i * (size_t)num_b + (size_t)j] = MODE == MSSVT_BOX_IOU_NORMAL ? iou_normal(ai, bj) : pair_value<MODE>(ai, bj, 0.f);
        }
        if (MODE != MSSVT_BOX_IOU_NORMAL) {
            wave_lds_sync();
            for (int q0 = 0; q0 < queued; q0 += MSSVT_WAVE) {
                if (q0 + lane < queued) {  // entries < BOX_ROWS_PER_WAVE * 64: rows and columns this pass found in range
                    const int e = queue[q0 + lane];
                    const int i = r_begin + (e >> 6), jj = j0 + (e & 63);
                    const Box7 a = load_box(boxes_a, i, stride_a), b = load_box(boxes_b, jj, stride_b);
                    out[(size_t)i * (size_t)num_b + (size_t)jj] = pair_value<MODE>(a, b, rect_overlap(a, b));
                }
            }
            wave_lds_sync();  // the next round refills the queue
        }
    }
}

template <int MODE>
static void box_pairs_launch(int num_a, const float *boxes_a, int stride_a, int num_b, const float *boxes_b, int stride_b,
                             float *out, hipStream_t st) {
    const int tiles = divup(num_a, BOX_ROWS_PER_WAVE * BOX_WAVES);
    const dim3 grid(divup(num_b, MSSVT_WAVE), tiles < 65535 ? tiles : 65535);
    k_box_pairs<MODE><<<grid, MSSVT_WAVE * BOX_WAVES, 0, st>>>(num_a, boxes_a, stride_a, num_b, boxes_b, stride_b, out);
}

extern "C" int mssvt_boxes_pairwise(int mode, int num_a, const float *boxes_a, int stride_a, int num_b, const float *boxes_b,
                                    int stride_b, float *out, void *stream) {
    if (mode < MSSVT_BOX_OVERLAP_BEV || mode > MSSVT_BOX_IOU_NORMAL || num_a < 0 || num_b < 0 || stride_a < 7 || stride_b < 7)
        return MSSVT_E_BADARG;
    if ((num_a > 0 && !boxes_a) || (num_b > 0 && !boxes_b)) return MSSVT_E_BADARG;
    if (num_a == 0 || num_b == 0) return MSSVT_OK;
    if (!out) return MSSVT_E_BADARG;
    if (num_b > 0x7FFFFFFF - MSSVT_WAVE) return MSSVT_E_TOOLARGE;  // the column index of the last tile stays an int
    hipStream_t st = (hipStream_t)stream;
    switch (mode) {
    case MSSVT_BOX_OVERLAP_BEV: box_pairs_launch<MSSVT_BOX_OVERLAP_BEV>(num_a, boxes_a, stride_a, num_b, boxes_b, stride_b, out, st); break;
    case MSSVT_BOX_IOU_BEV: box_pairs_launch<MSSVT_BOX_IOU_BEV>(num_a, boxes_a, stride_a, num_b, boxes_b, stride_b, out, st); break;
    case MSSVT_BOX_IOU_3D: box_pairs_launch<MSSVT_BOX_IOU_3D>(num_a, boxes_a, stride_a, num_b, boxes_b, stride_b, out, st); break;
    default: box_pairs_launch<MSSVT_BOX_IOU_NORMAL>(num_a, boxes_a, stride_a, num_b, boxes_b, stride_b, out, st); break;
    }
    return mssvt_launch_status();
}
