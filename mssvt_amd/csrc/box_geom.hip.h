// box_geom.hip.h -- geometry of two boxes in the bird's-eye view, shared by nms_bev.hip (suppression bit matrix) and
// box_iou.hip (pairwise overlap / IoU matrices).
//
// The overlap of two rotated rectangles follows the reference's procedure (pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu)
// so that the same boxes are kept and the same pairs count as overlapping: edge crossings (bounding-box pre-test, strict
// sign test; ref :42-48,:63-92), corners of one box inside the other with a 1e-2 margin (:50-61), points ordered by atan2
// around their mean (:98-100,:178-187), fan area (:199-206); IoU = overlap / max(sa + sb - overlap, 1e-8) (:209-217).
// tests/ pin this arithmetic to oracle/nms_ref.py expression for expression: do not reorder it.
#pragma once
#include "common.hip.h"

#define NMS_EPS 1e-8f
#define NMS_MARGIN 1e-2f

struct P2 {
    float x, y;
};

__device__ __forceinline__ float cross3(P2 p1, P2 p2, P2 p0) {
    return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

__device__ __forceinline__ bool seg_cross(P2 p1, P2 p0, P2 q1, P2 q0, P2 &out) {
    if (!(fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
          fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y)))
        return false;
    const float s1 = cross3(q0, p1, p0), s2 = cross3(p1, q1, p0), s3 = cross3(p0, q1, q0), s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0.f && s3 * s4 > 0.f)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > NMS_EPS) {
        out.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        out.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        out.x = (b0 * c1 - b1 * c0) / D;
        out.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

struct Box7 {
    float x, y, z, dx, dy, dz, r;
};

__device__ __forceinline__ bool inside(const Box7 &b, P2 p) {
    const float c = cosf(-b.r), s = sinf(-b.r);
    const float rx = (p.x - b.x) * c + (p.y - b.y) * (-s), ry = (p.x - b.x) * s + (p.y - b.y) * c;
    return fabsf(rx) < b.dx / 2 + NMS_MARGIN && fabsf(ry) < b.dy / 2 + NMS_MARGIN;
}

__device__ __forceinline__ void corners_of(const Box7 &b, P2 (&c)[5]) {
    // the reference's arithmetic, rounding for rounding (iou3d_nms_kernel.cu:109-111,125-128: axis-aligned corners
    // x -+ dx/2 FIRST; :94-98 rotate_around_center subtracts the centre again) -- for large |x| the corners differ in the
    // last bits from (-+ dx/2) rotated directly, enough to flip a pair whose IoU sits at the threshold
    const float hx = b.dx / 2, hy = b.dy / 2, cs = cosf(b.r), sn = sinf(b.r);
    const float x1 = b.x - hx, x2 = b.x + hx, y1 = b.y - hy, y2 = b.y + hy;
    const float px[4] = {x1, x2, x2, x1}, py[4] = {y1, y1, y2, y2};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c[k].x = (px[k] - b.x) * cs + (py[k] - b.y) * (-sn) + b.x;
        c[k].y = (px[k] - b.x) * sn + (py[k] - b.y) * cs + b.y;
    }
    c[4] = c[0];
}

__device__ float rect_overlap(const Box7 &a, const Box7 &b) {
    P2 ca[5], cb[5], pts[24];
    corners_of(a, ca);
    corners_of(b, cb);
    int n = 0;
    float sx = 0.f, sy = 0.f;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            P2 p;
            if (seg_cross(ca[i + 1], ca[i], cb[j + 1], cb[j], p)) {
                pts[n++] = p;
                sx += p.x;
                sy += p.y;
            }
        }
    for (int k = 0; k < 4; ++k) {
        if (inside(a, cb[k])) {
            pts[n++] = cb[k];
            sx += cb[k].x;
            sy += cb[k].y;
        }
        if (inside(b, ca[k])) {
            pts[n++] = ca[k];
            sx += ca[k].x;
            sy += ca[k].y;
        }
    }
    if (n == 0) return 0.f;
    const float mx = sx / n, my = sy / n;
    float ang[24];
    for (int k = 0; k < n; ++k) ang[k] = atan2f(pts[k].y - my, pts[k].x - mx);
    for (int j = 0; j < n - 1; ++j)  // the reference's bubble sort (stable for equal angles)
        for (int i = 0; i < n - j - 1; ++i)
            if (ang[i] > ang[i + 1]) {
                const float t = ang[i]; ang[i] = ang[i + 1]; ang[i + 1] = t;
                const P2 q = pts[i]; pts[i] = pts[i + 1]; pts[i + 1] = q;
            }
    float area = 0.f;
    for (int k = 0; k < n - 1; ++k)
        area += (pts[k].x - pts[0].x) * (pts[k + 1].y - pts[0].y) - (pts[k].y - pts[0].y) * (pts[k + 1].x - pts[0].x);
    return fabsf(area) / 2.0f;
}

__device__ __forceinline__ float iou_bev(const Box7 &a, const Box7 &b) {
    const float sa = a.dx * a.dy, sb = b.dx * b.dy, ov = rect_overlap(a, b);
    return ov / fmaxf(sa + sb - ov, NMS_EPS);
}

// axis-aligned IoU, the heading ignored (ref iou3d_nms_kernel.cu:314-325)
__device__ __forceinline__ float iou_normal(const Box7 &a, const Box7 &b) {
    const float left = fmaxf(a.x - a.dx / 2, b.x - b.dx / 2), right = fminf(a.x + a.dx / 2, b.x + b.dx / 2);
    const float top = fmaxf(a.y - a.dy / 2, b.y - b.dy / 2), bottom = fminf(a.y + a.dy / 2, b.y + b.dy / 2);
    const float width = fmaxf(right - left, 0.f), height = fmaxf(bottom - top, 0.f);
    const float inter = width * height, sa = a.dx * a.dy, sb = b.dx * b.dy;
    return inter / fmaxf(sa + sb - inter, NMS_EPS);
}

// rows of >= 7 floats, `stride` floats apart
__device__ __forceinline__ Box7 load_box(const float *boxes, int i, int stride = 7) {
    const float *p = boxes + (size_t)i * stride;
    return Box7{p[0], p[1], p[2], p[3], p[4], p[5], p[6]};
}
