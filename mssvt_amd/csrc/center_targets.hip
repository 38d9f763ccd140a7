// center_targets.hip -- CenterHead's training targets for one head and the whole batch in ONE launch.
//
// Replaces assign_target_of_single_head + the per-sample host loop around it (ref: pcdet/models/dense_heads/
// center_head.py:103-158 and :160-214; gaussian_radius / draw_gaussian_to_heatmap, pcdet/models/model_utils/
// centernet_utils.py:9-69): boxes to the host, one numpy patch and one torch.max per object, maps back to the device.
//   k_center_targets : a 256-thread workgroup owns one (sample, class, 32 x 32 tile) of the heat map in LDS.  It walks the
//                      sample's box rows 256 at a time, works out each row's record (class inside the head, slot, cell,
//                      radius), keeps the objects of its class whose patch meets its tile, max-merges their Gaussians into
//                      the tile (LDS atomicMax on the bit pattern: every value is >= 0, so unsigned order is float order, and
//                      a maximum does not depend on the order) and stores the tile.  The workgroup of tile 0 / class 0 of a
//                      sample also writes that sample's target_boxes / inds / masks rows.
// Every output element is written exactly once with a plain store: no memset, no global atomic, nothing read back.
// The per-row record is recomputed by every workgroup on purpose (a few hundred rows x ~30 flops: less than a second launch).
//
// Arithmetic: each step of the record is ONE correctly rounded float32 operation in the order of the reference's torch
// expressions (no contraction: a fused discriminant can move the truncated radius by one, which moves a whole patch); the
// Gaussian's exponent is evaluated in double and rounded to float once, as numpy does it.  The reference's "drop entries
// below eps x peak" cannot fire (the smallest entry of a patch is exp(-36 r^2 / (2 r + 1)^2) > e^-9) and is not built.
#include "common.hip.h"

#define CT_TILE 32
#define CT_THREADS 256
#define CT_WAVES (CT_THREADS / MSSVT_WAVE)
#define CT_MAX_RADIUS (1 << 20)  // cells; a larger radius (a box > 10^6 cells long) is cut to this

struct CtParams {
    int N, D, num_labels, H, W, M, tiles_x, min_radius;
    float x_min, y_min, voxel_x, voxel_y, stride, k1, k2, k3, k4, k5;
};

struct CtRecord {
    int cls;    // class inside the head, -1: the row is not selected (takes no slot)
    bool ok;    // finite, positive extent: gets a target
    int ix, iy, radius;
    float cx, cy;
};

// the record of one box row (row[0..D-1], label last)
__device__ __forceinline__ CtRecord ct_record(const float *row, const int *class_of_label, const CtParams &p) {
#pragma clang fp contract(off)
    CtRecord r;
    r.cls = -1; r.ok = false; r.ix = 0; r.iy = 0; r.radius = 0; r.cx = 0.f; r.cy = 0.f;
    const float lab = row[p.D - 1];
    // the label is compared as a float first: NaN / out of 0..C never reaches the conversion or the table
    if (!(lab > -1.f && lab < (float)p.num_labels)) return r;
    r.cls = class_of_label[(int)lab];
    if (r.cls < 0) return r;
    bool finite = true;
    for (int k = 0; k < p.D - 1; ++k) finite = finite && __builtin_isfinite(row[k]);
    const float dx = (row[3] / p.voxel_x) / p.stride, dy = (row[4] / p.voxel_y) / p.stride;
    if (!(finite && dx > 0.f && dy > 0.f)) return r;
    r.ok = true;
    const float tx = ((row[0] - p.x_min) / p.voxel_x) / p.stride, ty = ((row[1] - p.y_min) / p.voxel_y) / p.stride;
    r.cx = fminf(fmaxf(tx, 0.f), (float)p.W - 0.5f);
    r.cy = fminf(fmaxf(ty, 0.f), (float)p.H - 0.5f);
    r.ix = (int)r.cx;  // in [0, W - 1] / [0, H - 1] by the clamp
    r.iy = (int)r.cy;
    // gaussian_radius(height = dx, width = dy): the smallest of CornerNet's three roots
    const float s = dx + dy, q = dx * dy;
    const float r1 = (s + sqrtf(s * s - ((4.0f * q) * p.k1) / p.k2)) / 2.0f;
    const float r2 = (2.0f * s + sqrtf((4.0f * s) * s - p.k3 * q)) / 2.0f;
    const float b = p.k4 * s;
    const float r3 = (b + sqrtf(b * b - p.k5 * q)) / 2.0f;
    const float rm = fminf(fminf(r1, r2), r3);
    // truncation; below 1 (negative and NaN included) the minimum radius (>= 0) wins anyway
    const int ri = rm >= 1.f ? (rm < (float)CT_MAX_RADIUS ? (int)rm : CT_MAX_RADIUS) : 0;
    r.radius = ri > p.min_radius ? ri : p.min_radius;
    return r;
}

template <bool VEC4>
__global__ void __launch_bounds__(CT_THREADS) k_center_targets(CtParams p, const float *gt_boxes, const int *class_of_label,
                                                                float *heatmaps, float *target_boxes, long long *inds,
                                                                long long *masks) {
    __shared__ unsigned int tile[CT_TILE * CT_TILE];
    __shared__ int wave_count[2][CT_WAVES];
    __shared__ int kept_count[2];
    __shared__ int kept_x[2][CT_THREADS], kept_y[2][CT_THREADS], kept_r[2][CT_THREADS];

    const int tid = threadIdx.x, lane = lane_id(), wave = tid / MSSVT_WAVE;
    const int tile_id = blockIdx.x, my_cls = blockIdx.y, b = blockIdx.z, num_cls = gridDim.y;
    const int x0 = (tile_id % p.tiles_x) * CT_TILE, y0 = (tile_id / p.tiles_x) * CT_TILE;
    // inclusive tile bounds inside the map
    const int x1 = min(x0 + CT_TILE, p.W) - 1, y1 = min(y0 + CT_TILE, p.H) - 1;
    const bool writes_objects = tile_id == 0 && my_cls == 0;

    for (int i = tid; i < CT_TILE * CT_TILE; i += CT_THREADS) tile[i] = 0u;
    if (tid < 2) kept_count[tid] = 0;

    const float *boxes = gt_boxes + (size_t)b * (size_t)p.N * (size_t)p.D;
    float *tb = target_boxes + (size_t)b * (size_t)p.M * (size_t)p.D;
    long long *ind = inds + (size_t)b * (size_t)p.M, *msk = masks + (size_t)b * (size_t)p.M;

    int running = 0;  // selected rows before this chunk (workgroup-uniform)
    for (int chunk = 0, par = 0; chunk < p.N; chunk += CT_THREADS, par ^= 1) {
        const int row_i = chunk + tid;
        const float *row = boxes + (size_t)(row_i < p.N ? row_i : 0) * (size_t)p.D;
        CtRecord rec = ct_record(row, class_of_label, p);
        if (row_i >= p.N) { rec.cls = -1; rec.ok = false; }
        const bool selected = rec.cls >= 0;
        const unsigned long long m = __ballot(selected);
        const int before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (lane == 0) wave_count[par][wave] = __popcll(m);
        __syncthreads();  // A: the wave counts of this chunk (and, on the first pass, the cleared tile and counters)
        int slot = running + before, total = 0;
        for (int w = 0; w < CT_WAVES; ++w) {
            const int c = wave_count[par][w];
            slot += w < wave ? c : 0;
            total += c;
        }
        running += total;
        if (tid == 0) kept_count[par ^ 1] = 0;  // the next chunk's list; its readers passed barrier A of this chunk
        const bool placed = selected && slot < p.M;

        if (writes_objects && placed) {  // slot < M: one thread per slot
            float *o = tb + (size_t)slot * (size_t)p.D;
            if (rec.ok) {
                o[0] = rec.cx - (float)rec.ix;
                o[1] = rec.cy - (float)rec.iy;
                o[2] = row[2];
                o[3] = logf(row[3]);
                o[4] = logf(row[4]);
                o[5] = logf(row[5]);
                o[6] = cosf(row[6]);
                o[7] = sinf(row[6]);
                for (int k = 8; k < p.D; ++k) o[k] = row[k - 1];
            } else {
                for (int k = 0; k < p.D; ++k) o[k] = 0.f;
            }
            ind[slot] = rec.ok ? (long long)rec.iy * p.W + rec.ix : 0ll;
            msk[slot] = rec.ok ? 1ll : 0ll;
        }

        // keep the objects of this class whose (2 r + 1)^2 patch meets the tile (64-bit: the radius may be large)
        if (placed && rec.ok && rec.cls == my_cls && (long long)rec.ix + rec.radius >= x0 && (long long)rec.ix - rec.radius <= x1 &&
            (long long)rec.iy + rec.radius >= y0 && (long long)rec.iy - rec.radius <= y1) {
            const int k = atomicAdd(&kept_count[par], 1);  // LDS; < CT_THREADS: one entry per thread at most
            kept_x[par][k] = rec.ix;
            kept_y[par][k] = rec.iy;
            kept_r[par][k] = rec.radius;
        }
        __syncthreads();  // B: the list
        const int kept = kept_count[par];
        for (int j = 0; j < kept; ++j) {
            const int ox = kept_x[par][j], oy = kept_y[par][j], rad = kept_r[par][j];
            // the patch clipped to the tile: [ux0, ux1] x [uy0, uy1], non-empty by the filter, inside the tile
            const int ux0 = (int)max((long long)ox - rad, (long long)x0), ux1 = (int)min((long long)ox + rad, (long long)x1);
            const int uy0 = (int)max((long long)oy - rad, (long long)y0), uy1 = (int)min((long long)oy + rad, (long long)y1);
            const int w = ux1 - ux0 + 1, n = w * (uy1 - uy0 + 1);  // <= 32 x 32
            const double sigma = (2 * rad + 1) / 6.0;
            const double den = 2.0 * sigma * sigma;
            for (int e = tid; e < n; e += CT_THREADS) {
                const int x = ux0 + e % w, y = uy0 + e / w;
                const double u = (double)(x - ox), v = (double)(y - oy);
                const float g = (float)exp(-(u * u + v * v) / den);
                atomicMax(&tile[(y - y0) * CT_TILE + (x - x0)], __float_as_uint(g));
            }
        }
    }

    if (writes_objects) {  // the unused slots
        const int used = running < p.M ? running : p.M;
        for (int s = used + tid; s < p.M; s += CT_THREADS) {
            float *o = tb + (size_t)s * (size_t)p.D;
            for (int k = 0; k < p.D; ++k) o[k] = 0.f;
            ind[s] = 0ll;
            msk[s] = 0ll;
        }
    }

    __syncthreads();  // the tile is complete (N = 0: also orders the clearing before the store)
    float *hm = heatmaps + ((size_t)b * (size_t)num_cls + (size_t)my_cls) * (size_t)p.H * (size_t)p.W;
    if (VEC4) {  // W % 4 == 0 and a 16-byte aligned base: each thread one float4, whole inside or outside the map
        const int ty = tid / (CT_TILE / 4), tx = (tid % (CT_TILE / 4)) * 4;
        const int x = x0 + tx, y = y0 + ty;
        if (x < p.W && y < p.H) {
            const unsigned int *t = tile + ty * CT_TILE + tx;
            *reinterpret_cast<float4 *>(hm + (size_t)y * (size_t)p.W + (size_t)x) =
                make_float4(__uint_as_float(t[0]), __uint_as_float(t[1]), __uint_as_float(t[2]), __uint_as_float(t[3]));
        }
    } else {
        for (int i = tid; i < CT_TILE * CT_TILE; i += CT_THREADS) {
            const int x = x0 + i % CT_TILE, y = y0 + i / CT_TILE;
            if (x < p.W && y < p.H) hm[(size_t)y * (size_t)p.W + (size_t)x] = __uint_as_float(tile[i]);
        }
    }
}

extern "C" int mssvt_center_targets(int batch_size, int num_boxes, int code_size, const float *gt_boxes,
                                    const int *class_of_label, int num_labels, int num_classes, int H, int W,
                                    int num_max_objs, float x_min, float y_min, float voxel_x, float voxel_y, float stride,
                                    float k1, float k2, float k3, float k4, float k5, int min_radius, float *heatmaps,
                                    float *target_boxes, long long *inds, long long *masks, void *stream) {
    if (batch_size <= 0 || num_classes <= 0 || H <= 0 || W <= 0 || num_max_objs <= 0 || num_boxes < 0 || code_size < 8 ||
        num_labels <= 0 || min_radius < 0)
        return MSSVT_E_BADARG;
    if (!class_of_label || !heatmaps || !target_boxes || !inds || !masks || (num_boxes > 0 && !gt_boxes)) return MSSVT_E_BADARG;
    // grid limits; W - 0.5 must be a float and the tile count an int
    if (batch_size > 65535 || num_classes > 65535 || H > (1 << 20) || W > (1 << 20) || min_radius > CT_MAX_RADIUS ||
        num_boxes > 0x7FFFFFFF - CT_THREADS)
        return MSSVT_E_TOOLARGE;
    CtParams p;
    p.N = num_boxes; p.D = code_size; p.num_labels = num_labels; p.H = H; p.W = W; p.M = num_max_objs;
    p.tiles_x = divup(W, CT_TILE); p.min_radius = min_radius;
    p.x_min = x_min; p.y_min = y_min; p.voxel_x = voxel_x; p.voxel_y = voxel_y; p.stride = stride;
    p.k1 = k1; p.k2 = k2; p.k3 = k3; p.k4 = k4; p.k5 = k5;
    const dim3 grid(p.tiles_x * divup(H, CT_TILE), num_classes, batch_size);
    hipStream_t st = (hipStream_t)stream;
    if (W % 4 == 0 && ((uintptr_t)heatmaps & 15) == 0)
        k_center_targets<true><<<grid, CT_THREADS, 0, st>>>(p, gt_boxes, class_of_label, heatmaps, target_boxes, inds, masks);
    else
        k_center_targets<false><<<grid, CT_THREADS, 0, st>>>(p, gt_boxes, class_of_label, heatmaps, target_boxes, inds, masks);
    return mssvt_launch_status();
}
