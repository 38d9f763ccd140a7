// vfe_train.hip -- the index and reduction operators of DynamicVFE's TRAINING step over points GROUPED BY VOXEL: a voxel's
// points are a contiguous run of rows, every output element is written by exactly one work item and every float sum has a
// fixed order -- no float atomics, so values and gradients are bit-identical run to run and across streams.
// (ref pcdet/models/backbones_3d/vfe/dynamic_vfe.py:71-131; torch_scatter's scatter_mean / scatter_max with the gradient of
// the maximum split equally between exact ties, as oracle/gen_golden_vfe.py restates them.)
//
//   mssvt_vfe_group          point_voxel (P) -> order (kept points sorted by voxel, ascending point index inside a voxel),
//                            row_voxel, run_off (N + 1), sizes [N, P'] left on the device.  The stable order comes from a
//                            stable library radix sort of the voxel ids (rocPRIM; the result of a stable sort is unique, so
//                            it cannot depend on scheduling), run_off from a binary search of the sorted ids.
//   mssvt_vfe_augment        the PFN input [features, xyz - cluster centre, xyz - voxel centre, |xyz|] of the grouped rows;
//                            the cluster centre from the exact 64-bit fixed-point sums of csrc/vfe.hip (order independent).
//   mssvt_vfe_run_max_*      concat = 1: (P', F) -> (P', 2F) rows [x ; max over the row's run]; concat = 0: (P', F) -> (N, F).
//
// The run kernels give F / 4 lanes to a run (a float4 of channels per lane, 16-byte row accesses; 16 runs per workgroup at
// F = 64): no lane ever needs another lane's value.  Runs are short at the workload's scale (2.1 points per voxel) and very
// long next to the sensor, so a run of more than CHUNK = MSSVT_VFE_TRAIN_CHUNK rows is cut where the fixed windows
// [j CHUNK, (j + 1) CHUNK) of the ROW order cut it: a window meets at most two long runs (one holding its first row, one
// holding its last), so piece (j, which) has a slot of its own in a partials buffer, a first launch reduces every piece
// by a lane group of its own, and the second launch combines a run's pieces in ascending window order.
#include "common.hip.h"

#include <rocprim/device/device_radix_sort.hpp>

#define VT_CHUNK MSSVT_VFE_TRAIN_CHUNK
#define VT_FIX 1048576.0  // 2^20 steps per metre (csrc/vfe.hip)
#define VT_MAX_ROWS 0x7FFFFF00

// ---------------------------------------------------------------------------------------------------------------- grouping

__global__ void __launch_bounds__(256)
    k_vt_keys(const int *point_voxel, int P, int cap, const int *num_voxels_dev, unsigned int *keys, int *vals) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int n = num_voxels_dev ? min(max(*num_voxels_dev, 0), cap) : cap;
    const int v = point_voxel[i];
    keys[i] = v >= 0 && v < n ? (unsigned int)v : (unsigned int)cap;  // dropped points sort behind every voxel
    vals[i] = i;
}

// first index whose key is >= v
__device__ __forceinline__ int vt_lower_bound(const unsigned int *keys, int P, unsigned int v) {
    int lo = 0, hi = P;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256)
    k_vt_offsets(const unsigned int *sorted_keys, int P, int cap, const int *num_voxels_dev, int *run_off, int *sizes) {
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v > cap) return;
    const int n = num_voxels_dev ? min(max(*num_voxels_dev, 0), cap) : cap;
    const int off = vt_lower_bound(sorted_keys, P, (unsigned int)min(v, n));  // entries behind N repeat P': empty runs
    run_off[v] = off;
    if (v == n) {
        sizes[0] = n;
        sizes[1] = off;
    }
}

static unsigned int vt_key_bits(int cap) {
    unsigned int bits = 1;
    while (bits < 32 && ((unsigned int)cap >> bits) != 0) ++bits;
    return bits;
}

static size_t vt_align256(size_t v) { return (v + 255) & ~(size_t)255; }

static hipError_t vt_sort_temp_bytes(long long P, unsigned int bits, size_t *bytes) {
    unsigned int *k = nullptr;
    int *v = nullptr;
    *bytes = 0;
    return rocprim::radix_sort_pairs(nullptr, *bytes, k, k, v, v, (size_t)P, 0u, bits, (hipStream_t)0, false);
}

extern "C" long long mssvt_vfe_group_workspace_bytes(long long num_points, int voxel_capacity) {
    if (num_points < 0 || num_points > VT_MAX_ROWS || voxel_capacity < 0) return 0;
    size_t temp = 0;
    if (num_points > 0 && vt_sort_temp_bytes(num_points, vt_key_bits(voxel_capacity), &temp) != hipSuccess) return 0;
    return (long long)(2 * vt_align256((size_t)num_points * 4) + vt_align256(temp) + 256);
}

extern "C" int mssvt_vfe_group(const int *point_voxel, long long num_points, int voxel_capacity, const int *num_voxels_dev,
                               int *order, int *row_voxel, int *run_off, int *sizes, void *workspace,
                               long long workspace_bytes, void *stream_) {
    if (num_points < 0 || voxel_capacity < 0 || (num_points > 0 && (!point_voxel || !order || !row_voxel || !workspace)) ||
        !run_off || !sizes)
        return MSSVT_E_BADARG;
    if (num_points > VT_MAX_ROWS) return MSSVT_E_TOOLARGE;
    hipStream_t stream = (hipStream_t)stream_;
    const int P = (int)num_points, cap = voxel_capacity;
    if (P > 0) {
        const unsigned int bits = vt_key_bits(cap);
        size_t temp = 0;
        hipError_t e = vt_sort_temp_bytes(P, bits, &temp);
        if (e != hipSuccess) return (int)e;
        const size_t col = vt_align256((size_t)P * 4);
        if (workspace_bytes < (long long)(2 * col + vt_align256(temp)) || (reinterpret_cast<uintptr_t>(workspace) & 15))
            return MSSVT_E_BADARG;
        unsigned int *keys = reinterpret_cast<unsigned int *>(workspace);
        int *vals = reinterpret_cast<int *>(reinterpret_cast<char *>(workspace) + col);
        void *tmp = reinterpret_cast<char *>(workspace) + 2 * col;
        k_vt_keys<<<divup(P, 256), 256, 0, stream>>>(point_voxel, P, cap, num_voxels_dev, keys, vals);
        e = rocprim::radix_sort_pairs(tmp, temp, keys, reinterpret_cast<unsigned int *>(row_voxel), vals, order, (size_t)P, 0u, bits,
                                      stream, false);
        if (e != hipSuccess) return (int)e;
    }
    k_vt_offsets<<<divup((long long)cap + 1, 256), 256, 0, stream>>>(reinterpret_cast<const unsigned int *>(row_voxel), P, cap,
                                                                     num_voxels_dev, run_off, sizes);
    return mssvt_launch_status();
}

// ------------------------------------------------------------------------------------------------------------ augmentation

__device__ __forceinline__ long long vt_row_sum_ll(long long v) {  // all-reduce over the 16 lanes of a run's group (exact)
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
        const int lo = __shfl_xor((int)(unsigned int)(unsigned long long)v, off), hi = __shfl_xor((int)((unsigned long long)v >> 32), off);
        v += (long long)(((unsigned long long)(unsigned int)hi << 32) | (unsigned int)lo);
    }
    return v;
}

__device__ __forceinline__ void vt_bounds(const int *run_off, int v, int n_rows, int &s, int &e) {
    e = max(min(run_off[v + 1], n_rows), 0);
    s = min(max(run_off[v], 0), e);
}

// cluster centre of every run: 16 lanes per run, lane q takes rows s + q, s + q + 16, ..., four of them in flight; the
// expression of k_vfe_sum_xyz / k_vfe_mean_xyz (integer sums: any order)
__global__ void __launch_bounds__(256)
    k_vt_center(const float *points, int stride, int P, const int *order, const int *run_off, int n_rows, int N, float *mean3) {
    const int q = threadIdx.x & 15;
    const int v = min(blockIdx.x * 16 + (threadIdx.x >> 4), N - 1);  // (clamped: every lane takes part in the lane sums)
    int s, e;
    vt_bounds(run_off, v, n_rows, s, e);
    long long sx = 0, sy = 0, sz = 0;
    for (int i = s + q; i < e; i += 64) {
        int p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) p[u] = i + 16 * u < e ? order[i + 16 * u] : -1;
        float c[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool ok = (unsigned int)p[u] < (unsigned int)P;
            const float *pr = points + (size_t)(ok ? p[u] : 0) * stride;
#pragma unroll
            for (int k = 0; k < 3; ++k) c[u][k] = ok ? pr[1 + k] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            sx += __double2ll_rn((double)c[u][0] * VT_FIX);
            sy += __double2ll_rn((double)c[u][1] * VT_FIX);
            sz += __double2ll_rn((double)c[u][2] * VT_FIX);
        }
    }
    sx = vt_row_sum_ll(sx); sy = vt_row_sum_ll(sy); sz = vt_row_sum_ll(sz);
    if (q < 3 && blockIdx.x * 16 + (threadIdx.x >> 4) < N) {
        const long long t = q == 0 ? sx : q == 1 ? sy : sz;
        mean3[(size_t)v * 3 + q] = e > s ? (float)((double)t / VT_FIX / (double)(e - s)) : 0.f;
    }
}

struct VtAugArgs {
    const float *points;
    int stride, P;
    const int *order, *row_voxel, *coords;
    int n_rows, N, npf, cc, vc, dist, C;
    const float *mean3;
    float vs[3], off[3];
    float *out;
};

// one thread per element of the (P', C) PFN input (coalesced stores); the reference's expressions, multiply and add rounded
// separately (ref :96-112)
__global__ void __launch_bounds__(256) k_vt_augment(VtAugArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.n_rows * a.C) return;
    const int r = (int)(idx / a.C);
    int c = (int)(idx - (long long)r * a.C);
    const int p = a.order[r], v = a.row_voxel[r];
    float val = 0.f;
    if ((unsigned int)p < (unsigned int)a.P && (unsigned int)v < (unsigned int)a.N) {
        const float *pr = a.points + (size_t)p * a.stride;
        if (c < a.npf) {
            val = pr[1 + c];
        } else {
            c -= a.npf;
            if (a.cc && c < 3) {
                val = pr[1 + c] - a.mean3[(size_t)v * 3 + c];
            } else {
                c -= a.cc ? 3 : 0;
                if (a.vc && c < 3) {
                    const int cell = a.coords[(size_t)v * 4 + 3 - c];  // [b, z, y, x]
                    val = pr[1 + c] - __fadd_rn(__fmul_rn((float)cell, a.vs[c]), a.off[c]);
                } else {
                    const float x = pr[1], y = pr[2], z = pr[3];
                    val = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z)));
                }
            }
        }
    }
    a.out[idx] = val;
}

extern "C" int mssvt_vfe_augment(const float *points, int point_stride, long long num_points, const int *order,
                                 const int *row_voxel, const int *run_off, int num_rows, int num_voxels,
                                 const int *voxel_coords, const float *host_voxel_size3, const float *host_offset3,
                                 int num_point_features, int with_cluster_center, int with_voxel_center, int with_distance,
                                 float *mean3_scratch, float *out, void *stream_) {
    if (num_points < 0 || num_rows < 0 || num_voxels < 0 || num_point_features < 1 ||
        point_stride < 1 + max(num_point_features, 3) || !host_voxel_size3 || !host_offset3)
        return MSSVT_E_BADARG;
    if (num_rows == 0 || num_voxels == 0) return MSSVT_OK;
    if (!points || !order || !row_voxel || !run_off || !voxel_coords || !out || (with_cluster_center && !mean3_scratch) ||
        num_rows > num_points)
        return MSSVT_E_BADARG;
    if (num_points > VT_MAX_ROWS) return MSSVT_E_TOOLARGE;
    hipStream_t stream = (hipStream_t)stream_;
    VtAugArgs a;
    a.points = points; a.stride = point_stride; a.P = (int)num_points;
    a.order = order; a.row_voxel = row_voxel; a.coords = voxel_coords;
    a.n_rows = num_rows; a.N = num_voxels; a.npf = num_point_features;
    a.cc = with_cluster_center ? 1 : 0; a.vc = with_voxel_center ? 1 : 0; a.dist = with_distance ? 1 : 0;
    a.C = a.npf + 3 * a.cc + 3 * a.vc + a.dist;
    a.mean3 = mean3_scratch;
    for (int k = 0; k < 3; ++k) { a.vs[k] = host_voxel_size3[k]; a.off[k] = host_offset3[k]; }
    a.out = out;
    if (a.cc)
        k_vt_center<<<divup(num_voxels, 16), 256, 0, stream>>>(points, point_stride, a.P, order, run_off, num_rows, num_voxels,
                                                               mean3_scratch);
    k_vt_augment<<<divup((long long)num_rows * a.C, 256), 256, 0, stream>>>(a);
    return mssvt_launch_status();
}

// ------------------------------------------------------------------------------------------------------------ run maxima

// the last v in [0, N) with run_off[v] <= r: the (non-empty) run that holds row r
__device__ __forceinline__ int vt_run_of(const int *run_off, int N, int r) {
    int lo = 0, hi = N;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (run_off[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// piece (j, which) of the row windows: which = 0 the run that holds the window's first row, which = 1 the run that holds its
// last row when it starts inside the window.  True when that run is long (more than CHUNK rows); its rows [lo, hi) lie in
// window j.  A long run [s, e) meets the windows s / CHUNK .. (e - 1) / CHUNK, in window j its slot is vt_slot(s, j).
__device__ __forceinline__ bool vt_piece(const int *run_off, int N, int n_rows, int j, int which, int &v, int &s, int &e,
                                         int &lo, int &hi) {
    const int b0 = j * VT_CHUNK, b1 = min(b0 + VT_CHUNK, n_rows) - 1;
    v = vt_run_of(run_off, N, which ? b1 : b0);
    vt_bounds(run_off, v, n_rows, s, e);
    if (e - s <= VT_CHUNK) return false;
    if (which ? s <= b0 : s > b0) return false;
    lo = which ? s : b0;
    hi = min(e, b0 + VT_CHUNK);
    return lo < hi;
}
__device__ __forceinline__ size_t vt_slot(int s, int j) { return 2 * (size_t)j + (s <= j * VT_CHUNK ? 0 : 1); }

__device__ __forceinline__ float4 vt_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void vt_st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
__device__ __forceinline__ float4 vt_max4(float4 a, float4 b) {
    return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}
__device__ __forceinline__ float4 vt_add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// channel-wise maximum of rows [lo, hi) (hi > lo) of x (row stride ld floats) at channels c0 .. c0 + 3: eight rows in flight.
// Seeded with the first row, never with zero: a run of negative values keeps its own maximum.
__device__ __forceinline__ float4 vt_rows_max(const float *x, int ld, int c0, int lo, int hi) {
    float4 m = vt_ld4(x + (size_t)lo * ld + c0);
    for (int r = lo; r < hi; r += 8) {
        float4 t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = vt_ld4(x + (size_t)min(r + u, hi - 1) * ld + c0);
#pragma unroll
        for (int u = 0; u < 8; ++u) m = vt_max4(m, t[u]);
    }
    return m;
}

struct VtRunArgs {
    int n_rows, N, F, G, gpb;  // G = F / 4 lanes per group, gpb groups per workgroup
    int run_blocks;            // workgroups [0, run_blocks) take runs, the ones behind them pieces
    long long n_tasks;         // pieces: 2 per window of CHUNK rows
    const int *run_off;
    const float *x;      // forward: (P', F).  backward: concat ? the forward's output (P', 2F) : x (P', F)
    const float *m;      // backward, concat = 0: the forward's output (N, F)
    const float *g;      // backward: concat ? (P', 2F) : (N, F)
    float *parts;        // 2 F floats per slot, slot = 2 window + which
    float *out;          // forward: concat ? (P', 2F) : (N, F).  backward: gx (P', F)
};

// first launch of the forward: the maximum of every piece of a long run
__global__ void __launch_bounds__(256) k_vt_piece_max(VtRunArgs a) {
    const int grp = threadIdx.x / a.G, q = threadIdx.x - grp * a.G;
    if (grp >= a.gpb) return;
    const long long t = (long long)blockIdx.x * a.gpb + grp;
    if (t >= a.n_tasks) return;
    int v, s, e, lo, hi;
    if (!vt_piece(a.run_off, a.N, a.n_rows, (int)(t >> 1), (int)(t & 1), v, s, e, lo, hi)) return;
    vt_st4(a.parts + (size_t)t * 2 * a.F + 4 * q, vt_rows_max(a.x, a.F, 4 * q, lo, hi));
}

__device__ __forceinline__ float4 vt_combine_max(const VtRunArgs &a, int q, int s, int e) {
    const int j0 = s / VT_CHUNK, j1 = (e - 1) / VT_CHUNK;
    float4 m = vt_ld4(a.parts + vt_slot(s, j0) * 2 * a.F + 4 * q);
    for (int j = j0 + 1; j <= j1; ++j) m = vt_max4(m, vt_ld4(a.parts + vt_slot(s, j) * 2 * a.F + 4 * q));
    return m;
}

__device__ __forceinline__ void vt_write_concat(const VtRunArgs &a, int q, int lo, int hi, float4 m) {
    for (int r = lo; r < hi; r += 4) {
        float4 t[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = vt_ld4(a.x + (size_t)min(r + u, hi - 1) * a.F + 4 * q);
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (r + u < hi) {
                float *dst = a.out + (size_t)(r + u) * 2 * a.F + 4 * q;
                vt_st4(dst, t[u]);
                vt_st4(dst + a.F, m);
            }
    }
}

// second launch of the forward.  A group per run: its maximum (a short run: a loop over its rows; a long one: its pieces in
// window order) and, CONCAT, the rows [x ; max] of a short run; CONCAT: a group per piece writes the rows of a long run.
template <bool CONCAT>
__global__ void __launch_bounds__(256) k_vt_run_max(VtRunArgs a) {
    const int grp = threadIdx.x / a.G, q = threadIdx.x - grp * a.G;
    if (grp >= a.gpb) return;
    if ((int)blockIdx.x < a.run_blocks) {
        const long long v = (long long)blockIdx.x * a.gpb + grp;
        if (v >= a.N) return;
        int s, e;
        vt_bounds(a.run_off, (int)v, a.n_rows, s, e);
        if (e == s) {  // an empty run: a zero row, nothing else
            if (!CONCAT) vt_st4(a.out + (size_t)v * a.F + 4 * q, make_float4(0.f, 0.f, 0.f, 0.f));
            return;
        }
        const bool is_long = e - s > VT_CHUNK;
        if (CONCAT && is_long) return;
        const float4 m = is_long ? vt_combine_max(a, q, s, e) : vt_rows_max(a.x, a.F, 4 * q, s, e);
        if (CONCAT)
            vt_write_concat(a, q, s, e, m);
        else
            vt_st4(a.out + (size_t)v * a.F + 4 * q, m);
        return;
    }
    const long long t = (long long)((int)blockIdx.x - a.run_blocks) * a.gpb + grp;
    if (t >= a.n_tasks) return;
    int v, s, e, lo, hi;
    if (!vt_piece(a.run_off, a.N, a.n_rows, (int)(t >> 1), (int)(t & 1), v, s, e, lo, hi)) return;
    vt_write_concat(a, q, lo, hi, vt_combine_max(a, q, s, e));
}

// ---- backward.  The maximal rows of a run share its gradient equally: count = rows whose value EQUALS the maximum (-0 == +0
// is a tie), each of them gets gm / count; CONCAT: gm = sum over the run's rows of g[:, F:] in ascending row order (a long run:
// pieces in row order, then the piece sums in window order), and g[:, :F] passes through.

template <bool CONCAT>
__device__ __forceinline__ const float *vt_xrow(const VtRunArgs &a, int r, int q) {
    return a.x + (size_t)r * (CONCAT ? 2 * a.F : a.F) + 4 * q;
}
template <bool CONCAT>
__device__ __forceinline__ float4 vt_run_maximum(const VtRunArgs &a, int v, int s, int q) {
    // CONCAT: the forward's own output holds the broadcast maximum in every row of the run
    return CONCAT ? vt_ld4(a.x + (size_t)s * 2 * a.F + a.F + 4 * q) : vt_ld4(a.m + (size_t)v * a.F + 4 * q);
}

// ties and (CONCAT) the gradient sum of rows [lo, hi), ascending
template <bool CONCAT>
__device__ __forceinline__ void vt_rows_count_sum(const VtRunArgs &a, int q, int lo, int hi, float4 m, int4 &cnt, float4 &sum) {
    cnt = make_int4(0, 0, 0, 0);
    sum = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = lo; r < hi; r += 4) {
        float4 t[4], gm[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int rr = min(r + u, hi - 1);
            t[u] = vt_ld4(vt_xrow<CONCAT>(a, rr, q));
            if (CONCAT) gm[u] = vt_ld4(a.g + (size_t)rr * 2 * a.F + a.F + 4 * q);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (r + u < hi) {
                cnt.x += t[u].x == m.x; cnt.y += t[u].y == m.y; cnt.z += t[u].z == m.z; cnt.w += t[u].w == m.w;
                if (CONCAT) sum = vt_add4(sum, gm[u]);
            }
    }
}

template <bool CONCAT>
__device__ __forceinline__ void vt_rows_grad(const VtRunArgs &a, int q, int lo, int hi, float4 m, int4 cnt, float4 gm) {
    const float4 share = make_float4(cnt.x > 0 ? __fdiv_rn(gm.x, (float)cnt.x) : 0.f, cnt.y > 0 ? __fdiv_rn(gm.y, (float)cnt.y) : 0.f,
                                     cnt.z > 0 ? __fdiv_rn(gm.z, (float)cnt.z) : 0.f, cnt.w > 0 ? __fdiv_rn(gm.w, (float)cnt.w) : 0.f);
    for (int r = lo; r < hi; r += 4) {
        float4 t[4], g0[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int rr = min(r + u, hi - 1);
            t[u] = vt_ld4(vt_xrow<CONCAT>(a, rr, q));
            g0[u] = CONCAT ? vt_ld4(a.g + (size_t)rr * 2 * a.F + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (r + u < hi) {
                float4 o;
                // (a row that does not attain the maximum passes its own gradient on unchanged, not plus zero)
                o.x = t[u].x == m.x ? (CONCAT ? g0[u].x + share.x : share.x) : g0[u].x;
                o.y = t[u].y == m.y ? (CONCAT ? g0[u].y + share.y : share.y) : g0[u].y;
                o.z = t[u].z == m.z ? (CONCAT ? g0[u].z + share.z : share.z) : g0[u].z;
                o.w = t[u].w == m.w ? (CONCAT ? g0[u].w + share.w : share.w) : g0[u].w;
                vt_st4(a.out + (size_t)(r + u) * a.F + 4 * q, o);
            }
    }
}

// first launch of the backward: ties and gradient sum of every piece of a long run -> parts[slot] = [sum (F) | count (F, int32)]
template <bool CONCAT>
__global__ void __launch_bounds__(256) k_vt_piece_grad(VtRunArgs a) {
    const int grp = threadIdx.x / a.G, q = threadIdx.x - grp * a.G;
    if (grp >= a.gpb) return;
    const long long t = (long long)blockIdx.x * a.gpb + grp;
    if (t >= a.n_tasks) return;
    int v, s, e, lo, hi;
    if (!vt_piece(a.run_off, a.N, a.n_rows, (int)(t >> 1), (int)(t & 1), v, s, e, lo, hi)) return;
    int4 cnt;
    float4 sum;
    vt_rows_count_sum<CONCAT>(a, q, lo, hi, vt_run_maximum<CONCAT>(a, v, s, q), cnt, sum);
    float *dst = a.parts + (size_t)t * 2 * a.F + 4 * q;
    vt_st4(dst, sum);
    *reinterpret_cast<int4 *>(dst + a.F) = cnt;
}

// second launch of the backward: a group per SHORT run (count, then its rows), a group per piece of a long run (the run's
// pieces combined in window order, then the piece's rows)
template <bool CONCAT>
__global__ void __launch_bounds__(256) k_vt_run_grad(VtRunArgs a) {
    const int grp = threadIdx.x / a.G, q = threadIdx.x - grp * a.G;
    if (grp >= a.gpb) return;
    int v, s, e, lo, hi;
    int4 cnt;
    float4 sum;
    if ((int)blockIdx.x < a.run_blocks) {
        const long long vv = (long long)blockIdx.x * a.gpb + grp;
        if (vv >= a.N) return;
        v = (int)vv;
        vt_bounds(a.run_off, v, a.n_rows, s, e);
        if (e == s || e - s > VT_CHUNK) return;
        lo = s;
        hi = e;
        vt_rows_count_sum<CONCAT>(a, q, s, e, vt_run_maximum<CONCAT>(a, v, s, q), cnt, sum);
    } else {
        const long long t = (long long)((int)blockIdx.x - a.run_blocks) * a.gpb + grp;
        if (t >= a.n_tasks) return;
        if (!vt_piece(a.run_off, a.N, a.n_rows, (int)(t >> 1), (int)(t & 1), v, s, e, lo, hi)) return;
        cnt = make_int4(0, 0, 0, 0);
        sum = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = s / VT_CHUNK; j <= (e - 1) / VT_CHUNK; ++j) {
            const float *src = a.parts + vt_slot(s, j) * 2 * a.F + 4 * q;
            const int4 c = *reinterpret_cast<const int4 *>(src + a.F);
            cnt.x += c.x; cnt.y += c.y; cnt.z += c.z; cnt.w += c.w;
            if (CONCAT) sum = j == s / VT_CHUNK ? vt_ld4(src) : vt_add4(sum, vt_ld4(src));
        }
    }
    const float4 m = vt_run_maximum<CONCAT>(a, v, s, q);
    vt_rows_grad<CONCAT>(a, q, lo, hi, m, cnt, CONCAT ? sum : vt_ld4(a.g + (size_t)v * a.F + 4 * q));
}

extern "C" long long mssvt_vfe_run_parts_floats(int num_rows, int F) {
    if (num_rows < 0 || num_rows > VT_MAX_ROWS || F <= 0) return 0;
    return 2LL * divup(num_rows, VT_CHUNK) * 2 * F + 4;
}

static int vt_run_args(VtRunArgs &a, const int *run_off, int num_rows, int num_voxels, int F, float *parts) {
    if (num_rows < 0 || num_voxels < 0 || F < 4 || F > 256 || (F & 3)) return MSSVT_E_BADARG;
    if (num_rows > VT_MAX_ROWS) return MSSVT_E_TOOLARGE;
    if (num_voxels > 0 && (!run_off || (num_rows > 0 && !parts))) return MSSVT_E_BADARG;
    a.n_rows = num_rows; a.N = num_voxels; a.F = F; a.G = F / 4; a.gpb = 256 / a.G;
    a.run_blocks = divup(num_voxels, a.gpb);
    a.n_tasks = 2LL * divup(num_rows, VT_CHUNK);
    a.run_off = run_off; a.parts = parts;
    a.x = a.m = a.g = nullptr;
    a.out = nullptr;
    return MSSVT_OK;
}

static bool vt_aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int mssvt_vfe_run_max_forward(const float *x, const int *run_off, int num_rows, int num_voxels, int F, int concat,
                                         float *parts, float *out, void *stream_) {
    VtRunArgs a;
    const int st = vt_run_args(a, run_off, num_rows, num_voxels, F, parts);
    if (st != MSSVT_OK) return st;
    if (num_voxels == 0 || (concat && num_rows == 0)) return MSSVT_OK;
    if (!out || (num_rows > 0 && !x) || !vt_aligned16(x) || !vt_aligned16(out) || !vt_aligned16(parts)) return MSSVT_E_BADARG;
    hipStream_t stream = (hipStream_t)stream_;
    a.x = x; a.out = out;
    const int piece_blocks = divup(a.n_tasks, a.gpb);
    if (piece_blocks) k_vt_piece_max<<<piece_blocks, 256, 0, stream>>>(a);
    if (concat)
        k_vt_run_max<true><<<a.run_blocks + piece_blocks, 256, 0, stream>>>(a);
    else
        k_vt_run_max<false><<<a.run_blocks, 256, 0, stream>>>(a);
    return mssvt_launch_status();
}

extern "C" int mssvt_vfe_run_max_backward(const float *saved, const float *maxima, const float *grad_out, const int *run_off,
                                          int num_rows, int num_voxels, int F, int concat, float *parts, float *grad_x,
                                          void *stream_) {
    VtRunArgs a;
    const int st = vt_run_args(a, run_off, num_rows, num_voxels, F, parts);
    if (st != MSSVT_OK) return st;
    if (num_voxels == 0 || num_rows == 0) return MSSVT_OK;
    if (!saved || !grad_out || !grad_x || (!concat && !maxima) || !vt_aligned16(saved) || !vt_aligned16(maxima) ||
        !vt_aligned16(grad_out) || !vt_aligned16(grad_x) || !vt_aligned16(parts))
        return MSSVT_E_BADARG;
    hipStream_t stream = (hipStream_t)stream_;
    a.x = saved; a.m = maxima; a.g = grad_out; a.out = grad_x;
    const int piece_blocks = divup(a.n_tasks, a.gpb);
    if (concat) {
        k_vt_piece_grad<true><<<piece_blocks, 256, 0, stream>>>(a);
        k_vt_run_grad<true><<<a.run_blocks + piece_blocks, 256, 0, stream>>>(a);
    } else {
        k_vt_piece_grad<false><<<piece_blocks, 256, 0, stream>>>(a);
        k_vt_run_grad<false><<<a.run_blocks + piece_blocks, 256, 0, stream>>>(a);
    }
    return mssvt_launch_status();
}
