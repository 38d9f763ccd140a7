// voxel_tables.hip.h -- the work of one workgroup of the voxel-table launch (voxel_tables.hip), shared by k_voxel_tables and
// by the launch of k_query_rows (window_plan.hip) that carries the same workgroups behind its own.
#pragma once
#include "common.hip.h"

#define VT_MAX_TABS 4
#define VT_BATCH 8  // candidates whose loads travel together (a run-time loop with a load in it is a chain of round trips)

struct VtArgs {
    int n, win_capacity, n_tabs, tab_blocks;
    const int *indices, *vox_win, *nq_valid;
    float vsx, vsy, vsz, minx, miny, minz;
    struct Tab {
        int list, maxn, interp, zero_row;
        const float4 *qmeta;  // of the table's query list
        int4 *tab_row;
        float4 *tab_w;
    } tabs[VT_MAX_TABS];
    // chunk ends (optional)
    int groups;
    const int *num_wins, *pair_win;
    int2 *ends;
};

__device__ __forceinline__ float vt_centre(int idx, float cell, float lo) {  // plan_centre of window_plan.hip
    return __fadd_rn(__fmul_rn(__fadd_rn((float)idx, 0.5f), cell), lo);
}

// One wavefront per interior end c of 1 .. G - 1 (compress_ws.hip: cost before row r = 8 r + 5 pair_win[r], windows numbered
// in row order): the first row whose cost reaches c / G of the total, by a 64-way search (3 rounds at 160k points), then the
// next window START at or after it.  Rows in no window (-1) make the cost dip; the search takes the first sample that reaches
// the target in every round, which keeps the ends non-decreasing in c whatever the dips.
__device__ __forceinline__ void vt_chunk_end(const VtArgs &a, int c) {
    const int lane = lane_id(), n = a.n, G = a.groups;
    const int nw = *a.num_wins;
    if (c == 0 || c >= G || nw <= 0) {
        if (lane == 0) a.ends[c] = c == 0 ? make_int2(0, 0) : make_int2(max(nw, 0), n);
        return;
    }
    const long long total = 8ll * n + 5ll * nw, tgt = total * c / G;
    int lo = 0, hi = n;  // the answer lies in [lo, hi]; hi == n or cost(hi) >= tgt
    while (lo < hi) {
        const int step = (hi - lo + MSSVT_WAVE - 1) / MSSVT_WAVE;
        const int s = min(lo + (lane + 1) * step - 1, hi - 1);
        const long long cost = 8ll * s + 5ll * max(a.pair_win[s], 0);
        const unsigned long long reach = __ballot(cost >= tgt);
        if (!reach) {
            lo = hi;
        } else {
            const int l = __ffsll((long long)reach) - 1;
            hi = __builtin_amdgcn_readlane(s, l);
            lo = l == 0 ? lo : __builtin_amdgcn_readlane(s, l - 1) + 1;
            lo = min(lo, hi);
        }
    }
    int ew = nw, er = n;
    if (hi < n) {
        int pv = hi > 0 ? a.pair_win[hi - 1] : -1;
        for (int rr = hi; rr < n; rr += MSSVT_WAVE) {
            const int pw = rr + lane < n ? a.pair_win[rr + lane] : -1;
            // the first listed row whose window differs from the last listed window before these rows.  pv is seeded from row
            // hi - 1 alone, which may be unlisted (-1): that is the last listed window only because a pillar window is ONE
            // contiguous run of rows and the unlisted rows of a column sit at its end, so an unlisted row hi - 1 ends its
            // column and the next listed row starts a window (k_cmp_ws's own search relies on the same layout)
            const unsigned long long hit = __ballot(pw >= 0 && pw != pv);
            if (hit) {
                const int l = __ffsll((long long)hit) - 1;
                ew = __builtin_amdgcn_readlane(pw, l);
                er = rr + l;
                break;
            }
            const unsigned long long any = __ballot(pw >= 0);
            if (any) pv = __builtin_amdgcn_readlane(pw, 63 - __clzll((long long)any));
        }
    }
    if (lane == 0) a.ends[c] = make_int2(ew, er);
}

// workgroup `blk` of n_tabs * tab_blocks table workgroups (256 lanes) followed by the chunk-end workgroups (4 wavefronts)
__device__ __forceinline__ void vt_block(const VtArgs &a, const int blk) {
    if (blk >= a.n_tabs * a.tab_blocks) {
        const int c = (blk - a.n_tabs * a.tab_blocks) * 4 + (int)threadIdx.x / MSSVT_WAVE;
        if (c <= a.groups) vt_chunk_end(a, c);
        return;
    }
    const int t = blk / a.tab_blocks;  // workgroup-uniform
    const int v = (blk - t * a.tab_blocks) * 256 + threadIdx.x;
    if (v >= a.n) return;
    const VtArgs::Tab &tb = a.tabs[t];
    const int maxn = tb.maxn, zero = tb.zero_row;
    const int w = a.vox_win[v];
    const int4 none = make_int4(-1, -1, -1, -1);
    if (w < 0) {  // in no win1 list: the attention does not update the voxel
        tb.tab_row[v] = none;
        return;
    }
    const int nvl = a.nq_valid[(size_t)tb.list * a.win_capacity + w];
    const float4 *qm = tb.qmeta + (size_t)w * maxn;
    if (!tb.interp) {  // ref mssvt_backbone.py:327-330: only the query voxels are updated -- the voxel's own slot, if any
        int slot = -1;
        for (int k0 = 0; k0 < nvl; k0 += VT_BATCH) {
            int row[VT_BATCH];
#pragma unroll
            for (int u = 0; u < VT_BATCH; ++u) row[u] = k0 + u < nvl ? __builtin_bit_cast(int, qm[k0 + u].w) : -1;
#pragma unroll
            for (int u = 0; u < VT_BATCH; ++u) slot = row[u] == v ? k0 + u : slot;
        }
        if (slot >= 0) {
            tb.tab_row[v] = make_int4(w * maxn + slot, zero, zero, 0);
            tb.tab_w[v] = make_float4(1.f, 0.f, 0.f, 0.f);
        } else {
            tb.tab_row[v] = none;
        }
        return;
    }
    // K9 (ref interpolate_gpu.cu:16-59) + weights (ref :305-307).  Known points = ALL query slots of the window, in slot
    // order: every valid slot (they come first), and of the EMPTY slots -- all the same point, the world origin, with zero
    // features (ref :302) -- only the first three: the search keeps the first seen on ties (strict <), a fourth never enters
    const int ncand = nvl + min(3, maxn - nvl);
    const int4 vi = reinterpret_cast<const int4 *>(a.indices)[v];  // [b, z, y, x]
    const float ux = vt_centre(vi.w, a.vsx, a.minx), uy = vt_centre(vi.z, a.vsy, a.miny), uz = vt_centre(vi.y, a.vsz, a.minz);
    float b1 = INFINITY, b2 = INFINITY, b3 = INFINITY;
    int c1 = -1, c2 = -1, c3 = -1;
    // (requesting a fixed number of slots before the count is known was measured: 32 us against 12 -- the launch is bound by
    // the number of memory requests, not by their latency)
    for (int k0 = 0; k0 < ncand; k0 += VT_BATCH) {
        int row[VT_BATCH];
        int4 ci[VT_BATCH];
#pragma unroll
        for (int u = 0; u < VT_BATCH; ++u) row[u] = k0 + u < nvl ? __builtin_bit_cast(int, qm[k0 + u].w) : -1;
#pragma unroll
        for (int u = 0; u < VT_BATCH; ++u)
            ci[u] = row[u] >= 0 ? reinterpret_cast<const int4 *>(a.indices)[row[u]] : make_int4(0, 0, 0, 0);
#pragma unroll
        for (int u = 0; u < VT_BATCH; ++u) {
            const int k = k0 + u;
            if (k >= ncand) break;
            const bool valid = k < nvl;
            const float kx = valid ? vt_centre(ci[u].w, a.vsx, a.minx) : 0.f, ky = valid ? vt_centre(ci[u].z, a.vsy, a.miny) : 0.f,
                        kz = valid ? vt_centre(ci[u].y, a.vsz, a.minz) : 0.f;
            const float dx = ux - kx, dy = uy - ky, dz = uz - kz;
            const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
            if (d < b1) { b3 = b2; c3 = c2; b2 = b1; c2 = c1; b1 = d; c1 = k; }
            else if (d < b2) { b3 = b2; c3 = c2; b2 = d; c2 = k; }
            else if (d < b3) { b3 = d; c3 = k; }
        }
    }
    // fewer than three candidates (nq < 3): the reference leaves index 0 / distance 1e40 -> weight ~0
    // (hardware square root / reciprocal, 1 ulp each, exactly as k_window_plan forms them)
    const float d1 = fmaxf(c1 >= 0 ? __builtin_amdgcn_sqrtf(b1) : INFINITY, 1e-10f),
                d2 = fmaxf(c2 >= 0 ? __builtin_amdgcn_sqrtf(b2) : INFINITY, 1e-10f),
                d3 = fmaxf(c3 >= 0 ? __builtin_amdgcn_sqrtf(b3) : INFINITY, 1e-10f);
    float w1 = __builtin_amdgcn_rcpf(d1), w2 = __builtin_amdgcn_rcpf(d2), w3 = __builtin_amdgcn_rcpf(d3);
    const float rnorm = __builtin_amdgcn_rcpf((w1 + w2) + w3);
    w1 *= rnorm; w2 *= rnorm; w3 *= rnorm;
    if (c2 < 0) w1 = 1.f;  // one candidate (nq == 1): the reference's w / w is exactly 1, rcp(w) * w need not be
    if (c1 < 0 || c1 >= nvl) w1 = 0.f;  // empty slots carry zero features
    if (c2 < 0 || c2 >= nvl) w2 = 0.f;
    if (c3 < 0 || c3 >= nvl) w3 = 0.f;
    tb.tab_row[v] = make_int4(w1 != 0.f ? w * maxn + c1 : zero, w2 != 0.f ? w * maxn + c2 : zero, w3 != 0.f ? w * maxn + c3 : zero, 0);
    tb.tab_w[v] = make_float4(w1, w2, w3, 0.f);
}

// workgroups of 256 lanes that vt_block needs for `a`
static inline int vt_blocks(const VtArgs &a) { return a.n_tabs * a.tab_blocks + (a.groups > 0 ? divup(a.groups + 1, 4) : 0); }

// fills `a` from the arguments of mssvt_voxel_tables (defined in voxel_tables.hip); MSSVT_OK or an error code
int vt_make_args(VtArgs &a, int num_voxels, const int *indices, const int *vox_win, const int *nq_valid, int win_capacity,
                 const float *qmeta_odd, const float *qmeta_even, const float *qmeta_win1, int max_num_odd, int max_num_even,
                 int max_num_win1, const float *host_voxel_size3, const float *host_range_min3, int num_tabs,
                 const int *host_tab_list, const int *host_tab_interp, const int *host_tab_zero_row, int *const *host_tab_row,
                 float *const *host_tab_w, int chunk_groups, const int *chunk_num_wins_dev, const int *chunk_pair_win,
                 int *chunk_ends);

// step lists of the paired window launch, built by the plan-order launches (window_plan.hip, mssvt_plan_order_steps):
// live[g] = the plan kernel's flag of head group g, steps / num_steps[list * num_groups + g], scratch of
// mssvt_plan_order_steps_scratch_ints ints
struct PlanStepsArgs {
    int num_groups;
    const int *const *live;
    int *const *steps, *const *num_steps;
    int *scratch;
};

// mssvt_plan_order_multi (window_plan.hip) whose k_query_rows launch also carries the workgroups of `vt` (NULL: none) and whose
// k_plan_order launches also build the step lists of `sa` (NULL: none)
int mssvt_plan_order_multi_vt(int num_sets, const int *num_wins_dev, const int *const *host_nq_valid, const int *host_nq,
                              const float *const *host_qmeta, int win_capacity, int row_capacity, int *const *host_perm,
                              int *const *host_num_active, int *const *host_q_off, float *const *host_qrow_meta,
                              int *const *host_qrow_src, int *const *host_num_rows, const VtArgs *vt, const PlanStepsArgs *sa,
                              void *stream);
