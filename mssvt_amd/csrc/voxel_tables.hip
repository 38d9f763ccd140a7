// voxel_tables.hip -- the interpolation tables of a window plan, one lane per (voxel, table), and the CompressBlock's chunk
// ends in the same launch.
//
// k_window_plan runs one wavefront per window; a 160k-point scene has 3.8 voxels per window, so its table phase (ref K9 + K10
// + weights, mssvt_backbone.py:298-311) kept ~8 of 64 lanes busy behind per-window candidate staging in LDS.  Here the same
// arithmetic runs with full wavefronts in a light launch: the plan kernel leaves, per voxel of a win1 list, the window that
// lists it (vox_win), and every (voxel, table) lane rebuilds the window's candidate list from what the plan stored anyway --
// nq_valid (valid slots of the list) and qmeta (.w of a slot = the global feature row of its voxel) -- and the voxel cells
// of `indices`.  The tables are BYTE-identical to those of mssvt_window_plan_two(num_tabs > 0): the same candidates in the
// same (slot) order, the same distance expression and strict `<`, the same hardware square root / reciprocal.
//
// Workgroups behind the table lanes carry a second, independent job (as k_frame_fill_ln does): the chunk ends of
// k_cmp_ws (compress_ws.hip).  Each of its gridDim workgroups used to repeat the same cost partition of the level in its
// prologue; one wavefront per end computes the G + 1 (window, row) pairs once.
#include "voxel_tables.hip.h"

__global__ void __launch_bounds__(256) k_voxel_tables(VtArgs a) { vt_block(a, (int)blockIdx.x); }

int vt_make_args(VtArgs &a, int num_voxels, const int *indices, const int *vox_win, const int *nq_valid, int win_capacity,
                 const float *qmeta_odd, const float *qmeta_even, const float *qmeta_win1, int max_num_odd, int max_num_even,
                 int max_num_win1, const float *host_voxel_size3, const float *host_range_min3, int num_tabs,
                 const int *host_tab_list, const int *host_tab_interp, const int *host_tab_zero_row, int *const *host_tab_row,
                 float *const *host_tab_w, int chunk_groups, const int *chunk_num_wins_dev, const int *chunk_pair_win,
                 int *chunk_ends) {
    if (num_voxels < 0 || num_tabs < 0 || chunk_groups < 0) return MSSVT_E_BADARG;
    if (num_tabs > VT_MAX_TABS) return MSSVT_E_TOOLARGE;
    a.n = num_voxels; a.win_capacity = win_capacity; a.n_tabs = num_voxels > 0 ? num_tabs : 0;
    a.tab_blocks = divup(num_voxels, 256);
    a.indices = indices; a.vox_win = vox_win; a.nq_valid = nq_valid;
    a.vsx = a.vsy = a.vsz = a.minx = a.miny = a.minz = 0.f;
    for (int t = 0; t < VT_MAX_TABS; ++t) a.tabs[t] = VtArgs::Tab{0, 1, 0, 0, nullptr, nullptr, nullptr};
    if (num_tabs > 0) {
        if (!indices || !vox_win || !nq_valid || win_capacity <= 0 || !host_voxel_size3 || !host_range_min3 || !host_tab_list ||
            !host_tab_interp || !host_tab_zero_row || !host_tab_row || !host_tab_w)
            return MSSVT_E_BADARG;
        a.vsx = host_voxel_size3[0]; a.vsy = host_voxel_size3[1]; a.vsz = host_voxel_size3[2];
        a.minx = host_range_min3[0]; a.miny = host_range_min3[1]; a.minz = host_range_min3[2];
        for (int t = 0; t < num_tabs; ++t) {
            const int l = host_tab_list[t];
            if (l < 0 || l > 2 || !host_tab_row[t] || !host_tab_w[t]) return MSSVT_E_BADARG;
            VtArgs::Tab &tb = a.tabs[t];
            tb.list = l;
            tb.maxn = l == 0 ? max_num_odd : l == 1 ? max_num_even : max_num_win1;
            tb.qmeta = reinterpret_cast<const float4 *>(l == 0 ? qmeta_odd : l == 1 ? qmeta_even : qmeta_win1);
            if (tb.maxn <= 0 || !tb.qmeta) return MSSVT_E_BADARG;
            tb.interp = host_tab_interp[t] ? 1 : 0;
            tb.zero_row = host_tab_zero_row[t];
            tb.tab_row = reinterpret_cast<int4 *>(host_tab_row[t]);
            tb.tab_w = reinterpret_cast<float4 *>(host_tab_w[t]);
        }
    }
    a.groups = chunk_groups; a.num_wins = chunk_num_wins_dev; a.pair_win = chunk_pair_win;
    a.ends = reinterpret_cast<int2 *>(chunk_ends);
    if (chunk_groups > 0 && (!chunk_num_wins_dev || !chunk_pair_win || !chunk_ends)) return MSSVT_E_BADARG;
    return MSSVT_OK;
}

extern "C" int mssvt_voxel_tables(int num_voxels, const int *indices, const int *vox_win, const int *nq_valid, int win_capacity,
                                  const float *qmeta_odd, const float *qmeta_even, const float *qmeta_win1, int max_num_odd,
                                  int max_num_even, int max_num_win1, const float *host_voxel_size3,
                                  const float *host_range_min3, int num_tabs, const int *host_tab_list,
                                  const int *host_tab_interp, const int *host_tab_zero_row, int *const *host_tab_row,
                                  float *const *host_tab_w, int chunk_groups, const int *chunk_num_wins_dev,
                                  const int *chunk_pair_win, int *chunk_ends, void *stream) {
    VtArgs a;
    const int rc = vt_make_args(a, num_voxels, indices, vox_win, nq_valid, win_capacity, qmeta_odd, qmeta_even, qmeta_win1, max_num_odd,
                                max_num_even, max_num_win1, host_voxel_size3, host_range_min3, num_tabs, host_tab_list, host_tab_interp,
                                host_tab_zero_row, host_tab_row, host_tab_w, chunk_groups, chunk_num_wins_dev, chunk_pair_win, chunk_ends);
    if (rc != MSSVT_OK) return rc;
    const int grid = vt_blocks(a);
    if (grid <= 0) return MSSVT_OK;
    k_voxel_tables<<<grid, 256, 0, (hipStream_t)stream>>>(a);
    return mssvt_launch_status();
}
