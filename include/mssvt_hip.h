/*
 * mssvt_hip.h -- C ABI of libmssvt_hip.so: the MI355X (gfx950) implementation of
 * MsSVT's mixed-scale sparse-voxel attention hot path.
 *
 * This is the drop-in boundary.  Every entry point in
 * part 1 replaces one pybind wrapper of the reference's two CUDA extensions,
 * with the same argument order and meaning, except that
 *   - at::Tensor arguments become raw DEVICE pointers (caller-owned buffers,
 *     C-contiguous, pre-allocated and pre-filled exactly as the reference's
 *     Python callers pre-fill them);
 *   - a trailing `void *stream` (a hipStream_t; NULL = default stream) is added:
 *     the reference launches on the legacy default stream;
 *   - a few calls take a caller-provided `int *workspace` (sizes below) -- the
 *     library never allocates, keeps no global state and never exit()s;
 *   - the return value is 0 on success, a positive hipError_t if a launch
 *     failed, or a negative MSSVT_E_* code for argument errors (the reference
 *     returns the constant 1 and exit(-1)s on error).
 * All pointers are device pointers unless stated otherwise.  All kernels are
 * asynchronous with respect to the host.
 *
 * "ref:" citations are relative to /root/reference/pcdet/ops/.
 */
#ifndef MSSVT_HIP_H
#define MSSVT_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MSSVT_OK 0
#define MSSVT_E_BADARG (-1)   /* null pointer / non-positive size            */
#define MSSVT_E_TOOLARGE (-2) /* a size exceeds what the kernel supports     */

/* Library / build identification.  Returns e.g. 100 for 1.0.0. */
int mssvt_hip_abi_version(void);
/* Static string for a status code returned by any function below. */
const char *mssvt_hip_status_string(int status);

/* ======================================================================== *
 * Part 1a -- replacements for pybind module `mssvt_ops_cuda`
 *            (ref: mssvt/src/ms_api.cpp:7-14)
 * ======================================================================== */

/* Number of int32 words of workspace the two hash builders need for
 * `num_voxels` voxels (flags, ranks and scan partials). */
long long mssvt_hash_workspace_ints(int num_voxels, int batch_size);

/* ref: build_mapping_with_hash_wrapper, mssvt/src/ms_sparse_attention.cpp:23-35
 *      (kernel ms_sparse_attention_gpu.cu:66-97).
 * v_indices (N,4) int32 [b,z,y,x], batch-contiguous; v_bs_cnt (B) int32;
 * xyz_to_vidx (B,H,2) int32 pre-filled with -1 by the caller.
 * The table layout produced equals SEQUENTIAL insertion in voxel-index order
 * (one legal outcome of the reference's racing atomicCAS insertions); for
 * duplicate keys the highest voxel index owns the value.
 * Extra vs the reference: batch_size (to bound b), workspace, stream.        */
int mssvt_build_mapping_with_hash(int x_max, int y_max, int z_max, int num_voxels, int hash_size,
                                  int batch_size, const int *v_indices, const int *v_bs_cnt,
                                  int *xyz_to_vidx, int *workspace, void *stream);

/* ref: window_with_hash_wrapper, ms_sparse_attention.cpp:37-59 (kernel :117-168).
 * w_indices (B,num_windows,3) int32 pre-filled -1 -> rows [wz,wy,wx];
 * xyz_to_vidx (B,H,2) pre-filled -1; vcount (B) zeroed.
 * Windows are numbered by FIRST OCCURRENCE in voxel-index order within each
 * sample and the table equals sequential insertion in that order.  Windows
 * beyond num_windows are counted in vcount but not written (the reference
 * writes out of bounds there).                                               */
int mssvt_window_with_hash(int x_wgs, int y_wgs, int z_wgs, int x_ws, int y_ws, int z_ws,
                           int num_voxels, int num_windows, int hash_size, int batch_size,
                           const int *v_indices, int *w_indices, int *xyz_to_vidx, int *vcount,
                           int *workspace, void *stream);

/* ref: gather_two_window_voxels_with_hash_wrapper, ms_sparse_attention.cpp:61-120
 *      (kernel :193-350).  vox_ind_* (nw,max_num_*) pre-filled -1, vox_coord_*
 * (nw,max_num_*,3) pre-filled 0; vox_query_* (num_*,3) int32 offset tables;
 * win_indices (nw,4) [b,wz,wy,wx]; xyz_to_vidx (B,H,2).                      */
int mssvt_gather_two_window_voxels_with_hash(
    int x_max, int y_max, int z_max, int x_ws, int y_ws, int z_ws, int max_num_odd,
    int max_num_even, int max_num_win1, int max_num_win2, int num_wins, int hash_size, int num_odd,
    int num_even, int num_win1, int num_win2, int *vox_ind_odd, int *vox_ind_even,
    int *vox_ind_win1, int *vox_ind_win2, int *vox_coord_odd, int *vox_coord_even,
    int *vox_coord_win1, int *vox_coord_win2, const int *vox_query_odd, const int *vox_query_even,
    const int *vox_query_win1, const int *vox_query_win2, const int *win_indices,
    const int *xyz_to_vidx, void *stream);

/* ref: gather_one_window_voxels_with_hash_wrapper, ms_sparse_attention.cpp:122-150
 *      (kernel :383-433).                                                    */
int mssvt_gather_one_window_voxels_with_hash(int x_max, int y_max, int z_max, int x_ws, int y_ws,
                                             int z_ws, int max_num_win1, int num_wins,
                                             int hash_size, int num_win1, int *vox_ind_win1,
                                             int *vox_coord_win1, const int *vox_query_win1,
                                             const int *win_indices, const int *xyz_to_vidx,
                                             void *stream);

/* ref: group_features_wrapper_stack, mssvt/src/group_features.cpp:50-68
 *      (kernel group_features_gpu.cu:73-106).  features (N,C) f32, idx (M,nsample)
 * int32 (index within the sample, <0 = skip), out (M,C,nsample) f32 pre-zeroed. */
int mssvt_group_features(int B, int M, int C, int nsample, const float *features,
                         const int *features_batch_cnt, const int *idx, const int *idx_batch_cnt,
                         float *out, void *stream);

/* ref: group_features_grad_wrapper_stack, group_features.cpp:29-47
 *      (kernel group_features_gpu.cu:15-47).  grad_features (N,C) pre-zeroed.  */
int mssvt_group_features_grad(int B, int M, int C, int N, int nsample, const float *grad_out,
                              const int *idx, const int *idx_batch_cnt,
                              const int *features_batch_cnt, float *grad_features, void *stream);

/* ======================================================================== *
 * Part 1b -- replacements for the four forward ops (and two grads) of pybind
 *            module `pointnet2_batch_cuda` that the path uses
 *            (ref: pointnet2/pointnet2_batch/src/pointnet2_api.cpp:10-24)
 * ======================================================================== */

/* ref: farthest_point_sampling_wrapper, pointnet2/pointnet2_batch/src/sampling.cpp:41-50
 *      (kernel sampling_gpu.cu:100-216).  dataset (B,N,3) f32, temp (B,N) f32
 * pre-filled 1e10 (scratch, overwritten), idxs (B,m) int32.  Ties resolve
 * exactly as the reference block of opt_n_threads(N) threads resolves them.   */
int mssvt_farthest_point_sampling(int b, int n, int m, const float *dataset, float *temp,
                                  int *idxs, void *stream);

/* ref: gather_points_wrapper_fast, sampling.cpp:18-27 (kernel sampling_gpu.cu:15-31).
 * points (B,C,N), idx (B,npoints) -> out (B,C,npoints).                       */
int mssvt_gather_points(int b, int c, int n, int npoints, const float *points, const int *idx,
                        float *out, void *stream);
/* ref: gather_points_grad_wrapper_fast, sampling.cpp:29-39 (kernel :53-90).   */
int mssvt_gather_points_grad(int b, int c, int n, int npoints, const float *grad_out,
                             const int *idx, float *grad_points, void *stream);

/* ref: three_nn_wrapper_fast, pointnet2/pointnet2_batch/src/interpolate.cpp:21-30
 *      (kernel interpolate_gpu.cu:16-59).  unknown (B,N,3), known (B,M,3) ->
 * dist2 (B,N,3) squared distances, idx (B,N,3).                               */
int mssvt_three_nn(int b, int n, int m, const float *unknown, const float *known, float *dist2,
                   int *idx, void *stream);

/* ref: group_points_wrapper_fast, pointnet2/pointnet2_batch/src/group_points.cpp:30-40
 *      (kernel group_points_gpu.cu:53-72).  points (B,C,N), idx (B,npoints,nsample)
 * -> out (B,C,npoints,nsample).                                               */
int mssvt_group_points(int b, int c, int n, int npoints, int nsample, const float *points,
                       const int *idx, float *out, void *stream);
/* ref: group_points_grad_wrapper_fast, group_points.cpp:18-28 (kernel :14-50). */
int mssvt_group_points_grad(int b, int c, int n, int npoints, int nsample, const float *grad_out,
                            const int *idx, float *grad_points, void *stream);

/* ======================================================================== *
 * Part 2 -- device-resident variants used by the module fast path.  They
 *           compute exactly what the reference's Python glue computes around
 *           the wrappers above, without host round trips.
 * ======================================================================== */

/* workspace[0] = status bits after any hash builder call (host-readable after a
 * stream sync): */
#define MSSVT_ST_DUPLICATE_KEY 1   /* duplicate voxel coordinates were present   */
#define MSSVT_ST_TABLE_OVERFLOW 2  /* a sample has more distinct keys than H     */
#define MSSVT_ST_WINDOW_OVERFLOW 4 /* a sample has more than max_num_wins windows */

/* K2 + the per-sample compaction of ref mssvt/mssvt_ops.py:45-53 on the device:
 * win_ind receives the (nw,4) rows [b,wz,wy,wx] in sample order, then window
 * number order (capacity: num_voxels rows); vcount (B) = windows per sample
 * (= k_bs_cnt of ref mssvt_backbone.py:218); workspace[1] = nw.              */
int mssvt_window_partition_compact(int x_wgs, int y_wgs, int z_wgs, int x_ws, int y_ws, int z_ws,
                                   int num_voxels, int max_num_wins, int hash_size, int batch_size,
                                   const int *v_indices, int *win_ind, int *xyz_to_vidx,
                                   int *vcount, int *workspace, void *stream);

/* Several window partitions of ONE voxel list in the same five launches (grid.y = partition), e.g. a
 * Block's [3,3,5] windows and the following CompressBlock's [1,1,32] pillars: both only depend on the voxel
 * indices (ref: Block.window_partition, mssvt_backbone.py:139-152, recomputed per block there).
 * Host arrays of num_sets (<= 4) entries: win_grid3 / win_size3 (3 ints each), max_num_wins, and the
 * device pointers win_ind (N,4), tables (B,H,2; pre-filled with -1), vcount (B).  scratch_tables (array or
 * entries may be NULL): a second -1-filled (B,H,2) buffer per partition for the first-occurrence pass --
 * without it the table is its own scratch and is refilled in between.  workspaces: num_sets slices of
 * workspace_stride_ints (>= mssvt_hash_workspace_ints) ints of one allocation; slice k holds
 * [status, window count, ...] of partition k as in mssvt_window_partition_compact. */
int mssvt_window_partition_multi(int num_sets, const int *host_win_grid3, const int *host_win_size3,
                                 const int *host_max_num_wins, int num_voxels, int hash_size, int batch_size,
                                 const int *v_indices, int *const *host_win_ind, int *const *host_tables,
                                 int *const *host_scratch_tables, int *const *host_vcount, int *workspaces,
                                 long long workspace_stride_ints, void *stream);

/* Everything a resolution level needs before its first Block, in one call behind ONE fill:
 * samples' voxel counts (with_bs_cnt, mssvt_backbone.py:124-130), the voxel hash table
 * (SparseTensor.build_map_table, mssvt_utils.py:31-48 = mssvt_build_mapping_with_hash), the occupancy
 * columns of mssvt_occupancy_columns (optional: NULL) and num_sets (0..4) window partitions as in
 * mssvt_window_partition_multi.  zero_region / zero_bytes: one caller allocation that this function clears and
 * that must contain v_bs_cnt (B ints), the first 4 ints of map_workspace, occ_columns (B*X*Y words) and
 * the first 4 ints of every partition workspace (and the vcount arrays when num_voxels == 0);
 * MSSVT_E_BADARG otherwise.  map_table and the partition tables / scratch tables are pre-filled with -1 by the
 * caller as for the single entry points. */
int mssvt_level_setup(int num_voxels, int batch_size, int x_max, int y_max, int z_max, int hash_size,
                      const int *v_indices, void *zero_region, long long zero_bytes, int *v_bs_cnt, int *map_table,
                      int *map_workspace, unsigned long long *occ_columns, int num_sets, const int *host_win_grid3,
                      const int *host_win_size3, const int *host_max_num_wins, int *const *host_win_ind,
                      int *const *host_tables, int *const *host_scratch_tables, int *const *host_vcount,
                      int *workspaces, long long workspace_stride_ints, void *stream);

/* The same level set-up for a voxel list that is SORTED by (b,x,y,z) -- the order DynamicVFE emits
 * (vfe/dynamic_vfe.py:83-93,114-118: torch.unique over the voxel keys) -- from one occupancy bitmap, without the
 * voxel hash table (K1, ms_sparse_attention_gpu.cu:66-97), without the insert-min / rank passes of K2 (:117-168)
 * and without counting atomics (mssvt_utils.py:35-37), three launches behind one fill (z_max <= 64):
 *   v_bs_cnt (B), sample_start (B+1) rows of every sample; occ_columns (B*X*Y words, bit z);
 *   column_vbase (B*X*Y): voxels of the sample in earlier columns (index of cell (x,y,z) in its sample =
 *   column_vbase + popcount(word below z)); per partition k < num_sets (<= 4): win_ind[k] (num_voxels,4) window rows
 *   [b,wz,wy,wx] in first-occurrence order, tables[k] (B,H,2) pre-filled with -1 or NULL (no table wanted),
 *   vcount[k] (B) windows per sample, ws[k]: 4 header ints ([0] status bits, [1] number of windows).
 * level_status[0] gets ST_UNSORTED (8) when the list is not strictly ascending in (b,x,y,z) or holds an out-of-grid
 * voxel; every partition then reports 0 windows and the caller must use mssvt_level_setup (any order).
 * zero_region / zero_bytes: one caller allocation cleared by this call that contains sample_start, occ_columns,
 * level_status and the ws headers (zero_bytes < 0: |zero_bytes| bytes the caller has cleared itself, e.g. with
 * mssvt_fill_two -- no clear here).  scratch: mssvt_level_sorted_scratch_ints(B, X, Y) ints.                     */
long long mssvt_level_sorted_scratch_ints(int batch_size, int x_max, int y_max);
/* a[0..n_a) = value_a and b[0..n_b) = value_b (int32, both 16-byte aligned) in ONE launch: the -1 prefill of a frame's
 * tables / owner arrays (ref: torch.full(-1) per table, mssvt_utils.py:39, mssvt_ops.py:47) and its zeroed words.    */
int mssvt_fill_two(int *a, long long n_a, int value_a, int *b, long long n_b, int value_b, void *stream);
int mssvt_level_setup_sorted(int num_voxels, int batch_size, int x_max, int y_max, int z_max, int hash_size,
                             const int *v_indices, void *zero_region, long long zero_bytes, int *v_bs_cnt,
                             int *sample_start, unsigned long long *occ_columns, int *column_vbase, int *level_status,
                             int num_sets, const int *host_win_grid3, const int *host_win_size3,
                             const int *host_max_num_wins, int *const *host_win_ind, int *const *host_tables,
                             int *const *host_vcount, int *const *host_ws, int *scratch, void *stream);

/* mssvt_level_setup_sorted that also writes the K4 lists of partition `pillar_set` -- pillar windows [1,1,z], offsets of
 * vox_query_win1 (num_win1 <= 64 rows) with x = y = 0 -- i.e. the outputs of mssvt_window_plan_one(disjoint_lists = 2,
 * with_pad = 0) for that partition (k_ind (cap,max_num_win1), win_vstart, win_cnt, pair_base (cap), pair_win / pair_vox (N);
 * pair_win AND k_ind pre-filled with -1 -- only listed slots are written --; k_ind / pair_base / pair_vox may be NULL:
 * mssvt_compress_fused reads neither; table z offsets in [-32, 31]): every such window is a slab of ONE column's occupancy word, so its list falls out where
 * the window is numbered, without a launch of its own (ref gather_one_window_voxels, ms_sparse_attention_gpu.cu:383-433).
 * MSSVT_E_TOOLARGE: the partition's windows are not pillars.                                                        */
int mssvt_level_setup_sorted_pillars(
    int num_voxels, int batch_size, int x_max, int y_max, int z_max, int hash_size, const int *v_indices, void *zero_region,
    long long zero_bytes, int *v_bs_cnt, int *sample_start, unsigned long long *occ_columns, int *column_vbase,
    int *level_status, int num_sets, const int *host_win_grid3, const int *host_win_size3, const int *host_max_num_wins,
    int *const *host_win_ind, int *const *host_tables, int *const *host_vcount, int *const *host_ws, int *scratch,
    int pillar_set, int max_num_win1, int num_win1, const int *vox_query_win1, int *k_ind, int *win_vstart, int *win_cnt,
    int *pair_base, int *pair_win, int *pair_vox, void *stream);

/* Fused window plan of a two-scale Block: K3 + 2 x K7 + 2 x K8 + the key-mask logic
 * of ref mssvt_backbone.py:247-258 in one launch, one wavefront per window, hit lists
 * kept in LDS.  num_wins_dev: DEVICE scalar (e.g. workspace+1 of
 * mssvt_window_partition_compact); win_capacity: rows allocated in the per-window
 * outputs.  Outputs: ind_odd/ind_even/ind_win1 (cap,max_num_*) as K3 writes them (-1
 * padded); k_ind1/k_ind2 (cap,K) sampled key voxels of the win1 / win2 list (an EMPTY
 * slot picked by FPS becomes voxel 0, as in the reference); k_mask1/k_mask2 (cap,K)
 * bytes, 1 = masked; win_vstart (cap) first feature row of the window's sample;
 * owner_* (N) pre-filled -1: highest flat list slot (w*max_num + s) holding the voxel.
 * Optional resolved metadata (kmeta1 == NULL: skipped; each qmeta_* may be NULL on its own): qmeta_* (cap,max_num_*,4), kmeta1/2
 * (cap,K,4) f32 = (voxel centre - window centre in metres, bits of the global feature row or
 * -1 for empty / masked slots); wcentre (cap,4) = window centre; nq_valid (3,cap) = valid odd /
 * even / win1 entries per window.  indices (N,4) voxel coords.  With the metadata asked for, the list rows ind_*, the key
 * indices / masks k_ind* / k_mask* and the owner_* arrays may each be NULL (the fused consumers read the metadata and the
 * interpolation tables: mssvt_frame_forward passes none of them); the weights of the tables use the hardware's square root
 * and reciprocal (1 ulp each); a voxel with a single candidate (a query list of one slot) gets the weight 1 exactly.
 * column_vbase / level_status_dev (optional, with occ_columns; from mssvt_level_setup_sorted): for a voxel list sorted
 * by (b,x,y,z) the index of an occupied cell is column_vbase + popcount(column word below z) and the hash is not
 * probed at all (xyz_to_vidx may then be NULL); when level_status_dev[0] has ST_UNSORTED (8) set the hash is used.
 * win_counts_dev (optional, B ints: windows per sample, as the window partition reports them): the windows are
 * accepted and unused (a centre-out work order was measured: no gain).
 * num_tabs (0..4) interpolation tables built in the same launch (what mssvt_block_interp_table_multi builds from the
 * finished lists; requires kmeta1 and window lists that cannot overlap, i.e. every voxel owned by one window -- the
 * caller checks the tables): host_tab_list[t] = query list (0 odd, 1 even, 2 win1), host_tab_interp[t] = the Block's
 * use_feature_interpolation, host_tab_zero_row[t] = a row of the attention buffer that holds zeros, host_tab_row[t]
 * (N,4) int32 pre-filled with -1 / host_tab_w[t] (N,4) f32 as for mssvt_block_interp_table.                    */
int mssvt_window_plan_two(
    int x_max, int y_max, int z_max, int x_ws, int y_ws, int z_ws, int max_num_odd, int max_num_even,
    int max_num_win1, int max_num_win2, int hash_size, int batch_size, int num_odd, int num_even,
    int num_win1, int num_win2, const int *vox_query_odd, const int *vox_query_even,
    const int *vox_query_win1, const int *vox_query_win2, int key_num_sample, const int *win_indices,
    const int *num_wins_dev, int win_capacity, const int *xyz_to_vidx, const int *v_bs_cnt,
    int *ind_odd, int *ind_even, int *ind_win1, int *k_ind1, int *k_ind2, unsigned char *k_mask1,
    unsigned char *k_mask2, int *win_vstart, int *owner_win1, int *owner_odd, int *owner_even,
    const int *indices, const float *host_voxel_size3, const float *host_range_min3,
    const float *host_win_size3, float *qmeta_odd, float *qmeta_even, float *qmeta_win1, float *kmeta1,
    float *kmeta2, float *wcentre, int *nq_valid, const unsigned long long *occ_columns,
    const int *host_footprint4, const int *packed_offsets, const int *column_vbase, const int *level_status_dev,
    const int *win_counts_dev, int num_tabs, const int *host_tab_list, const int *host_tab_interp,
    const int *host_tab_zero_row, int *const *host_tab_row, float *const *host_tab_w, void *stream);

/* mssvt_window_plan_two without interpolation tables (the arguments up to win_counts_dev are the same; kmeta1 required):
 * vox_win (N) int32, pre-filled with -1, receives for every voxel of a win1 list the window that lists it -- the input of
 * mssvt_voxel_tables, which builds the tables with one lane per voxel instead of one wavefront per window.  For window
 * lists that cannot overlap (as for num_tabs > 0) whose odd / even entries all lie inside the win1 list:
 * MSSVT_E_TOOLARGE unless max_num_odd <= max_num_win1 and num_odd + max_num_even <= max_num_win1.                */
int mssvt_window_plan_two_vox(
    int x_max, int y_max, int z_max, int x_ws, int y_ws, int z_ws, int max_num_odd, int max_num_even,
    int max_num_win1, int max_num_win2, int hash_size, int batch_size, int num_odd, int num_even,
    int num_win1, int num_win2, const int *vox_query_odd, const int *vox_query_even,
    const int *vox_query_win1, const int *vox_query_win2, int key_num_sample, const int *win_indices,
    const int *num_wins_dev, int win_capacity, const int *xyz_to_vidx, const int *v_bs_cnt,
    int *ind_odd, int *ind_even, int *ind_win1, int *k_ind1, int *k_ind2, unsigned char *k_mask1,
    unsigned char *k_mask2, int *win_vstart, int *owner_win1, int *owner_odd, int *owner_even,
    const int *indices, const float *host_voxel_size3, const float *host_range_min3,
    const float *host_win_size3, float *qmeta_odd, float *qmeta_even, float *qmeta_win1, float *kmeta1,
    float *kmeta2, float *wcentre, int *nq_valid, const unsigned long long *occ_columns,
    const int *host_footprint4, const int *packed_offsets, const int *column_vbase, const int *level_status_dev,
    const int *win_counts_dev, int *vox_win, void *stream);

/* mssvt_window_plan_two_vox that also writes, per window and key scale, whether the key list holds a row in a slot
 * 16 .. key_num_sample-1: live1 / live2 (win_capacity) int32, 1 = such a slot is live, 0 = every live key sits in slots
 * 0 .. 15; written for every window below *num_wins_dev.  Every other output has the bits it has without them. */
int mssvt_window_plan_two_live(
    int x_max, int y_max, int z_max, int x_ws, int y_ws, int z_ws, int max_num_odd, int max_num_even,
    int max_num_win1, int max_num_win2, int hash_size, int batch_size, int num_odd, int num_even,
    int num_win1, int num_win2, const int *vox_query_odd, const int *vox_query_even,
    const int *vox_query_win1, const int *vox_query_win2, int key_num_sample, const int *win_indices,
    const int *num_wins_dev, int win_capacity, const int *xyz_to_vidx, const int *v_bs_cnt,
    int *ind_odd, int *ind_even, int *ind_win1, int *k_ind1, int *k_ind2, unsigned char *k_mask1,
    unsigned char *k_mask2, int *win_vstart, int *owner_win1, int *owner_odd, int *owner_even,
    const int *indices, const float *host_voxel_size3, const float *host_range_min3,
    const float *host_win_size3, float *qmeta_odd, float *qmeta_even, float *qmeta_win1, float *kmeta1,
    float *kmeta2, float *wcentre, int *nq_valid, const unsigned long long *occ_columns,
    const int *host_footprint4, const int *packed_offsets, const int *column_vbase, const int *level_status_dev,
    const int *win_counts_dev, int *vox_win, int *live1, int *live2, void *stream);

/* The interpolation tables of mssvt_window_plan_two(num_tabs > 0), byte for byte, from a finished plan: one lane per
 * (voxel, table).  vox_win from mssvt_window_plan_two_vox; nq_valid (3, win_capacity) and the qmeta of every list a table
 * names from the same plan (.w of a slot = the global feature row of its voxel); indices (N,4); the host_tab_* arrays as
 * for mssvt_window_plan_two.  host_tab_row[t] is written for EVERY voxel ((-1,-1,-1,-1): not updated; no pre-fill
 * needed), host_tab_w[t] for the updated ones.
 * The same launch carries an independent second job when chunk_groups > 0: the chunk ends of mssvt_compress_ws_chunked
 * for a grid of chunk_groups = mssvt_compress_ws_groups(win_capacity of the pillar level) workgroups -- chunk_ends
 * (chunk_groups + 1, 2) int32 (window, row) pairs, non-decreasing, every one a window start, (0, 0) first and
 * (*chunk_num_wins_dev, num_voxels) last, cut by cost (8 per row + 5 per window) from chunk_pair_win (N).  num_tabs = 0
 * with chunk_groups > 0 computes the ends only.  (mssvt_frame_forward runs the same workgroups in front of those of the
 * k_query_rows launch of its work orders instead of in a launch of their own.)                                     */
int mssvt_voxel_tables(int num_voxels, const int *indices, const int *vox_win, const int *nq_valid, int win_capacity,
                       const float *qmeta_odd, const float *qmeta_even, const float *qmeta_win1, int max_num_odd,
                       int max_num_even, int max_num_win1, const float *host_voxel_size3, const float *host_range_min3,
                       int num_tabs, const int *host_tab_list, const int *host_tab_interp, const int *host_tab_zero_row,
                       int *const *host_tab_row, float *const *host_tab_w, int chunk_groups,
                       const int *chunk_num_wins_dev, const int *chunk_pair_win, int *chunk_ends, void *stream);

/* Occupancy columns of a voxel set (z_max <= 64): columns (B*x_max*y_max) 64-bit words, bit z of
 * word (b*x_max + x)*y_max + y set when cell (b,x,y,z) holds a voxel.  Optional input of
 * mssvt_window_plan_two (together with host_footprint4 = {min x offset, min y offset, x extent,
 * y extent} of the four query tables and packed_offsets = the tables concatenated odd | even |
 * win1 | win2, one word (x+64) | (y+64)<<7 | (z+64)<<14 | column<<21 per offset, column = (x - min x) * y extent +
 * (y - min y), on the device; |offset| <= 60, x extent * y extent <= 1024): the K3 hit test then reads one word per (x,y) column of the
 * neighbourhood instead of probing the hash for each of its cells (ref K3 probes all of them,
 * ms_sparse_attention_gpu.cu:193-330); the hash is only probed for the hits.               */
int mssvt_occupancy_columns(const int *indices, int num_voxels, int batch_size, int x_max, int y_max,
                            int z_max, unsigned long long *columns, void *stream);

/* Work order and compact query rows for mssvt_block_attention_group, from one row of the
 * plan's (3,cap) nq_valid (odd / even / win1) and that list's qmeta (cap,nq,4):
 *   perm (cap)          the windows with >= 1 valid query, sorted by descending min(nq_valid, 256) (a counting sort:
 *                       every window with >= 256 queries shares the first bucket; the order inside a bucket is free);
 *   num_active_dev      how many;
 *   q_off (cap)         exclusive prefix sum of nq_valid in window order = first compact
 *                       query row of each window;
 *   qrow_meta (rows,4)  per compact row: the slot's qmeta entry (rel.xyz, bits(feature row));
 *   qrow_src (rows,2)   per compact row: (window, attn row = window * nq + slot);
 *   num_rows_dev        total rows (<= num_voxels: the query lists of one pattern are
 *                       disjoint).  A window whose rows end beyond row_capacity is dropped
 *                       whole, with every window behind it: num_rows_dev = its first row,
 *                       and the attention writes none of its rows.                         */
int mssvt_plan_order(const int *num_wins_dev, const int *nq_valid, int nq, const float *qmeta,
                     int win_capacity, int row_capacity, int *perm, int *num_active_dev, int *q_off,
                     float *qrow_meta, int *qrow_src, int *num_rows_dev, void *stream);

/* mssvt_plan_order for several query lists of one plan in ONE launch pair (host arrays of
 * num_sets <= 4 device pointers / sizes, one entry per list).                                 */
int mssvt_plan_order_multi(int num_sets, const int *num_wins_dev, const int *const *host_nq_valid,
                           const int *host_nq, const float *const *host_qmeta, int win_capacity,
                           int row_capacity, int *const *host_perm, int *const *host_num_active,
                           int *const *host_q_off, float *const *host_qrow_meta, int *const *host_qrow_src,
                           int *const *host_num_rows, void *stream);

/* mssvt_plan_order_multi that also builds, in the same launches, the step lists of mssvt_block_attention_kv16_steps: one
 * per (query list i, head group g), host_steps[i * num_groups + g] (2 x win_capacity) int32 and host_num_steps[..] (1),
 * from the list's nq_valid and host_live[g] (win_capacity; mssvt_window_plan_two_live: 1 = the window needs the upper
 * key tile in group g).  A step is (wA, wB), wB = -1 for one window alone.  Every window of perm is in exactly one step;
 * a pair holds two distinct windows with live == 0 and equal min(nq_valid, 256); steps come in descending order of that
 * count; of the live == 0 windows of one count at most one is alone (who pairs with whom is free).  Nothing is written at
 * or behind step *num_steps.  scratch: mssvt_plan_order_steps_scratch_ints(num_sets, num_groups) ints.
 * num_sets * (1 + num_groups) <= 12 (MSSVT_E_TOOLARGE).  perm, q_off, the rows and the counts as mssvt_plan_order_multi. */
long long mssvt_plan_order_steps_scratch_ints(int num_sets, int num_groups);
int mssvt_plan_order_steps(int num_sets, const int *num_wins_dev, const int *const *host_nq_valid,
                           const int *host_nq, const float *const *host_qmeta, int win_capacity,
                           int row_capacity, int *const *host_perm, int *const *host_num_active,
                           int *const *host_q_off, float *const *host_qrow_meta, int *const *host_qrow_src,
                           int *const *host_num_rows, int num_groups, const int *const *host_live,
                           int *const *host_steps, int *const *host_num_steps, int *scratch, void *stream);

/* Fused attention of a Block, all head groups (group g = channels [c0[g], c0[g]+Cg[g]),
 * Cg = heads[g]*head_dim <= 64, attends to key scale g): gathers + positional MLP +
 * MixedScaleAttention (ref mssvt_backbone.py:260-295, mssvt_utils.py:112-150) for every valid
 * query of every window.  xhat (N,C) = norm1 output; perm / num_active_dev / q_off / qrow_meta /
 * qrow_src / num_rows_dev: from mssvt_plan_order for the query list of this block's cbs_pattern,
 * nq_valid = the row it was built from; host_kmeta[g] (cap,K,4) / wcentre (cap,4): the plan
 * kernel's resolved metadata of key scale g; host_Wq[g] (Cg,Cg), host_Wkv[g] (2Cg,Cg),
 * host_Wo[g] (Cg,Cg) + biases, Wpos (C,6), bpos = the module's parameters (host arrays of device
 * pointers); qbuf: scratch of row_capacity x sum_g 4*ceil(heads[g]/4)*Cg[g] floats handed between
 * the three launches (queries / keys+softmax / output); attn (cap*nq [+1],C): rows of valid
 * query slots are written.  Groups of equal width share the launches (grid.y = group).
 * C and every c0 must be multiples of 4.                                                  */
int mssvt_block_attention(
    int C, int num_groups, const int *host_c0, const int *host_cg, const int *host_heads, int head_dim, float scale,
    int nq, int key_num_sample, const float *xhat, const int *num_active_dev, const int *perm, const int *q_off,
    const int *nq_valid, const int *num_rows_dev, int row_capacity, const float *qrow_meta, const int *qrow_src,
    const float *const *host_kmeta, const float *wcentre, const float *const *host_Wq, const float *const *host_bq,
    const float *const *host_Wkv, const float *const *host_bkv, const float *const *host_Wo,
    const float *const *host_bo, const float *Wpos, const float *bpos, float *qbuf, float *attn, void *stream);

/* mssvt_block_attention with split-fp16 matrix operands: every product sum as three v_mfma_f32_16x16x32_f16 on
 * (hi, lo = 2^11 (v - hi)) fp16 halves with fp32 accumulation -- the fp32 instruction's error at ~1/4 of its cycles.
 * The per-window launch (k_attn_kvh: scores, weighted key sum; Qt crosses qbuf pre-split, same bytes) always; the
 * two row-tiled launches (k_attn_q16 / k_attn_o16) when host_packed gives one mssvt_attn_pack_weights blob per head
 * group (head_dim 16), else they keep the fp32 instruction (host_packed may be NULL).  With the blobs and
 * key_num_sample <= 32 only Q' crosses qbuf (a quarter of the bytes) and the window launch forms Qt = (scale Wk_h)^T q'_h
 * itself from the blob's head-pair fragments, its softmax in base 2 (log2 e folded into them).  Same arguments and results (to
 * the fp32 tolerance) as mssvt_block_attention; shapes outside Cg % 32 == 0, 16 < key_num_sample <= 64 run the fp32
 * form.  The CALLER guarantees the fp16 range of key tokens, Q', Qt, Xbar, V (mssvt_amd/fused.py, _attn_kv16_ok). */
int mssvt_block_attention_kv16(
    int C, int num_groups, const int *host_c0, const int *host_cg, const int *host_heads, int head_dim, float scale,
    int nq, int key_num_sample, const float *xhat, const int *num_active_dev, const int *perm, const int *q_off,
    const int *nq_valid, const int *num_rows_dev, int row_capacity, const float *qrow_meta, const int *qrow_src,
    const float *const *host_kmeta, const float *wcentre, const float *const *host_Wq, const float *const *host_bq,
    const float *const *host_Wkv, const float *const *host_bkv, const float *const *host_Wo,
    const float *const *host_bo, const float *Wpos, const float *bpos, float *qbuf, float *attn,
    const void *const *host_packed, void *stream);

/* mssvt_block_attention_kv16 whose window launch walks the step lists of mssvt_plan_order_steps (host_steps[g] /
 * host_num_steps[g]: head group g's list of this block's query pattern): the two windows of a step share a wavefront, window
 * B's key slots 0 .. 15 in the upper key tile, each column masking the other window's tile.  The attention rows have the
 * bits of mssvt_block_attention_kv16 on the same inputs.  Only the Q' hand-off form takes pairs (host_packed blobs for
 * every group, head_dim 16, 16 < key_num_sample <= 32, equal group widths): MSSVT_E_TOOLARGE otherwise, nothing launched. */
int mssvt_block_attention_kv16_steps(
    int C, int num_groups, const int *host_c0, const int *host_cg, const int *host_heads, int head_dim, float scale,
    int nq, int key_num_sample, const float *xhat, const int *num_active_dev, const int *perm, const int *q_off,
    const int *nq_valid, const int *num_rows_dev, int row_capacity, const float *qrow_meta, const int *qrow_src,
    const float *const *host_kmeta, const float *wcentre, const float *const *host_Wq, const float *const *host_bq,
    const float *const *host_Wkv, const float *const *host_bkv, const float *const *host_Wo,
    const float *const *host_bo, const float *Wpos, const float *bpos, float *qbuf, float *attn,
    const void *const *host_packed, const int *const *host_steps, const int *const *host_num_steps, void *stream);

/* Split-fp16 fragments of one head group's projections for mssvt_block_attention_kv16, in MFMA operand order: Wq
 * (Cg,Cg), Wkv (2Cg,Cg: K rows then V rows; the softmax scale folded into the K fragments, scale x log2 e into their
 * head-pair copy), Wo (Cg,Cg) -- nn.Linear layouts of ref mssvt_utils.py:92-103.  Once per parameter version.  mssvt_attn_packed_bytes: size of `packed`, 0 = shape not
 * instantiated (head_dim 16, Cg 32 / 64).                                                                          */
long long mssvt_attn_packed_bytes(int Cg, int head_dim);
int mssvt_attn_pack_weights(int Cg, int head_dim, float scale, const float *Wq, const float *Wkv, const float *Wo,
                            void *packed, void *stream);

/* mssvt_block_attention with bf16 matrix-core operands (BASELINE configs[2]; an extension of this build -- the
 * reference's MixedScaleAttention computes in fp32, ref mssvt_utils.py:112-150): ONE launch, one wavefront per
 * (window, head group); keys and values are projected inside the kernel (v_mfma_f32_16x16x32_bf16), so there is
 * no qbuf hand-off.  Tokens, weights, Q', K', V', P and O are rounded to bf16 as MFMA operands; accumulation,
 * softmax, biases, the positional MLP and the attention rows written stay fp32.  Same arguments as
 * mssvt_block_attention minus qbuf.  MSSVT_E_TOOLARGE: shape not instantiated (use the fp32 entry point).   */
int mssvt_block_attention_bf16(
    int C, int num_groups, const int *host_c0, const int *host_cg, const int *host_heads, int head_dim, float scale,
    int nq, int key_num_sample, const float *xhat, const int *num_active_dev, const int *perm, const int *q_off,
    const int *nq_valid, const int *num_rows_dev, int row_capacity, const float *qrow_meta, const int *qrow_src,
    const float *const *host_kmeta, const float *wcentre, const float *const *host_Wq, const float *const *host_bq,
    const float *const *host_Wkv, const float *const *host_bkv, const float *const *host_Wo,
    const float *const *host_bo, const float *Wpos, const float *bpos, float *attn, void *stream);

/* 3-NN inverse-distance interpolation of the attention rows onto the win1 voxels (K9,
 * K10, ref mssvt_backbone.py:298-311) + scatter + first residual (ref :313-338):
 * x_new[v] = interp(v) + x_in[v] for every voxel v owned by a list slot; rows of other
 * voxels are left untouched (the caller pre-fills x_new = 2*x_in, ref quirk R12).
 * use_interpolation = 0: x_new[v] = attn[slot] + x_in[v] for the query voxels only.   */
int mssvt_block_interp_scatter(int C, int nq, int n_upd, int use_interpolation, const float *attn,
                               const float *x_in, float *x_new, const int *indices,
                               const int *win_ind, const int *num_wins_dev, int win_capacity,
                               const int *win_vstart, const int *q_ind, const int *upd_ind,
                               const int *owner, const float *host_voxel_size3,
                               const float *host_range_min3, void *stream);

/* ---- CompressBlock fast path (ref mssvt_backbone.py:351-398): ragged pieces ---------
 * K4 list per window + allocation of one "pair row" per valid (window, slot) (+ one PAD
 * row per window if with_pad).  k_ind (cap,max_num_win1) as K4 writes it; win_cnt (cap)
 * valid slots; pair_base (cap); pair_win / pair_vox (row capacity) window id and global
 * voxel row (-1 = pad) of every pair row.  disjoint_lists != 0 (no voxel in two lists: odd
 * window sizes): pair row = the voxel's feature row, pad row of window w = num_voxels + w,
 * pair_win must be pre-filled with -1, pair_base = -1.  Otherwise rows are reserved through
 * counters[0] (= rows handed out; cleared by this call) and pair_base[w] is the window's
 * first row.  With disjoint lists counters[0] is not touched.
 * occ_columns / column_vbase / level_status_dev (optional, all or none; mssvt_level_setup_sorted): sorted voxel
 * list -> occupancy bit = hit, column base + popcount below z = voxel index, the hash is not probed
 * (xyz_to_vidx may be NULL) unless level_status_dev[0] has ST_UNSORTED (8) set.
 * disjoint_lists == 2: disjoint AND every table offset has x = y = 0 (the caller checked): with x_ws = y_ws = 1 on a
 * sorted level the lists are built one LANE per window from the column words (pillar windows).        */
int mssvt_window_plan_one(int x_max, int y_max, int z_max, int x_ws, int y_ws, int z_ws,
                          int max_num_win1, int hash_size, int num_win1, const int *vox_query_win1,
                          const int *win_indices, const int *num_wins_dev, int win_capacity,
                          const int *xyz_to_vidx, const int *v_bs_cnt, int with_pad,
                          int disjoint_lists, int num_voxels, int *k_ind, int *win_vstart, int *win_cnt,
                          int *pair_base, int *pair_win, int *pair_vox, int *counters,
                          const unsigned long long *occ_columns, const int *column_vbase,
                          const int *level_status_dev, void *stream);
/* out (R,C) = relu(W1 [voxel centre - window centre ; window centre] + b1) per pair row
 * (first layer of pos_proj, ref :49-54, :372-373).                                     */
int mssvt_compress_pos1(int C, const int *num_rows_dev, int row_capacity, const int *pair_win,
                        const int *pair_vox, const int *indices, const int *win_indices,
                        const float *host_voxel_size3, const float *host_range_min3,
                        const float *host_win_size3, const float *W1, const float *b1, float *out,
                        void *stream);
/* rows[r] += xhat[pair_vox[r]] for non-pad rows (key token = feature + positional emb.). */
int mssvt_compress_add_features(int C, const int *num_rows_dev, int row_capacity, const int *pair_vox,
                                const float *xhat, float *rows, void *stream);
/* q_tok (nw,C) = channel-wise max over the window's zero-padded key features (ref :370). */
int mssvt_compress_pool(int C, int max_num_win1, const int *num_wins_dev, int win_capacity,
                        const int *k_ind, const int *win_vstart, const int *win_cnt, const float *xhat,
                        float *q_tok, void *stream);
/* nq=1 attention of head group `group` (channels [c0,c0+Cg), list slots
 * [group*keys_per_group, (group+1)*keys_per_group)): qp (nw,C) projected queries,
 * kv (R,2*Cg) = [K|V] rows of this group's to_kvs for every pair row -> out (nw,C)
 * columns [c0,c0+Cg) (before the output projection).                                   */
int mssvt_compress_attention_group(int C, int c0, int Cg, int head_dim, float scale,
                                   int keys_per_group, int group, int with_pad, int max_num_win1,
                                   int num_voxels, const int *num_wins_dev, int win_capacity,
                                   const int *win_cnt, const int *pair_base, const int *k_ind,
                                   const int *win_vstart, const float *qp, const float *kv, float *out,
                                   void *stream);

/* CompressBlock attention up to (not including) the FFN tail, for ONE head group and
 * non-overlapping window lists (ref mssvt_backbone.py:351-383; MixedScaleAttention
 * mssvt_utils.py:112-150), four launches on the fp32 matrix cores, every count read on the
 * device (no host synchronisation):  out (nw,C) = projs( softmax_v( scale (Wq max_v xhat_v + bq)
 * . (Wk k_v + bk) ) (Wv k_v + bv) ),  k_v = xhat_v + pos_proj([centre_v - centre_w ; centre_w]).
 * k_ind / win_vstart / win_cnt / pair_win: from mssvt_window_plan_one with disjoint_lists = 1,
 * with_pad = 0.  Wpos1 (C,6), Wpos2 (C,C), Wq (C,C), Wkv (2C,C), Wo (C,C) + biases: the module's
 * parameters.  Scratch: qp (win_capacity,C), ktok (N,C), score (N,C/head_dim), vp (N,C).
 * split_f16 != 0: the C x C products with every fp32 operand split into two fp16 halves (22 of 24 mantissa bits)
 * (3 x v_mfma_f32_16x16x32_f16, fp32 accumulation: the fp32 instruction's error at 3/16 of its
 * cycles); the CALLER guarantees the fp16 range of xhat, the positional hidden layer, the key
 * tokens and the V rows (mssvt_amd/fused.py bounds them from the parameters), else pass 0.
 * Instantiated for C in {32,64,128}, head_dim in {8,16,32} (C/head_dim <= 8).               */
int mssvt_compress_fused(
    int C, int head_dim, float scale, int max_num_win1, int num_voxels, const int *num_wins_dev, int win_capacity,
    const int *win_ind, const int *indices, const int *k_ind, const int *win_vstart, const int *win_cnt,
    const int *pair_win, const float *host_voxel_size3, const float *host_range_min3, const float *host_win_size3,
    const float *xhat, const float *Wpos1, const float *bpos1, const float *Wpos2, const float *bpos2,
    const float *Wq, const float *bq, const float *Wkv, const float *bkv, const float *Wo, const float *bo,
    float *qp, float *ktok, float *score, float *vp, float *out, int split_f16, void *stream);

/* The same attention (same inputs, same `out`) in ONE launch and without any scratch, for the case the detector runs:
 * a level set up as SORTED (mssvt_level_setup_sorted*: windows are numbered in row order), pillar windows x_ws = y_ws = 1
 * (window cell = (x, y, z / z_ws): the window rows are not read) whose lists cannot be truncated (z_ws <= max_num_win1 <= 32),
 * so that every window is one run of consecutive voxel rows and
 * consecutive windows are consecutive runs; one head group, head_dim 16, C = 128; split-fp16 products (the caller
 * guarantees the fp16 range exactly as for mssvt_compress_fused(split_f16 = 1)).  One workgroup per CU keeps pos_proj.2, Wk
 * and Wv as MFMA fragments in registers (wave h = head h), Wq / Wo in LDS; the key tokens, K, V, the scores and the
 * projected queries never leave the CU (csrc/compress_ws.hip).  packed: mssvt_compress_ws_packed_bytes(C) bytes written by
 * mssvt_compress_ws_pack from pos_proj.2 (C,C), to_q (C,C), to_kv (2C,C), proj (C,C) -- once per parameter version.
 * Of the K4 plan it reads win_cnt and pair_win only (the lists themselves are runs of rows).
 * MSSVT_E_TOOLARGE: shape not covered (use mssvt_compress_fused).  Deterministic; differs from mssvt_compress_fused by the
 * association of the softmax sums only.                                                                              */
long long mssvt_compress_ws_packed_bytes(int C);
int mssvt_compress_ws_pack(int C, const float *Wpos2, const float *Wq, const float *Wkv, const float *Wo, void *packed,
                           void *stream);
int mssvt_compress_ws(int C, int head_dim, float scale, int z_ws, int max_num_win1, int num_voxels, const int *num_wins_dev,
                      int win_capacity, const int *indices, const int *win_cnt, const int *pair_win,
                      const float *host_voxel_size3, const float *host_range_min3, const float *host_win_size3,
                      const float *xhat, const float *Wpos1, const float *bpos1, const float *bpos2, const float *bq,
                      const float *bkv, const float *bo, const void *packed, float *out, void *stream);
/* The same with the chunks of the level handed in: every workgroup of mssvt_compress_ws finds its chunk (consecutive windows
 * holding 1 / grid of the cost) by a search of its own; chunk_ends (chunk_groups + 1, 2) from mssvt_voxel_tables replaces the
 * search (chunk_groups must equal mssvt_compress_ws_groups(win_capacity), the number of workgroups; NULL: search).  The
 * output does not depend on where the chunks are cut.                                                            */
int mssvt_compress_ws_groups(int win_capacity);
int mssvt_compress_ws_chunked(int C, int head_dim, float scale, int z_ws, int max_num_win1, int num_voxels,
                              const int *num_wins_dev, int win_capacity, const int *indices, const int *win_cnt,
                              const int *pair_win, const float *host_voxel_size3, const float *host_range_min3,
                              const float *host_win_size3, const float *xhat, const float *Wpos1, const float *bpos1,
                              const float *bpos2, const float *bq, const float *bkv, const float *bo, const void *packed,
                              float *out, const int *chunk_ends, int chunk_groups, void *stream);

/* Backward of mssvt_layer_norm (training path; autograd's LayerNorm backward in the reference): dx (N,C), dweight (C),
 * dbias (C) from x, dy; mean / rstd are recomputed.  The column sums are per-workgroup partial rows in `workspace`
 * (512 * 2 * C floats) added in workgroup order: deterministic.  C in {16,32,64,128,256}.                      */
int mssvt_layer_norm_backward(const float *x, const float *dy, int num_rows, int C, const float *weight, float eps,
                              float *dx, float *dweight, float *dbias, float *workspace, void *stream);
/* The same with dx = (LayerNorm backward of dy) + dres: dres (N,C) or NULL = the gradient that reaches x through its
 * other uses (the residual connection around the normalised branch: ref mssvt_backbone.py:241, :339-343) -- the add
 * autograd would run as a pass of its own.                                                                       */
int mssvt_layer_norm_backward_residual(const float *x, const float *dy, const float *dres, int num_rows, int C,
                                       const float *weight, float eps, float *dx, float *dweight, float *dbias,
                                       float *workspace, void *stream);

/* Rows per sample of a (N,4) [b,z,y,x] int32 index tensor -> counts (B) int32, on the device
 * (ref: the host loops with .item() of mssvt_utils.py:35-37 / mssvt_backbone.py:124-130).   */
int mssvt_batch_counts(const int *indices, int num_rows, int batch_size, int *counts, void *stream);

/* y = LayerNorm(x) over the last dimension (N,C) f32, C in {16,32,64,128,256}
 * (ref: norm1, mssvt_backbone.py:241); MSSVT_E_TOOLARGE otherwise.                          */
int mssvt_layer_norm(const float *x, int num_rows, int C, const float *weight, const float *bias,
                     float eps, float *y, void *stream);

/* Fused feed-forward tail of a block on the fp32 matrix cores (ref mssvt_backbone.py:336-343,
 * :383-387): x = owner && owner[v] < 0 ? 2*x_in[v] : x_new[v];
 * y = x + linear2(relu(linear1(norm(x)))); optionally y_norm = next_norm(y) (the next block's
 * norm1).  x_new/x_in/y/y_norm (N,C) f32; W1 (FF,C), W2 (C,FF) as in nn.Linear.
 * phases 3 (fp32 matrix instruction): hidden = scratch of n_rows x FF floats, two launches with LDS-resident
 * weights (GEMM1 | GEMM2, the hidden activations make one round trip through `hidden`; hidden NULL ->
 * MSSVT_E_BADARG).  num_rows_dev (optional): the row count is read on the device and n_rows is only the
 * capacity.  phases 1 = only the first launch (LayerNorm + GEMM1 + ReLU -> hidden, x parked in y), 2 = only
 * the second (GEMM2 + residual + next norm) -- for measurement.
 * phases 4 (num_rows_dev allowed; hidden = NULL, or the fragments written by
 * mssvt_ffn_pack_weights for these W1 / W2: saves the in-kernel split): ONE launch with register-stationary weights
 * and every fp32 operand split into two fp16 halves (22 of 24 mantissa bits) (3 x v_mfma_f32_16x16x32_f16 per
 * product sum, fp32 accumulation: the fp32 kernels' error against float64 at 3/16 of the matrix
 * cycles; no hidden round trip).  The CALLER guarantees the fp16 range: sqrt(C) max|norm_w| +
 * max|norm_b| and max_h(|W1_h|_1 * that + |b1_h|) below 6e4 (fused.FFN_F16_LIMIT; mssvt_amd/fused.py checks the
 * parameters once per version and keeps phases 3 otherwise).
 * Instantiated for (C,FF) in {(128,256),(64,128),(32,64)}; MSSVT_E_TOOLARGE otherwise.   */
int mssvt_ffn_fused(int n_rows, int C, int FF, const float *x_new, const float *x_in, const int *owner,
                    const float *norm_w, const float *norm_b, float eps, const float *W1,
                    const float *b1, const float *W2, const float *b2, float *y,
                    const float *next_norm_w, const float *next_norm_b, float next_eps, float *y_norm,
                    float *hidden, const int *num_rows_dev, int phases, void *stream);

/* W1 / W2 of mssvt_ffn_fused split into fp16 (hi, lo) MFMA fragments, once per parameter version: `packed` of
 * mssvt_ffn_packed_bytes(C, FF) bytes (0: shape not instantiated), passed as `hidden` with phases 4.          */
long long mssvt_ffn_packed_bytes(int C, int FF);
int mssvt_ffn_pack_weights(int C, int FF, const float *W1, const float *W2, void *packed, void *stream);

/* Table form of mssvt_block_interp_scatter: for every voxel owned by a list slot, tab_row (N,4)
 * int32 = the three rows of `attn` (row = w*nq + slot; empty slots / zero weights -> zero_row) and
 * tab_w (N,4) f32 = their inverse-distance weights.  The caller pre-fills tab_row with -1
 * (= voxel owned by no slot).                                                            */
int mssvt_block_interp_table(int nq, int n_upd, int use_interpolation, const int *indices,
                             const int *win_ind, const int *num_wins_dev, int win_capacity,
                             const int *win_vstart, const int *q_ind, const int *upd_ind,
                             const int *owner, const float *host_voxel_size3,
                             const float *host_range_min3, int zero_row, int *tab_row, float *tab_w,
                             void *stream);
/* mssvt_block_interp_table for several (query list, interpolation mode) variants of one plan in
 * ONE launch (host arrays of num_sets <= 4 entries).                                          */
int mssvt_block_interp_table_multi(int num_sets, const int *host_nq, const int *host_n_upd,
                                   const int *host_interp, const int *indices, const int *win_ind,
                                   const int *num_wins_dev, int win_capacity, const int *win_vstart,
                                   const int *const *host_q_ind, const int *const *host_upd_ind,
                                   const int *const *host_owner, const float *host_voxel_size3,
                                   const float *host_range_min3, const int *host_zero_row,
                                   int *const *host_tab_row, float *const *host_tab_w, void *stream);
/* mssvt_ffn_fused fed by that table: x = tab_row[v][0] < 0 ? 2*x_in[v]
 *                                      : x_in[v] + sum_i tab_w[v][i] * attn[tab_row[v][i]].
 * y may be NULL when phases == 4 and y_norm is given (round 6): only the next LayerNorm's output is stored -- the last
 * Block in front of a CompressBlock, which has no input residual (ref mssvt_backbone.py:370-385).                    */
int mssvt_ffn_fused_interp(int n_rows, int C, int FF, const float *x_in, const int *tab_row,
                           const float *tab_w, const float *attn, const float *norm_w,
                           const float *norm_b, float eps, const float *W1, const float *b1,
                           const float *W2, const float *b2, float *y, const float *next_norm_w,
                           const float *next_norm_b, float next_eps, float *y_norm, float *hidden,
                           const int *num_rows_dev, int phases, void *stream);

/* ======================================================================== *
 * Part 3 -- voxelizer front-end: the index part of
 *           DynamicVFE.forward (ref pcdet/models/backbones_3d/vfe/dynamic_vfe.py:83-93,
 *           114-118) without a sort: occupancy bitmap + popcount rank.
 * ======================================================================== */

/* int32 words of workspace for a (batch_size, X, Y, Z) grid. */
long long mssvt_voxelize_workspace_ints(int batch_size, int X, int Y, int Z);

/* points (P, point_stride) f32 rows [b, x, y, z, ...] -> voxel_coords (capacity,4) int32 rows
 * [b,z,y,x], sorted by (b,x,y,z) exactly like torch.unique of the reference's linear key;
 * point_voxel (P) int32 (nullable) = index of the point's voxel, -1 if outside the grid;
 * num_voxels_dev: device int receiving the voxel count.  host_*3: HOST float[3].          */
int mssvt_voxelize(const float *points, int point_stride, long long num_points, int batch_size,
                   const float *host_range_min3, const float *host_voxel_size3, int X, int Y, int Z,
                   int voxel_capacity, int *voxel_coords, int *point_voxel, int *num_voxels_dev,
                   int *workspace, void *stream);

/* Per-voxel reductions of DynamicVFE without torch_scatter (ref dynamic_vfe.py:98,111,128-129);
 * point_voxel (P) = unq_inv of mssvt_voxelize (-1: point outside the grid).
 * mssvt_voxel_mean_xyz: mean3 (N,3) f32 = scatter_mean of the x,y,z columns (points rows
 *   [b,x,y,z,...]); count (N) points per voxel; scratch_sum3: N*3 64-bit words (fixed-point
 *   sums, 2^-20 m: order independent -> deterministic).
 * mssvt_voxel_max: out (N,F) f32 = scatter_max of features (P,F) (voxels without a point: -inf). */
int mssvt_voxel_mean_xyz(const float *points, int point_stride, long long num_points,
                         const int *point_voxel, int num_voxels, float *mean3, int *count,
                         long long *scratch_sum3, void *stream);
int mssvt_voxel_max(const float *features, int F, long long num_points, const int *point_voxel,
                    int num_voxels, float *out, void *stream);

/* ======================================================================== *
 * Part 4 -- dense output: SparseTensor.dense() + the view of
 *           HeightCompression (ref mssvt_utils.py:6-19,50-62; height_compression.py:41-45) in one pass.
 * out (B, C, Z, Y, X) f32 (= (B, C*Z, Y, X) for the BEV backbone), every element written (zeros for empty
 * cells): out[b, c, z, y, x] = features[row(b,x,y,z), c] where the row comes from the set's hash table
 * map_table (B,H,2) (key x*Y*Z + y*Z + z -> row within the sample; v_bs_cnt (B) rows per sample).
 * ======================================================================== */
int mssvt_dense_bev(const float *features, int C, const int *map_table, int hash_size, const int *v_bs_cnt,
                    int batch_size, int x_max, int y_max, int z_max, float *out, void *stream);

/* The same grid in channels-last memory (csrc/dense_bev.hip, k_dense_bev_nhwc), the hand-over to mssvt_bev_conv:
 * out (B, Y, X, C*Z) f32 with channel c*Z + z -- the memory of dense().view(B, C*Z, Y, X) (ref height_compression.py:41-45)
 * in torch.channels_last.  Every element written (a cell is a full row copy or zeros), bit-exact against mssvt_dense_bev.
 * C % 4 == 0 (MSSVT_E_TOOLARGE otherwise); features and out 16-byte aligned.                                          */
int mssvt_dense_bev_nhwc(const float *features, int C, const int *map_table, int hash_size, const int *v_bs_cnt,
                         int batch_size, int x_max, int y_max, int z_max, float *out, void *stream);

/* Deterministic segmented row sum -- replaces the atomicAdd accumulation of the reference's gather backward passes
 * (ref: group_features_grad_kernel_stack, pcdet/ops/mssvt/src/group_features_gpu.cu:15-47;
 * gather_points_grad_kernel_fast, pcdet/ops/pointnet2/pointnet2_batch/src/sampling_gpu.cu:53-90;
 * group_points_grad_kernel_fast, .../group_points_gpu.cu:14-50), whose sum order changes run to run:
 *   dst[d][0..C) = sum over e in [csr_off[d], csr_off[d+1]) of (csr_w ? csr_w[e] : 1) * src[csr_idx[e]][0..C),
 * added in ascending e (an inverted index of the gather, built once per index set), so gradients are bit-identical
 * from run to run.  csr_off (n_dst+1) int32, csr_idx (nnz) int32 rows of src, csr_w (nnz) f32 or NULL,
 * src (R,C) f32, dst (n_dst,C) f32 (every row written; C % 4 == 0).  Also the forward of a weighted row gather. */
int mssvt_segment_sum_rows(int C, int n_dst, const int *csr_off, const int *csr_idx, const float *csr_w,
                           const float *src, float *dst, void *stream);

/* The same sum over explicit entry ranges [seg_start[d], seg_end[d]) (an empty range writes a zero row): lets the
 * caller cut a destination with thousands of contributions -- e.g. voxel 0 of a sample, the target of every FPS-picked
 * empty slot (ref mssvt_backbone.py:253-256) -- into fixed chunks summed by separate lane groups, and add the chunk
 * sums in chunk order with a second call: the order stays fixed, no lane group runs for the whole launch.       */
int mssvt_segment_sum_rows_ranges(int C, int n_dst, const int *seg_start, const int *seg_end, const int *csr_idx,
                                  const float *csr_w, const float *src, float *dst, void *stream);

/* The same sum on C columns of wider rows: src / dst row strides in floats (multiples of 4, >= C; both pointers at the
 * first of the C columns), and dst either written (accumulate 0) or added to (1: dst[d] = dst[d] + sum, one add per
 * element).  The gradient of a gather of a column range -- a head group of a Block, ref mssvt_backbone.py:260-268 --
 * lands in that range of the full-width gradient without a zero-filled temporary and an add.                    */
int mssvt_segment_sum_rows_strided(int C, int n_dst, const int *seg_start, const int *seg_end, const int *csr_idx,
                                   const float *csr_w, const float *src, int src_stride, float *dst, int dst_stride,
                                   int accumulate, void *stream);

/* The same sum with a residual epilogue: dst[d] = row_a[d] * res[d] + row_b[d] * sum (res, dst (n_dst,C); row_a, row_b
 * (n_dst) f32).  The tail of a Block under autograd in one launch -- 3-NN interpolation of the attention rows, the
 * "untouched voxels keep x_in" select, DropPath and the residual add (ref mssvt_backbone.py:298-340): row_b = the
 * row's DropPath factor, row_a = 1 for a voxel the attention updates, 1 + row_b for one it does not.               */
int mssvt_segment_sum_rows_residual(int C, int n_dst, const int *seg_start, const int *seg_end, const int *csr_idx,
                                    const float *csr_w, const float *src, const float *res, const float *row_a,
                                    const float *row_b, float *dst, void *stream);

/* Tokens of a Block's attention on compact rows (training path):
 *   tok[r][c] = (src ? src[rows[r]][c0+c] : 0) + relu(b[c0+c] + sum_{j<6} W6[c0+c][j] geo8[r][j]),  r < M, c < cg
 * = gathered feature + positional embedding of (offset to the window centre, window centre) (ref pos_proj,
 * mssvt_backbone.py:43-47, token sums :270-285; padded gathers group_features_gpu.cu:52-84, group_points_gpu.cu:56-91).
 * src (N,C) f32 or NULL, rows (M) int32, geo8 (M,8) f32 (columns 6, 7 unused), W6 (Ctot,6) / b (Ctot) = the Conv1d(6,C,1)
 * parameters, tok (M,cg) f32; cg in {16,32,64,128,256}, c0 % 4 == 0.
 * Backward of the embedding: _partial writes the slab of one token set (mssvt_train_tok_slab_floats(M,cg) floats) from
 * dtok (M,cg), the ReLU mask recomputed from geo8; _reduce adds the slabs of up to 4 token sets (host arrays: rows M,
 * first channel c0, width cg, slab address per set; sets with M <= 0 are skipped) in a fixed order into dW6 (C,6) and
 * db (C) (channels no set covers get 0).  The gradient of src is mssvt_segment_sum_rows_strided over the inverted
 * index of `rows`.  No atomics: bit-identical run to run.                                                        */
int mssvt_train_tok_forward(int M, int C, int c0, int cg, const int *rows, const float *src, const float *geo8,
                            const float *W6, const float *b, float *tok, void *stream);
long long mssvt_train_tok_slab_floats(int M, int cg);
int mssvt_train_tok_backward_partial(int M, int c0, int cg, const float *geo8, const float *W6, const float *b,
                                     const float *dtok, float *slab, void *stream);
int mssvt_train_tok_backward_reduce(int C, int num_sets, const int *host_M, const int *host_c0, const int *host_cg,
                                    const float *const *host_slabs, float *dW, float *db, void *stream);

/* Compact key sets of a window plan (index work of the training path; the padded key lists of ref
 * mssvt_backbone.py:253-268 without their empty slots).  kmeta (cap,K,4) f32 = per key slot (offset to the window centre
 * xyz, voxel row as int bits, < 0: empty), as mssvt_window_plan_two leaves it; K <= 64.
 * _counts: cnt[w] = valid slots of window w (0 for w >= *num_wins_dev), *total_dev += their sum (zero it first).
 * _compact: with off = the exclusive prefix sum of cnt, slot k of window w goes to position off[w] + (valid slots before
 * k): k_rows (voxel row), k_win (window), k_geo8 (8 f32: offset xyz, centre xyz from wcentre (cap,4), 0, 0 -- the
 * positional embedding's inputs for mssvt_train_tok_forward).                                                    */
int mssvt_train_key_counts(int cap, int K, const int *num_wins_dev, const float *kmeta, int *cnt, int *total_dev,
                           void *stream);
int mssvt_train_key_compact(int num_wins, int K, const float *kmeta, const float *wcentre, const int *off, int *k_rows,
                            int *k_win, float *k_geo8, void *stream);

/* The table of mssvt_block_interp_table (tab_row4 / tab_w4 (N,4): three rows of the padded attention buffer + weights per
 * voxel, row < 0 in .x: a voxel the attention does not update) in compact form for the training path: idx3 / w3 (3 per
 * voxel) name compact attention rows through inv (padded row -> compact row); an untouched voxel gets row R (the zero
 * row) with weight 0; owned (N) bytes = 1 where the attention updates the voxel (ref mssvt_backbone.py:298-338).   */
int mssvt_train_interp_compact(int N, int R, const int *inv, const int *tab_row4, const float *tab_w4, int *idx3, float *w3,
                               unsigned char *owned, void *stream);

/* Compact (window, voxel) pairs of a CompressBlock's window lists (training path; index work): k_ind (num_wins,ns) int32 =
 * positions inside the window's run of voxel rows, < 0: empty (mssvt_window_plan_one), ns <= 64.  _counts: cnt[w] = valid
 * slots, *total_dev += their sum (zero it first).  _compact, with off = the exclusive prefix sum of cnt: pair_vox (voxel
 * row win_vstart[w] + k), pair_win, geo8 (8 f32: voxel centre - window centre, window centre, 0, 0; centres as
 * (index + 0.5) * cell + min in three rounded fp32 operations, ref with_coords mssvt_backbone.py:132-137) at the prefix
 * position of the slot.  indices (N,4) / win_ind (num_wins,4) int32 (b,z,y,x).                                    */
int mssvt_train_list_counts(int num_wins, int ns, const int *k_ind, int *cnt, int *total_dev, void *stream);
int mssvt_train_pairs_compact(int num_wins, int ns, const int *k_ind, const int *win_vstart, const int *off,
                              const int *indices, const int *win_ind, const float *host_voxel_size3,
                              const float *host_range_min3, const float *host_win_size3, int *pair_vox, int *pair_win,
                              float *geo8, void *stream);

/* Compact query rows of a query pattern of a window plan (training path; index work): from what mssvt_plan_order leaves
 * (row_meta (rows,4) f32 = offset to the window centre xyz + voxel row as int bits; row_src (rows,2) int32 = window,
 * padded attention row) the voxel rows q_rows (R) and the positional embedding's inputs q_geo8 (R,8: offset, centre from
 * wcentre (cap,4), 0, 0) of the first R rows.                                                                    */
int mssvt_train_query_sets(int R, const float *row_meta, const int *row_src, const float *wcentre, int *q_rows,
                           float *q_geo8, void *stream);

/* Inverse of a gather of DISTINCT rows (dst[i] = src[idx[i]], every source row named at most once: a window's query rows
 * when every window size is odd, the voxels of disjoint windows) as ranges for mssvt_segment_sum_rows_ranges over the
 * n_src source rows: seg_start[v] = v, seg_end[v] = bwd_end[v] (v + 1 or v), csr_idx = bwd_idx.  inv_scratch: n_src ints.
 * Replaces the sort of mssvt_csr_transpose for such gathers (the reference's atomicAdd backward needs no order there). */
int mssvt_train_unique_inverse(int nnz, int n_src, const int *idx, int *inv_scratch, int *bwd_idx, int *bwd_end,
                               void *stream);

/* ========================================================================
 * Post-processing behind the backbone: rotated BEV NMS of CenterHead's boxes.
 * ref: iou3d_nms_cuda.nms_gpu, pcdet/ops/iou3d_nms/src/iou3d_nms.cpp:90-135 (host loop) +
 * iou3d_nms_kernel.cu:107-278 (box_overlap / iou_bev / nms_kernel).  boxes_sorted (N,7) f32
 * [x,y,z,dx,dy,dz,heading] in descending score order (the caller sorts, as the reference's Python does,
 * iou3d_nms_utils.py:83-98); a box suppresses every later box whose BEV IoU exceeds thresh (strict).
 * keep (N) int32 receives the kept positions (ascending), *num_keep_dev their count -- the greedy walk runs
 * on the device, nothing but these is read back.  workspace: mssvt_nms_workspace_bytes(N) bytes. N <= 16384.
 * ======================================================================== */
long long mssvt_nms_workspace_bytes(int num_boxes);
int mssvt_nms_bev(int num_boxes, const float *boxes_sorted, float thresh, void *workspace, int *keep,
                  int *num_keep_dev, void *stream);
/* as mssvt_nms_bev with the axis-aligned IoU of iou_normal (heading ignored; ref nms_normal_gpu, iou3d_nms.cpp:138-188 +
 * iou3d_nms_kernel.cu:314-372); same workspace size, same N <= 16384 */
int mssvt_nms_normal(int num_boxes, const float *boxes_sorted, float thresh, void *workspace, int *keep,
                     int *num_keep_dev, void *stream);

/* Pairwise box measures (ref: boxes_overlap_bev_gpu / boxes_iou_bev_gpu, iou3d_nms_kernel.cu:236-265; boxes_iou3d_gpu,
 * iou3d_nms_utils.py:48-81, fused into the launch; iou_normal :314-325).  out[i * num_b + j] =
 *   OVERLAP_BEV  area of the intersection of the two rotated rectangles (the procedure of the NMS above)
 *   IOU_BEV      ov / max(sa + sb - ov, 1e-8)
 *   IOU_3D       ov3 / max(va + vb - ov3, 1e-6), ov3 = ov * max(min(za + dza/2, zb + dzb/2) - max(za - dza/2, zb - dzb/2), 0)
 *   IOU_NORMAL   axis-aligned BEV IoU, heading ignored
 * boxes_*: rows of >= 7 floats [x,y,z,dx,dy,dz,heading,...], stride_* floats apart (so a (N, 9) tensor with velocities
 * needs no copy); out (num_a, num_b) f32, row-major, fully written (no need to clear it).  num_a == 0 or num_b == 0:
 * success, nothing launched. */
#define MSSVT_BOX_OVERLAP_BEV 0
#define MSSVT_BOX_IOU_BEV     1
#define MSSVT_BOX_IOU_3D      2
#define MSSVT_BOX_IOU_NORMAL  3
int mssvt_boxes_pairwise(int mode, int num_a, const float *boxes_a, int stride_a, int num_b, const float *boxes_b,
                         int stride_b, float *out, void *stream);

/* CenterHead's training targets of ONE head for the whole batch in one launch (ref: assign_target_of_single_head and the
 * host loop around it, pcdet/models/dense_heads/center_head.py:103-158, :160-214; gaussian_radius /
 * draw_gaussian_to_heatmap, pcdet/models/model_utils/centernet_utils.py:9-69).
 * gt_boxes (B, num_boxes, code_size >= 8) f32 rows [x,y,z,dx,dy,dz,heading,...,label]; class_of_label (num_labels) int32:
 * the class inside this head of label 0..num_labels-1, or -1 (label 0 = padding).  A row whose truncated label has a class
 * takes the next slot of its sample, in row order; slots >= num_max_objs are dropped.  Per slot with finite values and
 * positive dx, dy: the cell of the centre on the (H, W) map (x_min / y_min, voxel size and stride as the reference divides
 * them, clamped into the map), CornerNet's radius (k1..k5: the constants 1 - ov, 1 + ov, 16 (1 - ov), -2 ov, 16 ov (ov - 1)
 * of gaussian_radius, folded in double by the caller and rounded to float once, as torch folds them; truncated, at least
 * min_radius), a (2 r + 1)^2 Gaussian with sigma = (2 r + 1) / 6 max-merged into heatmaps[b][class], and
 *   target_boxes[b][slot] = [cx - ix, cy - iy, z, log dx, log dy, log dz, cos h, sin h, row[7 .. code_size-2]],
 *   inds = iy * W + ix, masks = 1.  Any other slot (unused, zero extent, non-finite row): zero row, inds 0, masks 0.
 * heatmaps (B, num_classes, H, W) f32, target_boxes (B, num_max_objs, code_size) f32, inds / masks (B, num_max_objs) i64:
 * every element is written, once (no need to clear them); no host synchronisation, nothing read back.  num_boxes == 0 is
 * legal (all zero).  B, num_classes <= 65535, H, W <= 2^20; radii are cut at 2^20 cells.                              */
int mssvt_center_targets(int batch_size, int num_boxes, int code_size, const float *gt_boxes, const int *class_of_label,
                         int num_labels, int num_classes, int H, int W, int num_max_objs, float x_min, float y_min,
                         float voxel_x, float voxel_y, float stride, float k1, float k2, float k3, float k4, float k5,
                         int min_radius, float *heatmaps, float *target_boxes, long long *inds, long long *masks,
                         void *stream);

/* CenterHead's inference decode of ONE head for the whole batch (ref: decode_bbox_from_heatmap / _topk,
 * pcdet/models/model_utils/centernet_utils.py:136-216), a fixed number of launches (8) whatever B is; no host
 * synchronisation, nothing read back.  All maps f32 contiguous NCHW: hm (B, C, H, W) RAW logits, center (B, 2, H, W),
 * center_z (B, 1, H, W), dim (B, 3, H, W) raw log sizes, rot (B, 2, H, W) [cos, sin], vel (B, num_vel, H, W) or NULL with
 * num_vel = 0.
 * Selection: per sample the N = C H W cells are ranked by (logit descending, flat index c H W + y W + x ascending) and the
 * first K' = min(K, N) are taken -- exact for any input, run-to-run deterministic.  The order refines topk(sigmoid(hm))
 * wherever that is defined (sigmoid is monotone, equal scores are unordered there).  -0.0 and +0.0 compare equal (the
 * index decides); a NaN logit ranks below everything and never yields a box.
 * Decode of a selected cell (c, y, x) with logit l, in rank order, one rounded f32 operation per step:
 *   score = 1 / (1 + exp(-l));  bx = ((x + center[0]) * stride) * voxel_x + x_min;  by likewise with y, center[1], voxel_y,
 *   y_min;  z = center_z;  sizes = exp(dim[0..2]);  heading = atan2(rot[1], rot[0]);  vel[0..num_vel) copied.
 * Filter: kept iff limit_*_min <= (bx, by, z) <= limit_*_max (inclusive, a NaN fails) and, with has_score_thresh != 0,
 * score > score_thresh (strict).  Survivors are compacted in rank order into cand_boxes (B, K, 7 + num_vel) f32,
 * cand_scores (B, K) f32, cand_labels (B, K) i32 (the class inside the head), cand_num (B) i32; EVERY element is written,
 * the tails are zero.  workspace: mssvt_center_decode_workspace_bytes(...) bytes (0: shape refused), the caller's, cleared
 * by the call on `stream` -- no static device state, concurrent calls on different streams need different workspaces.
 * Limits: B <= 65535, C <= 255, C H W < 2^24, K <= MSSVT_CENTER_DECODE_MAX_K, num_vel <= 64; MSSVT_E_TOOLARGE beyond. */
#define MSSVT_CENTER_DECODE_MAX_K 4096
long long mssvt_center_decode_workspace_bytes(int batch_size, int num_classes, int H, int W, int K);
int mssvt_center_decode(int batch_size, int num_classes, int H, int W, int num_vel, const float *hm, const float *center,
                        const float *center_z, const float *dim, const float *rot, const float *vel, int K, float stride,
                        float voxel_x, float voxel_y, float x_min, float y_min, float limit_x_min, float limit_y_min,
                        float limit_z_min, float limit_x_max, float limit_y_max, float limit_z_max, int has_score_thresh,
                        float score_thresh, void *workspace, float *cand_boxes, float *cand_scores, int *cand_labels,
                        int *cand_num, void *stream);

/* CenterHead's training loss of ONE head for the whole batch, forward and backward (ref: CenterHead.get_loss,
 * pcdet/models/dense_heads/center_head.py:220-250, with FocalLossCenterNet / RegLossCenterNet,
 * pcdet/utils/loss_utils.py:264-386); no host synchronisation, nothing read back, no float atomics: every sum has a fixed
 * order, so results are bit-identical run to run and across streams.
 * hm (B, C, H, W) f32 RAW logits, heatmap (B, C, H, W) f32 targets; the regression maps in HEAD_ORDER as up to six separate
 * contiguous (B, ch_k, H, W) f32 tensors (NULL / 0 for unused ones; they are never concatenated): code_size D = sum ch_k,
 * code dimension d indexes their channels in order; target_boxes (B, M, target_stride >= D) f32, columns 0..D-1 used;
 * inds, masks (B, M) i64 (masks 0 / 1); code_weights (D) f32 on the device.
 *   p = clamp(sigmoid(x), (float)1e-4, (float)(1 - 1e-4));   pos = sum_{gt == 1} log(p) (1 - p)^2;
 *   neg = sum_{gt < 1} log(1 - p) p^2 (1 - gt)^4;   num_pos = #{gt == 1};
 *   hm_loss = -(pos + neg) / num_pos if num_pos > 0 else -neg  (decided on the device);   num = #{masks != 0};
 *   per_dim[d] = sum_{b,j unmasked} |map_d[b, :, inds[b,j]] - target_boxes[b,j,d]| / max(num, 1);
 *   loc_loss = loc_weight * sum_d code_weights[d] per_dim[d].
 * A masked-out slot is not read (its index and target row may hold anything); an unmasked slot whose index lies outside
 * [0, H W) counts in num and contributes neither loss nor gradient.  Sums are double from the first add, rounded once.
 * forward: two launches.  workspace: mssvt_center_loss_workspace_bytes(...) bytes (0: shape refused), 8-byte aligned, no
 * need to clear it.  out (4 + D floats, kept for the backward): [0] hm_loss, [1] loc_loss, [2] num_pos and [3] num as int32
 * bit patterns, [4 + d] per_dim[d].
 * backward: at most three launches.  g_hm / g_loc: the upstream gradients of hm_loss / loc_loss as DEVICE scalars (NULL:
 * zero).  d_hm (B, C, H, W) or NULL: every element written once (through the clamp as torch does: zero where the sigmoid
 * lies outside the bounds); recomputed from hm and heatmap, the forward saves no gradient buffer.  d_map_k (B, ch_k, H, W)
 * or NULL (no gradient wanted): zero-filled by the call, then the cell of slot (b, j) gets g_loc loc_weight
 * code_weights[d] sign(pred - target) / max(num, 1) (sign(0) = 0), slots that share a cell summed in ascending j.
 * The heat-map passes run a grid that depends on n = B C H W alone: min(ceil(n / MSSVT_CENTER_LOSS_SWEEP),
 * MSSVT_CENTER_LOSS_MAX_BLOCKS) workgroups.  Limits: M <= MSSVT_CENTER_LOSS_MAX_OBJS, D <= MSSVT_CENTER_LOSS_MAX_CODE,
 * n < 2^31, B M < 2^31; MSSVT_E_TOOLARGE beyond.  Null pointers and non-positive sizes: MSSVT_E_BADARG before any HIP call. */
#define MSSVT_CENTER_LOSS_SWEEP 1024
#define MSSVT_CENTER_LOSS_MAX_BLOCKS 2048
#define MSSVT_CENTER_LOSS_MAX_OBJS 4096
#define MSSVT_CENTER_LOSS_MAX_CODE 16
long long mssvt_center_loss_workspace_bytes(int batch_size, int num_classes, int H, int W, int num_max_objs, int code_size);
int mssvt_center_loss_forward(int batch_size, int num_classes, int H, int W, int num_max_objs, int code_size,
                              int target_stride, const float *hm, const float *heatmap, const float *map0, int ch0,
                              const float *map1, int ch1, const float *map2, int ch2, const float *map3, int ch3,
                              const float *map4, int ch4, const float *map5, int ch5, const float *target_boxes,
                              const long long *inds, const long long *masks, const float *code_weights, float loc_weight,
                              void *workspace, float *out, void *stream);
int mssvt_center_loss_backward(int batch_size, int num_classes, int H, int W, int num_max_objs, int code_size,
                               int target_stride, const float *hm, const float *heatmap, const float *map0, int ch0,
                               const float *map1, int ch1, const float *map2, int ch2, const float *map3, int ch3,
                               const float *map4, int ch4, const float *map5, int ch5, const float *target_boxes,
                               const long long *inds, const long long *masks, const float *code_weights, float loc_weight,
                               const float *out, const float *g_hm, const float *g_loc, float *d_hm, float *d_map0,
                               float *d_map1, float *d_map2, float *d_map3, float *d_map4, float *d_map5, void *stream);

/* The NMS of mssvt_nms_bev / mssvt_nms_normal (`normal` != 0) for a batch of padded candidate lists whose lengths live on
 * the device (the outputs of mssvt_center_decode): two launches whose sizes depend on K and pre_max only, nothing read back.
 * Per sample b: n = min(cand_num[b], pre_max) rows of cand_boxes[b] (K rows of row_floats >= 7 floats, descending score);
 * a box suppresses every LATER box with IoU > thresh (strict; the pair geometry of the unbatched entries).  With
 * base = out_num[b] ON ENTRY, the first min(kept, post_max, out_rows - base) kept rows j go to out_boxes[b][base + j]
 * (out_rows rows of row_floats floats per sample), out_scores[b][base + j] and out_labels[b][base + j] =
 * class_map[cand_label] + 1 (i64; class_map (num_classes) i64; a label outside it gives 0), and out_num[b] grows by their
 * number: calls for successive heads on one stream append head-major.  Rows at or beyond out_num[b] are not touched (the
 * caller zeroes the buffers once).  workspace: mssvt_nms_bev_batched_workspace_bytes(B, K, pre_max) bytes, no need to
 * clear it.  B <= 65535, K <= 4096; MSSVT_E_TOOLARGE beyond. */
long long mssvt_nms_bev_batched_workspace_bytes(int batch_size, int K, int pre_max);
int mssvt_nms_bev_batched(int batch_size, int K, int row_floats, const float *cand_boxes, const float *cand_scores,
                          const int *cand_labels, const int *cand_num, const long long *class_map, int num_classes,
                          int pre_max, int post_max, float thresh, int normal, void *workspace, int out_rows,
                          float *out_boxes, float *out_scores, long long *out_labels, int *out_num, void *stream);

/* Weight / bias gradient of an nn.Linear over compact rows (training path; what autograd's library GEMM computes for
 * the reference's to_qs / to_kvs / projs / linear1 / linear2, ref mssvt_utils.py:80-83, mssvt_backbone.py:25-27):
 *   dW (Cout,Cin) = dY^T X,  db (Cout) = column sums of dY (db may be NULL);  X (M,Cin), dY (M,Cout) f32 row-major.
 * Deterministic split over the M rows on the fp32 matrix cores: per-slice partial slabs in `workspace`
 * (mssvt_linear_wgrad_workspace_floats(M,Cin,Cout) floats), added in slice order.  Cin, Cout multiples of 4,
 * ceil(Cout/16) * (ceil(Cin/16) + 1) <= 160 (256 x 128, 128 x 256 ...); MSSVT_E_TOOLARGE otherwise.           */
long long mssvt_linear_wgrad_workspace_floats(int M, int Cin, int Cout);
int mssvt_linear_wgrad(int M, int Cin, int Cout, const float *X, const float *dY, float *dW, float *db,
                       float *workspace, void *stream);

/* Y = X B^T + bias over compact rows on the fp32 matrix cores (training path), for the SMALL weight matrices of a Block
 * (64 x 64 to_qs / projs of a head group: ref mssvt_utils.py:80-83, mssvt_backbone.py:25-27) and, with transpose_w, their
 * input gradient dX = dY W -- library GEMMs under autograd in the reference, which pick poor tiles on these shapes.
 *   Y[m][n] = out_scale * act(bias[n] + sum_k X[m][k] B[n][k]),  B = W (N,K) row-major, or B[n][k] = W[k][n] with W (K,N)
 * (transpose_w != 0); out_scale = 1 or the attention scale of a query projection (ref mssvt_utils.py:131-133);
 * X (M,K) f32 with row stride ldx (floats, % 4 == 0), Y (M,N) with row stride ldy, bias (N) or NULL, relu != 0 clamps Y
 * at 0.  K, N in {64,128} (mssvt_linear_rows_supported); MSSVT_E_TOOLARGE otherwise.                                  */
int mssvt_linear_rows_supported(int K, int N);
int mssvt_linear_rows(int M, int K, int N, const float *X, int ldx, const float *W, int transpose_w, const float *bias,
                      int relu, float out_scale, float *Y, int ldy, void *stream);

/* Window attention on compact rows, forward and backward (training path; the softmax(QK^T)V of ref
 * mssvt_utils.py:131-149 for one head group, without the padded (windows, slots) layout and the -100 mask):
 * window w owns query rows [q_off[w], +q_cnt[w]) of q (R,cg) (already scaled) and key rows [k_off[w], +k_cnt[w]) of
 * kv (Kn,2cg) = [K|V]; ranges of different windows are disjoint.  fwd: O (R,cg), lse (R,heads) = log-sum-exp of the
 * scores.  bwd: dq (R,cg), dkv (Kn,2cg) from dO; every row is written by exactly one wave in a fixed order (no
 * atomics, bit-identical run to run).  cg = heads * hd <= 128, hd in {4,8,16,32,64}; windows without keys give O = 0. */
int mssvt_pair_attention_fwd(int nw, int cg, int heads, int hd, const int *q_off, const int *q_cnt, const int *k_off,
                             const int *k_cnt, const float *q, const float *kv, float *O, float *lse, void *stream);
int mssvt_pair_attention_bwd(int nw, int cg, int heads, int hd, const int *q_off, const int *q_cnt, const int *k_off,
                             const int *k_cnt, const float *q, const float *kv, const float *O, const float *lse,
                             const float *dO, float *dq, float *dkv, void *stream);

/* Inverted index of a (weighted) row gather dst[d] = sum_{e in [off[d],off[d+1])} w[e] src[idx[e]] (off NULL: one entry
 * per row), built on the device: grad_src[s] = sum_{p in [t_off[s],t_off[s+1])} t_w[p] grad_dst[t_idx[p]] with the
 * entries of a source row in ascending e -- the fixed summation order that replaces the reference's atomicAdd backward
 * (ref group_features_gpu.cu:15-47, sampling_gpu.cu:53-90).  Entries of drop_src (or out of [0,n_src)) are left out.
 * *max_count = the longest list if one is longer than long_list, else 0.  t_off (n_src+1), t_idx / t_w (nnz; t_w NULL
 * iff w NULL); workspace of mssvt_csr_transpose_workspace_bytes(nnz, n_src) bytes.                                    */
long long mssvt_csr_transpose_workspace_bytes(int nnz, int n_src);
int mssvt_csr_transpose(int nnz, int n_dst, int n_src, const int *off, const int *idx, const float *w, int drop_src,
                        int long_list, int *t_off, int *t_idx, float *t_w, int *max_count, void *workspace, void *stream);

/* ======================================================================== *
 * Part 5 -- a whole backbone forward behind ONE call (round 4).
 *
 * ref: MixedScaleSparseTransformer.forward, pcdet/models/backbones_3d/mssvt_backbone.py:450-472, which drives its blocks
 * from Python (>= 5B + L(5B+2) host syncs, ~100 launches per Block).  A frame object describes one resolution level
 * of the network -- L two-scale Blocks that share one window configuration, closed by a CompressBlock over pillar
 * windows [1,1,z] -- and mssvt_frame_forward enqueues the entry points of part 2 for it in the order the Python
 * module path (mssvt_amd/fused.py) issues them, out of ONE caller-owned workspace: same kernels, same arguments,
 * bit-identical results, no allocation and no host synchronisation inside the call.  The object holds parameter
 * POINTERS (device memory owned by the caller: rebuild it when a parameter moves), one pinned 4-KiB host buffer and
 * one event for the frame's single device-to-host hand-over.  add_* return MSSVT_E_TOOLARGE for shapes this path
 * does not cover; the caller keeps its own path for those.
 * Input: a voxel list sorted by (b,x,y,z) (what DynamicVFE emits); any other order is reported in the status
 * word (MSSVT_ST_UNSORTED) and the outputs are then empty.
 * ======================================================================== */
#define MSSVT_ST_UNSORTED 8 /* level status: the voxel list is not strictly ascending in (b,x,y,z) */

int mssvt_frame_create(void **frame_out);
int mssvt_frame_destroy(void *frame);
/* Level geometry (ref mssvt_backbone.py:436-448): grid [x,y,z] (z <= 64), voxel size, point cloud range
 * [x0,y0,z0,x1,y1,z1] (HOST arrays), channel width C of every block and FF of every feed-forward layer ((C,FF)
 * instantiated in csrc/ffn.hip).  Clears the block list.                                                        */
int mssvt_frame_set_level(void *frame, int batch_size, int x_max, int y_max, int z_max, int hash_size,
                          const float *host_voxel_size3, const float *host_range6, int C, int FF);
/* One MixedScaleSparseTransformerBlock (ref mssvt_backbone.py:11-347): window configuration (arguments of
 * mssvt_window_plan_two: win1 size, list capacities, the four offset tables on the device, their footprint and packed
 * form, key_num_sample, max_num_wins -- identical for every Block of the level), cbs_pattern (0 even / 1 odd / 2 win1
 * queries), use_feature_interpolation, norm1, the attention parameters (arguments of mssvt_block_attention; two head
 * groups), attn_mode 0 = mssvt_block_attention, 1 = mssvt_block_attention_kv16 (host_packed: its blobs or NULL),
 * 2 = mssvt_block_attention_bf16; norm2 + linear1 / linear2 and the fragments of mssvt_ffn_pack_weights.           */
int mssvt_frame_add_block(
    void *frame, const int *host_win1_size3, int max_num_odd, int max_num_even, int max_num_win1, int max_num_win2,
    int num_odd, int num_even, int num_win1, int num_win2, const int *vox_query_odd, const int *vox_query_even,
    const int *vox_query_win1, const int *vox_query_win2, const int *host_footprint4, const int *packed_offsets,
    int key_num_sample, int max_num_wins, int cbs_pattern, int use_interpolation, const float *norm1_w,
    const float *norm1_b, float norm1_eps, int num_groups, const int *host_c0, const int *host_cg, const int *host_heads,
    int head_dim, float scale, const float *const *host_Wq, const float *const *host_bq, const float *const *host_Wkv,
    const float *const *host_bkv, const float *const *host_Wo, const float *const *host_bo,
    const void *const *host_packed, const float *Wpos, const float *bpos, int attn_mode, const float *norm2_w,
    const float *norm2_b, float norm2_eps, const float *W1, const float *b1, const float *W2, const float *b2,
    const void *ffn_packed);
/* The MixedScaleSparseTransformerCompressBlock that ends the level (ref mssvt_backbone.py:349-398): pillar windows
 * [1,1,z] whose offset table stays inside the window (one lane per window in the plan kernel), one head group;
 * arguments of mssvt_window_plan_one / mssvt_compress_fused / mssvt_ffn_fused.  compress_ws_packed: the fragments of
 * mssvt_compress_ws_pack when the caller has checked mssvt_compress_ws's preconditions (the table lists every cell of
 * the slab, fp16 range) -- the attention is then that one launch -- or NULL.                                          */
int mssvt_frame_add_compress(
    void *frame, const int *host_win_size3, int max_num_win1, int num_win1, const int *vox_query_win1, int max_num_wins,
    const float *norm1_w, const float *norm1_b, float norm1_eps, const float *Wpos1, const float *bpos1, const float *Wpos2,
    const float *bpos2, const float *Wq, const float *bq, const float *Wkv, const float *bkv, const float *Wo, const float *bo,
    int head_dim, float scale, int split_f16, const float *norm2_w, const float *norm2_b, float norm2_eps, const float *W1,
    const float *b1, const float *W2, const float *b2, const void *ffn_packed, const void *compress_ws_packed);
/* on != 0: the first norm1 and the CompressBlock's pillar plan run on a stream of the frame object, under the Blocks'
 * plan kernel (two event edges per frame; results unchanged).                                                     */
int mssvt_frame_set_overlap(void *frame, int on);
/* Bytes of workspace a forward over num_voxels voxels needs (0: frame incomplete). */
long long mssvt_frame_workspace_bytes(void *frame, int num_voxels);
/* Enqueue the forward on `stream`.  features (N,C) f32, indices (N,4) int32 [b,z,y,x]; workspace: 256-byte aligned,
 * contents irrelevant (reusable by the next frame on the same stream).  Outputs, capacity-sized and caller-owned:
 * out_features (N,C) / out_indices (N,4): the first `rows` rows are the output voxel set (window order);
 * out_table (B,H,2): its hash table (filled here, -1 prefill included); out_counts (B) rows per sample.
 * `rows` and the status words travel to the host through the frame's pinned buffer: mssvt_frame_wait_words blocks
 * until they have landed (long before the frame's kernels end) and copies words [0, num_words) out:
 * [0] level status (MSSVT_ST_UNSORTED), [64] status / [65] window count of the Blocks' partition,
 * [128] status / [129] window count of the CompressBlock's partition = rows.                                     */
int mssvt_frame_forward(void *frame, int num_voxels, const float *features, const int *indices, void *workspace,
                        long long workspace_bytes, float *out_features, int *out_indices, int *out_table,
                        int *out_counts, void *stream);
int mssvt_frame_wait_words(void *frame, int *host_out, int num_words);

/* Y = out_scale * act(X B^T + bias) over compact rows with split-fp16 matrix operands (csrc/linear_rows_h.hip; the
 * training path's nn.Linear forward and, with transpose_w, its input gradient dX = dY W -- ref mssvt_backbone.py:339-343,
 * mssvt_utils.py:80-83 through autograd): B = W (N, K) row-major, or B[n][k] = W[k][n] with transpose_w (W then (K, N)).
 * (K, N) in {(128,256), (256,128), (64,128), (128,64), (128,128), (64,64)}; ldx >= K, ldy >= N, multiples of 4.  Rows of X
 * and the weight matrix are normalised by powers of two inside the kernel: no range precondition.                    */
int mssvt_linear_rows_h_supported(int K, int N);
int mssvt_linear_rows_h(int M, int K, int N, const float *X, int ldx, const float *W, int transpose_w, const float *bias,
                        int relu, float out_scale, float *Y, int ldy, void *stream);

/* y = act(scale[c] * conv(x, w) + shift[c]) on channels-last fp32 tensors with split-fp16 matrix operands
 * (csrc/bev_conv.hip; the kernel is csrc/split_conv.hip.h's, shared with mssvt_head_conv_*): the Conv2d + BatchNorm2d +
 * ReLU triples of HeightCompression's compress_layers (ref
 * pcdet/models/backbones_2d/map_to_bev/height_compression.py:20-39, applied to the grid of :41-45) and of BaseBEVBackbone's
 * blocks / 1x1 deblocks (ref pcdet/models/backbones_2d/base_bev_backbone.py:30-78, forward :87-112) in eval mode.
 * Inference only.  Tap sets: 3x3 with stride 1 or 2, dilation 1 or 2 and zero padding = dilation (ZeroPad2d(1) + padding 0
 * at stride 2 is the padding-1 case); 1x1 with stride 1.  (cin, cout) in {(128,128), (128,256), (256,256), (32,32), (32,64),
 * (64,64)}.  Output size Ho = (H + 2 p - d (k - 1) - 1) / stride + 1.
 * mssvt_bev_conv_supported: 1 if the kernel covers the layer, else 0.
 * mssvt_bev_conv_pack_bytes: size of a layer's packed blob (0: not covered); 64 header bytes (float [0] = 2^-e, [1] = 2^e, e the
 *   exponent of max |w|), scale (cout) f32, shift (cout) f32, then per (128-wide slice of cout, tap, 128-wide chunk of cin) the
 *   hi and the lo fp16 image of the weights divided by 2^e as v_mfma_f32_16x16x32_f16 operand fragments
 *   [k step][column tile][lane][8] (tests/bev_conv_ref.py holds a host-side reader).
 * mssvt_bev_conv_pack: weight (cout, cin, k, k) as Conv2d holds it, or (cin, cout, 1, 1) with transposed != 0 (ConvTranspose2d,
 *   k = 1, stride 1); bias (cout) or NULL; BatchNorm2d in eval mode folded into scale / shift (bn_mean / bn_var (cout) or both
 *   NULL: no batch norm; bn_weight / bn_bias (cout) or NULL: no affine); scale / shift stay fp32, they are not rounded into the
 *   fp16 weights.  Two launches, no host read.  packed: 16-byte aligned, mssvt_bev_conv_pack_bytes bytes.
 * mssvt_bev_conv: x (B, H, W, cin) f32, y (B, Ho, Wo, cout) f32, both 16-byte aligned; exp_workspace (B*H*W) int32, written
 *   here (the largest |x| of every input pixel: each output pixel's operands are normalised by one exact power of two over
 *   its receptive field, the weights by one for the tensor: no range precondition, and scaling x by a power of two scales
 *   y bit for bit).  Never reads outside x, writes every element of y exactly once, bit-identical from call to call.
 * Null / unaligned pointers and non-positive sizes: MSSVT_E_BADARG; a layer mssvt_bev_conv_supported refuses, or
 * B*H*W >= 2^31 - 1024: MSSVT_E_TOOLARGE; neither launches anything.                                                  */
#define MSSVT_BEV_CONV_WAVE_PIXELS 32   /* output pixels of one wavefront */
#define MSSVT_BEV_CONV_BLOCK_PIXELS 256 /* output pixels of one workgroup */
int mssvt_bev_conv_supported(int ksize, int cin, int cout, int stride, int dilation);
long long mssvt_bev_conv_pack_bytes(int ksize, int cin, int cout);
int mssvt_bev_conv_pack(const float *weight, int transposed, const float *bias, const float *bn_weight, const float *bn_bias,
                        const float *bn_mean, const float *bn_var, float bn_eps, int ksize, int cin, int cout, void *packed,
                        void *stream);
int mssvt_bev_conv(const float *x, int B, int H, int W, int cin, const void *packed, int ksize, int cout, int stride,
                   int dilation, int relu, int *exp_workspace, float *y, void *stream);

/* The same layers writing a channel slice of a wider tensor, and the 2x2 stride-2 transposed deblock (csrc/bev_conv.hip; ref
 * pcdet/models/backbones_2d/base_bev_backbone.py:52-63 deblocks, :104-108 the concatenation they replace).  Inference only.
 * mssvt_bev_conv_into: mssvt_bev_conv with y (B, Ho, Wo, ystride) f32 of which the layer writes channels [ybase, ybase + cout)
 *   and touches no other; same arithmetic and bits as mssvt_bev_conv.
 * mssvt_bev_up2_*: ConvTranspose2d(cin, cout, 2, stride 2, no padding) + BatchNorm2d (eval) + ReLU,
 *   y[b, 2 iy + dy, 2 ix + dx, n] = act(scale[n] * sum_c x[b, iy, ix, c] w[c, n, dy, dx] + shift[n]); (cin, cout) in {(256, 256),
 *   (64, 32)}.  One launch over the B*H*W input pixels: the four output phases (dy, dx) are four 1x1 layers sharing every input
 *   row read, same split-fp16 arithmetic (three matrix instructions per product sum, fp32 scale / shift in the epilogue, one
 *   exact power of two per input pixel and one for the whole weight tensor).
 * mssvt_bev_up2_pack_bytes: size of the blob (0: not covered): the blob of mssvt_bev_conv_pack for a 1x1 layer of cin inputs and
 *   4 cout columns -- 64 header bytes, scale (4 cout), shift (4 cout), then per 128-wide (cout = 32: 32-wide) slice of the
 *   columns and 128-wide chunk of cin the hi and the lo fp16 image; column ph * cout + n holds w[c, n, dy, dx] with
 *   ph = dy * 2 + dx, scale / shift repeat per phase.
 * mssvt_bev_up2_pack: weight (cin, cout, 2, 2) as ConvTranspose2d holds it; bias / BatchNorm2d as in mssvt_bev_conv_pack
 *   (folded in double, rounded once, never into the fp16 weights).  Two launches, no host read.
 * mssvt_bev_up2: x (B, H, W, cin) f32, y (B, 2H, 2W, ystride) f32 of which channels [ybase, ybase + cout) are written, every
 *   element of that slice exactly once (no atomics, y is never read) and nothing outside it; exp_workspace (B*H*W) int32,
 *   written here.  Bit-identical from call to call; scaling x by a power of two scales y bit for bit.
 * Null / unaligned (16 bytes: x, y, packed) pointers, non-positive sizes, ystride % 4, ybase % 4, ybase < 0 or
 * ybase + cout > ystride: MSSVT_E_BADARG; an uncovered shape or B*Ho*Wo (the OUTPUT pixels) >= 2^31 - 1024: MSSVT_E_TOOLARGE;
 * neither launches anything.                                                                                          */
int mssvt_bev_conv_into(const float *x, int B, int H, int W, int cin, const void *packed, int ksize, int cout, int stride,
                        int dilation, int relu, int *exp_workspace, float *y, int ystride, int ybase, void *stream);
int mssvt_bev_up2_supported(int cin, int cout);
long long mssvt_bev_up2_pack_bytes(int cin, int cout);
int mssvt_bev_up2_pack(const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                       const float *bn_mean, const float *bn_var, float bn_eps, int cin, int cout, void *packed, void *stream);
int mssvt_bev_up2(const float *x, int B, int H, int W, int cin, const void *packed, int cout, int relu, int *exp_workspace,
                  float *y, int ystride, int ybase, void *stream);

/* The weight gradient of a 3x3, stride-1 convolution with dilation d in {1, 2} and zero padding d, on channels-last f32
 * tensors (csrc/bev_conv.hip, kernels in csrc/split_wgrad.hip.h): the training path of the layers above,
 *   dw[o, c, ky, kx] = sum over (b, y, x) of dy[b, y, x, o] * x[b, y + (ky - 1) d, x + (kx - 1) d, c]   (outside the image: 0),
 * (cin, cout) in {(128,128), (256,256), (32,32), (64,64)}.  A GEMM whose reduction runs over the B*H*W pixels in memory order,
 * in split-fp16 arithmetic (hi / lo rounded to nearest, three v_mfma_f32_16x16x32_f16 per product sum, fp32 accumulators in
 * registers).  The pixels are cut into slices of mssvt_bev_conv_wgrad_slice_pixels(cin, cout) (a function of the channel
 * shape alone: 4096 / 2048 / 256 / 256 for the shapes above; a slice may span two samples); per (slice, tap) the dy rows are
 * normalised by one exact power of two and the x rows the tap reads by another, both undone exactly on the partial, so
 * scaling x or dy by a power of two scales dw bit for bit.  Partials go to slabs of the workspace and a second launch adds
 * them in slice order: no atomics, bit-identical from call to call and across streams, whatever the workspace held.
 * mssvt_bev_conv_wgrad_supported: 1 if covered, else 0.
 * mssvt_bev_conv_wgrad_slice_pixels: the slice length (0: shape not covered).
 * mssvt_bev_conv_wgrad_workspace_bytes: 2 * roundup(4 B H W, 256) (one exponent word per pixel of x and of dy) +
 *   slices * 9 * cout * cin * 4 (0: not covered, non-positive sizes or too many pixels).
 * mssvt_bev_conv_wgrad: x (B, H, W, cin), dy (B, H, W, cout), dw (cout, cin, 3, 3) as Conv2d holds it, workspace of
 *   mssvt_bev_conv_wgrad_workspace_bytes bytes (written here, no need to clear); all 16-byte aligned.  Four launches, no host
 *   read, no host synchronisation.  Never reads outside x / dy, writes every element of dw exactly once.
 * Null / unaligned pointers and non-positive sizes: MSSVT_E_BADARG; an uncovered shape or B*H*W >= 2^31 - 1024:
 * MSSVT_E_TOOLARGE; neither launches anything.                                                                        */
int mssvt_bev_conv_wgrad_supported(int ksize, int cin, int cout, int stride, int dilation);
int mssvt_bev_conv_wgrad_slice_pixels(int cin, int cout);
long long mssvt_bev_conv_wgrad_workspace_bytes(int B, int H, int W, int ksize, int cin, int cout);
int mssvt_bev_conv_wgrad(const float *x, const float *dy, int B, int H, int W, int cin, int cout, int ksize, int dilation,
                         float *dw, void *workspace, void *stream);

/* The backward of a transposed deblock whose kernel equals its stride, ConvTranspose2d(cin, cout, s, stride = s) with s in
 * {1, 2}, no padding and no bias, on channels-last f32 tensors (csrc/bev_conv.hip, csrc/split_wgrad.hip.h; ref
 * pcdet/models/backbones_2d/base_bev_backbone.py:52-63).  H, W are the deblock's INPUT grid: x and dx are (B, H, W, cin), dy is
 * (B, s H, s W, cout), weight and dw are (cin, cout, s, s) as ConvTranspose2d holds them.  (stride, cin, cout) in
 * {(1,128,256), (2,256,256), (1,32,64), (2,64,32)}.
 * mssvt_bev_deblock_wgrad:  dw[c, n, dy, dx] = sum over (b, iy, ix) of x[b, iy, ix, c] * dy[b, s iy + dy, s ix + dx, n]:
 *   mssvt_bev_conv_wgrad's kernel and arithmetic with the phases (dy, dx) as taps, on 128 x 128 (narrow: 32 x 32) tiles of
 *   (cin, cout).  The B*H*W input pixels are cut into slices of mssvt_bev_deblock_wgrad_slice_pixels (1024 / 2048 / 256 / 256
 *   for the shapes above; a slice may span two samples); per slice the x rows are normalised by one exact power of two and per
 *   (slice, phase) the dy rows that phase reads by another, both undone exactly on the partial, so scaling x or dy by a power
 *   of two scales dw bit for bit.  Partials go to slabs of the workspace and a second launch adds them in slice order: no
 *   atomics, bit-identical from call to call and across streams, whatever the workspace held.  Four launches, no host read.
 *   Never reads outside x / dy, writes every element of dw exactly once.
 * mssvt_bev_deblock_wgrad_workspace_bytes: roundup(4 B H W, 256) + roundup(4 s s B H W, 256) (one exponent word per pixel of x
 *   and of dy) + slices * s * s * cin * cout * 4 (0: not covered, non-positive sizes or too many pixels).
 * mssvt_bev_deblock_dgrad:  dx[b, iy, ix, c] = sum over (n, dy, dx) of dy[b, s iy + dy, s ix + dx, n] * weight[c, n, dy, dx]:
 *   mssvt_bev_conv's kernel over dy with `weight` packed as the Conv2d weight (out = cin, in = cout, ky, kx) it already is --
 *   s x s taps at stride s, no padding, scale 1, shift 0, no activation; same arithmetic (one exact power of two per dx pixel
 *   over the dy pixels it reads and one for the weight tensor: scaling dy by a power of two scales dx bit for bit).  The
 *   packed weights and the exponent words of dy live in the workspace: four launches, no host read.  Never reads outside
 *   dy / weight, writes every element of dx exactly once, bit-identical from call to call whatever the workspace held.
 * mssvt_bev_deblock_dgrad_workspace_bytes: roundup(4 s s B H W, 256) + 64 + 8 cin + 4 s s cin cout (0 as above).
 * All pointers 16-byte aligned; workspaces are written here, no need to clear.  Null / unaligned pointers and non-positive
 * sizes: MSSVT_E_BADARG; an uncovered shape or s*s*B*H*W >= 2^31 - 1024: MSSVT_E_TOOLARGE; neither launches anything.    */
int mssvt_bev_deblock_train_supported(int stride, int cin, int cout);
int mssvt_bev_deblock_wgrad_slice_pixels(int stride, int cin, int cout);
long long mssvt_bev_deblock_wgrad_workspace_bytes(int B, int H, int W, int stride, int cin, int cout);
int mssvt_bev_deblock_wgrad(const float *x, const float *dy, int B, int H, int W, int cin, int cout, int stride, float *dw,
                            void *workspace, void *stream);
long long mssvt_bev_deblock_dgrad_workspace_bytes(int B, int H, int W, int stride, int cin, int cout);
int mssvt_bev_deblock_dgrad(const float *dy, const float *weight, int B, int H, int W, int cin, int cout, int stride, float *dx,
                            void *workspace, void *stream);

/* The backward of the 3x3 stride-2 convolution, Conv2d(cin, cout, 3, stride = 2, padding = 1, bias = False) (a ZeroPad2d(1) in
 * front of padding 0 is the same layer), on channels-last f32 tensors (csrc/bev_conv.hip, csrc/split_wgrad.hip.h,
 * csrc/split_conv.hip.h; ref pcdet/models/backbones_2d/base_bev_backbone.py:30-38).  H, W are the layer's INPUT grid: x and dx
 * are (B, H, W, cin), dy is (B, Ho, Wo, cout) with Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, weight and dw are
 * (cout, cin, 3, 3) as Conv2d holds them.  (cin, cout) in {(128,256), (32,64)}.  The forward is mssvt_bev_conv at stride 2.
 * mssvt_bev_down_wgrad:  dw[o, c, ky, kx] = sum over (b, oy, ox) of dy[b, oy, ox, o] * x[b, 2 oy + ky - 1, 2 ox + kx - 1, c]
 *   (outside the image: 0): mssvt_bev_conv_wgrad's kernel and arithmetic with the stride-2 tap map, on 128 x 128 (narrow:
 *   32 x 32) tiles of (cout, cin).  The B*Ho*Wo OUTPUT pixels are cut into slices of mssvt_bev_down_wgrad_slice_pixels (2048 /
 *   256 for the shapes above; a slice may span two samples); per slice the dy rows are normalised by one exact power of two and
 *   per (slice, tap) the x rows that tap reads by another, both undone exactly on the partial, so scaling x or dy by a power of
 *   two scales dw bit for bit.  Partials go to slabs of the workspace and a second launch adds them in slice order: no
 *   atomics, bit-identical from call to call and across streams, whatever the workspace held.  Four launches, no host read.
 *   Never reads outside x / dy, writes every element of dw exactly once.
 * mssvt_bev_down_wgrad_workspace_bytes: roundup(4 B H W, 256) + roundup(4 B Ho Wo, 256) (one exponent word per pixel of x and
 *   of dy) + slices * 9 * cout * cin * 4 (0: not covered, non-positive sizes or too many pixels).
 * mssvt_bev_down_dgrad:  dx[b, iy, ix, c] = sum over o and the taps (ky, kx) with 2 oy + ky - 1 = iy, 2 ox + kx - 1 = ix of
 *   dy[b, oy, ox, o] * weight[o, c, ky, kx].  By the parity of (iy, ix) dx falls into four phases, each a dense convolution
 *   over dy at stride 1: even iy = 2 j takes ky = 1 at oy = j, odd iy = 2 j + 1 takes ky = 2 at oy = j and ky = 0 at oy = j + 1
 *   (absent when j + 1 = Ho), the same in x -- 1, 2, 2 and 4 taps, the 9 taps of the weight each used once.  One launch of
 *   mssvt_bev_conv's kernel over dy serves all four (the 4-tap phase first): no zero-stuffed dy, no product with a structural
 *   zero, no atomics, every element of dx written exactly once; one exact power of two per dx pixel over exactly the dy pixels
 *   its taps read and one for the weight tensor, so scaling dy or weight by a power of two scales dx bit for bit.  The packed
 *   weights (the tensor as stored, taps in phase order) and the exponent words of dy live in the workspace: four launches, no
 *   host read.  Never reads outside dy / weight, bit-identical from call to call whatever the workspace held.
 * mssvt_bev_down_dgrad_workspace_bytes: roundup(4 B Ho Wo, 256) + 64 + 8 cin + 36 cin cout (0 as above).
 * All pointers 16-byte aligned; workspaces are written here, no need to clear.  Null / unaligned pointers and non-positive
 * sizes: MSSVT_E_BADARG; an uncovered shape or B*H*W >= 2^31 - 1024: MSSVT_E_TOOLARGE; neither launches anything.        */
int mssvt_bev_down_train_supported(int cin, int cout);
int mssvt_bev_down_wgrad_slice_pixels(int cin, int cout);
long long mssvt_bev_down_wgrad_workspace_bytes(int B, int H, int W, int cin, int cout);
int mssvt_bev_down_wgrad(const float *x, const float *dy, int B, int H, int W, int cin, int cout, float *dw, void *workspace,
                         void *stream);
long long mssvt_bev_down_dgrad_workspace_bytes(int B, int H, int W, int cin, int cout);
int mssvt_bev_down_dgrad(const float *dy, const float *weight, int B, int H, int W, int cin, int cout, float *dx, void *workspace,
                         void *stream);

/* CenterHead's convolutions in eval mode as three launches (csrc/head_conv.hip; ref pcdet/models/dense_heads/center_head.py:
 * shared_conv :76-84, SeparateHead :11-46, forward :350-360), on the kernel of mssvt_bev_conv (csrc/split_conv.hip.h: split-fp16 operands, three
 * matrix instructions per product sum, fp32 scale / shift in the epilogue, exact power-of-two normalisation per output pixel
 * and per weight tensor).  All tensors channels-last f32, 3x3, stride 1, zero padding 1.  Inference only.
 *   shared: x (B, H, W, cin) -> (B, H, W, s) = relu(bn(conv)), cin in {64, 256, 384, 512}, s in {32, 64};
 *   trunk:  the first Conv + BN + ReLU of all nb branches (of all heads) as one convolution s -> nb s: (B, H, W, nb s);
 *   finals: the last convolution of every branch, s -> k_b <= 16 with bias and no activation; branch b reads channels
 *           [b s, (b + 1) s) of the trunk tensor and writes PLANAR: its maps are the contiguous (B, k_b, H, W) block at float
 *           offset kbase_b B H W of y, kbase_b = the maps of the branches before it (y holds B H W sum k_b floats).
 * Exponent words: one int32 per (pixel, branch) = the largest |value| over the channels a later stage normalises together,
 * as bits.  mssvt_head_conv_shared writes the input's into exp_workspace (B H W) itself and leaves its output's in exp_out
 * (B H W); mssvt_head_conv_trunk reads those and leaves exp_out (B H W, nb), one word per pixel AND BRANCH, which
 * mssvt_head_conv_finals reads: every branch is normalised on its own slice.  mssvt_head_conv_expmap computes the words of any
 * (rows, c) matrix, c in {32, 64, 256, 384, 512} (a tensor that another producer wrote: rows = B H W, or B H W nb with c = s).
 * mssvt_head_conv_supported: 1 if the three stages cover a head with these sizes (nb <= 64 branches, kmax = max k_b <= 16).
 * Packed blobs: 16 bytes per slice {float 2^-e, float 2^e, int k, int kbase} padded to 64, scale then shift (slices x NS) f32,
 * then per slice, tap and 128-channel chunk of the input the hi and the lo fp16 image as operand fragments (NS = s; 16 for
 * the finals, rows beyond k_b zero).  *_pack_bytes: the size (0: not covered).  mssvt_head_conv_shared_pack packs the whole
 * blob; mssvt_head_conv_trunk_pack / mssvt_head_conv_finals_pack pack ONE branch per call into the blob of nb branches
 * (weight (s, s, 3, 3) / (k, s, 3, 3) as Conv2d holds it; BatchNorm2d in eval mode folded as in mssvt_bev_conv_pack; two
 * launches each, no host read).  Never reads outside its inputs, writes every output element exactly once, bit-identical
 * from call to call.  Null / unaligned (16 bytes: x, y, packed) pointers, sizes < 1, branch outside [0, nb): MSSVT_E_BADARG;
 * sizes outside the sets above, k > 16, B H W >= 2^31 - 1024: MSSVT_E_TOOLARGE; neither launches anything.              */
int mssvt_head_conv_supported(int cin, int s, int nb, int kmax);
long long mssvt_head_conv_shared_pack_bytes(int cin, int s);
long long mssvt_head_conv_trunk_pack_bytes(int s, int nb);
long long mssvt_head_conv_finals_pack_bytes(int s, int nb);
int mssvt_head_conv_shared_pack(const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                                const float *bn_mean, const float *bn_var, float bn_eps, int cin, int s, void *packed,
                                void *stream);
int mssvt_head_conv_trunk_pack(const float *weight, const float *bias, const float *bn_weight, const float *bn_bias,
                               const float *bn_mean, const float *bn_var, float bn_eps, int s, int nb, int branch,
                               void *packed, void *stream);
int mssvt_head_conv_finals_pack(const float *weight, const float *bias, int s, int nb, int branch, int k, int kbase,
                                void *packed, void *stream);
int mssvt_head_conv_expmap(const float *x, long long rows, int c, int *exp_words, void *stream);
int mssvt_head_conv_shared(const float *x, int B, int H, int W, int cin, int s, const void *packed, int *exp_workspace,
                           float *y, int *exp_out, void *stream);
int mssvt_head_conv_trunk(const float *x, int B, int H, int W, int s, int nb, const void *packed, const int *exp_in,
                          float *y, int *exp_out, void *stream);
int mssvt_head_conv_finals(const float *x, int B, int H, int W, int s, int nb, const void *packed, const int *exp_in,
                           float *y, void *stream);

/* CenterHead's shared layer and trunk in TRAINING mode, forward and backward (csrc/head_conv.hip, csrc/split_conv.hip.h,
 * csrc/split_wgrad.hip.h; ref center_head.py :76-84, :11-46).  The layers are the plain convolutions y = conv3x3(x, W) + bias
 * (stride 1, zero padding 1); their BatchNorm2d + ReLU are not part of these calls.  All tensors channels-last f32.
 * cin in {64, 256, 384, 512}, s in {32, 64}, 1 <= nb <= 64 branches: mssvt_head_conv_train_supported.
 *   shared  mssvt_head_conv_shared_train: x (B, H, W, cin) -> y (B, H, W, s); packed = mssvt_head_conv_shared_pack's blob with
 *             the BatchNorm pointers NULL (scale 1, shift = bias); exp_workspace (B H W) int32 is written here.
 *           mssvt_head_conv_shared_dgrad: dx (B, H, W, cin) = the convolution s -> cin over dy with the taps of weight
 *             (s, cin, 3, 3) rotated by 180 degrees and the channel axes swapped; the tensor is packed inside the call
 *             (workspace: roundup(4 B H W, 256) + 64 + 8 cin + 36 cin s bytes).
 *           mssvt_head_conv_shared_wgrad: dw (s, cin, 3, 3), mssvt_bev_conv_wgrad's kernel and arithmetic on s x s tiles of
 *             (s, cin); the pixels are cut into slices of mssvt_head_conv_train_wgrad_slice_pixels(cin, s) (the trunk: (s, s); workspace: 2 roundup(4 B H W,
 *             256) + slices 9 cin s 4 bytes).
 *   trunk   mssvt_head_conv_trunk_train: y (B, H, W, s) -> t [nb][B H W][s], BRANCH-MAJOR: branch b's output is the dense
 *             (B, H, W, s) tensor at float b B H W s; packed = mssvt_head_conv_trunk_pack's blob, BatchNorm pointers NULL.
 *           mssvt_head_conv_trunk_dgrad: dy (B, H, W, s) = sum over b of rot(W_b) applied to dT_b, one launch, one accumulation
 *             chain per element; one power of two per output pixel over its receptive field and ALL branches, one for all
 *             weights (workspace: roundup(4 nb B H W, 256) + 64 + 8 s + 36 s s nb bytes).
 *           mssvt_head_conv_trunk_wgrad: dw [nb][s][s][3][3]; per slice, every branch's dT_b rows are normalised by that
 *             branch's own power of two (workspace: roundup(4 B H W, 256) + roundup(4 nb B H W, 256) + slices 9 nb s s 4).
 *   bias    mssvt_head_conv_bgrad: db [nb][s] = the sums over pixels of dT_b (the shared layer: nb = 1), in pieces of
 *             mssvt_head_conv_train_bias_piece_rows rows: each of the 1024 / s threads of a column adds its rows (every
 *             1024 / s-th) in row order, those threads are added in order, the pieces in piece order (workspace: pieces nb s 4).
 * host_dts / host_dys / host_weights: HOST arrays of nb device pointers (the tensors autograd hands back, dT_b (B, H, W, s),
 * and the weights W_b (s, s, 3, 3)), read during the call and handed to the kernels by value.
 * No float atomics, one writer per output element, bit-identical from call to call whatever the workspaces held, no host read;
 * scaling an operand by a power of two scales the result bit for bit.  *_workspace_bytes: 0 where the call would refuse.
 * Null / unaligned (16 bytes) pointers and sizes < 1: MSSVT_E_BADARG; sizes outside the sets above, nb > 64,
 * B H W >= 2^31 - 1024: MSSVT_E_TOOLARGE; neither launches anything.                                                      */
int mssvt_head_conv_train_supported(int cin, int s, int nb);
int mssvt_head_conv_train_wgrad_slice_pixels(int cin, int s);
int mssvt_head_conv_train_bias_piece_rows(int s);
int mssvt_head_conv_shared_train(const float *x, int B, int H, int W, int cin, int s, const void *packed, int *exp_workspace,
                                 float *y, void *stream);
long long mssvt_head_conv_shared_dgrad_workspace_bytes(int B, int H, int W, int cin, int s);
int mssvt_head_conv_shared_dgrad(const float *dy, const float *weight, int B, int H, int W, int cin, int s, float *dx,
                                 void *workspace, void *stream);
long long mssvt_head_conv_shared_wgrad_workspace_bytes(int B, int H, int W, int cin, int s);
int mssvt_head_conv_shared_wgrad(const float *x, const float *dy, int B, int H, int W, int cin, int s, float *dw,
                                 void *workspace, void *stream);
long long mssvt_head_conv_bgrad_workspace_bytes(int B, int H, int W, int s, int nb);
int mssvt_head_conv_bgrad(const float *const *host_dys, int B, int H, int W, int s, int nb, float *db, void *workspace,
                          void *stream);
int mssvt_head_conv_trunk_train(const float *y, int B, int H, int W, int s, int nb, const void *packed, int *exp_workspace,
                                float *t, void *stream);
long long mssvt_head_conv_trunk_dgrad_workspace_bytes(int B, int H, int W, int s, int nb);
int mssvt_head_conv_trunk_dgrad(const float *const *host_dts, const float *const *host_weights, int B, int H, int W, int s,
                                int nb, float *dy, void *workspace, void *stream);
long long mssvt_head_conv_trunk_wgrad_workspace_bytes(int B, int H, int W, int s, int nb);
int mssvt_head_conv_trunk_wgrad(const float *y, const float *const *host_dts, int B, int H, int W, int s, int nb, float *dw,
                                void *workspace, void *stream);

/* DynamicVFE's two PFN layers in eval mode as two launches (csrc/pfn_fused.hip; ref
 * pcdet/models/backbones_3d/vfe/dynamic_vfe.py:96-131, PFNLayerV2 :14-52), default configuration: 5 point features + cluster
 * offset + voxel-centre offset (11 inputs), NUM_FILTERS [64, 128].  points (P, stride >= 6) f32 rows [b, x, y, z, f4, f5];
 * point_voxel (P) int32, -1 outside the grid; mean3 (N, 3) = mssvt_voxel_mean_xyz; voxel_coords (N, 4) int32 [b, z, y, x];
 * host_voxel_size3 / host_offset3: HOST float[3] (offset = voxel_size / 2 + range_min); layer parameters as the state dict holds
 * them (pfn.{0,1}.0.weight / .bias, pfn.{0,1}.1.weight / .bias / .running_mean / .running_var, eps); x1_scratch (P, 64),
 * m1_scratch (max(N,1), 64), x2_scratch (P, 128): caller-owned; out (N, 128) = the voxel features.                                       */
int mssvt_pfn_fused_64_128(const float *points, int point_stride, long long num_points, const int *point_voxel,
                           int num_voxels, const float *mean3, const int *voxel_coords, const float *host_voxel_size3,
                           const float *host_offset3, const float *W1, const float *b1, const float *bn1_w,
                           const float *bn1_b, const float *bn1_mean, const float *bn1_var, float bn1_eps, const float *W2,
                           const float *b2, const float *bn2_w, const float *bn2_b, const float *bn2_mean,
                           const float *bn2_var, float bn2_eps, float *x1_scratch, float *m1_scratch, float *x2_scratch,
                           float *out, void *stream);

/* Round 6: the same two layers AND the cluster-centre mean over points grouped by voxel (csrc/pfn_sorted.hip): a counting
 * sort on point_voxel, then every reduction is a loop over a voxel's run of rows -- no atomics on feature rows, no -inf
 * fills, the per-point layer-2 output never reaches memory.  Results bit-identical to mssvt_voxel_mean_xyz +
 * mssvt_pfn_fused_64_128.  workspace: mssvt_pfn_sorted_workspace_ints(P, N) int32; x1_scratch (P, 64), m1_scratch (N, 64):
 * caller-owned; out (N, 128).  Every voxel must hold at least one point (mssvt_voxelize's output does).                  */
long long mssvt_pfn_sorted_workspace_ints(long long num_points, int num_voxels);
int mssvt_pfn_sorted_64_128(const float *points, int point_stride, long long num_points, const int *point_voxel,
                            int num_voxels, const int *voxel_coords, const float *host_voxel_size3,
                            const float *host_offset3, const float *W1, const float *b1, const float *bn1_w,
                            const float *bn1_b, const float *bn1_mean, const float *bn1_var, float bn1_eps, const float *W2,
                            const float *b2, const float *bn2_w, const float *bn2_b, const float *bn2_mean,
                            const float *bn2_var, float bn2_eps, int *workspace, float *x1_scratch, float *m1_scratch,
                            float *out, void *stream);

/* DynamicVFE's TRAINING step over points grouped by voxel (csrc/vfe_train.hip): the index and reduction operators of
 * ref pcdet/models/backbones_3d/vfe/dynamic_vfe.py:71-131 -- the kept points and unq_inv of :83-93, scatter_mean of :98,
 * the features of :96-112, scatter_max + concat of PFNLayerV2 (:44-52) and the final scatter_max of :128-129 -- with
 * torch_scatter's scatter_mean / scatter_max as oracle/gen_golden_vfe.py restates them (the gradient of a maximum split
 * equally between the rows that attain it exactly).  No float atomics: every output element has one writer and every float
 * sum a fixed order, so values and gradients are bit-identical run to run and across streams.  All kernels gfx950, wave64.
 *
 * mssvt_vfe_group (ref :83-93): point_voxel (P) int32 of mssvt_voxelize (-1: outside the grid) -> order (P) int32, the
 *   original index of every kept point sorted by voxel and, inside a voxel, by ascending point index (entries behind P'
 *   hold the dropped points); row_voxel (P) int32, the voxel of every grouped row (voxel_capacity behind P'); run_off
 *   (voxel_capacity + 1) int32, rows [run_off[v], run_off[v + 1]) are voxel v's (a voxel no point carries: an empty run;
 *   entries behind N repeat P'); sizes (2) int32 = [N, P'] left on the device for ONE host read.  num_voxels_dev: the device
 *   word mssvt_voxelize left, or NULL: N = voxel_capacity.  An id outside [0, N) is dropped.  workspace: 16-byte aligned,
 *   mssvt_vfe_group_workspace_bytes(P, voxel_capacity) bytes (0: size refused).
 * mssvt_vfe_augment (ref :96-112, scatter_mean of :98), forward only: out (num_rows, C) f32, C = num_point_features +
 *   3 with_cluster_center + 3 with_voxel_center + with_distance, row r from point order[r] of voxel row_voxel[r]:
 *   [p[1 .. npf], xyz - mean_xyz(voxel), xyz - (cell * voxel_size + offset), |xyz|]; the mean from exact 64-bit fixed-point
 *   sums (mssvt_voxel_mean_xyz's arithmetic).  voxel_coords (N, 4) int32 [b, z, y, x]; host_*3: HOST float[3], offset =
 *   voxel_size / 2 + range_min; mean3_scratch (N, 3) f32, needed with the cluster centre.  A row whose point or voxel index
 *   is out of range is written as zeros.
 * mssvt_vfe_run_max_forward: x (num_rows, F) f32, run_off (num_voxels + 1) with run_off[0] = 0, ascending,
 *   run_off[num_voxels] = num_rows.  concat != 0 (PFNLayerV2 :44-52): out (num_rows, 2F), row r = [x[r] ; max over r's run];
 *   concat == 0 (ref :128-129): out (num_voxels, F) the maxima, an empty run a zero row.  The maximum of a run is taken from
 *   its rows alone (never seeded with zero).  Two launches: the pieces of runs longer than MSSVT_VFE_TRAIN_CHUNK rows, then
 *   the runs.  parts: mssvt_vfe_run_parts_floats(num_rows, F) floats, no need to clear.
 * mssvt_vfe_run_max_backward: grad_x (num_rows, F).  concat != 0: saved = the forward's output (num_rows, 2F) (it holds x and
 *   the broadcast maximum; maxima unused), grad_out (num_rows, 2F): gm = sum over the run's rows of grad_out[:, F:] in
 *   ascending row order, grad_x[r] = grad_out[r, :F] + (x[r] == max ? gm / count : 0), count = rows of the run equal to the
 *   maximum (-0 == +0).  concat == 0: saved = x, maxima (num_voxels, F) the forward's output, grad_out (num_voxels, F):
 *   grad_x[r] = x[r] == max ? grad_out[v] / count : 0.  Non-finite inputs are not specified.
 * F: a multiple of 4 in [4, 256]; float rows 16-byte aligned; rows and points below 2^31 - 256 (MSSVT_E_TOOLARGE beyond);
 * bad sizes / null / unaligned pointers: MSSVT_E_BADARG before any launch.                                                */
#define MSSVT_VFE_TRAIN_CHUNK 128
long long mssvt_vfe_group_workspace_bytes(long long num_points, int voxel_capacity);
int mssvt_vfe_group(const int *point_voxel, long long num_points, int voxel_capacity, const int *num_voxels_dev,
                    int *order, int *row_voxel, int *run_off, int *sizes, void *workspace, long long workspace_bytes,
                    void *stream);
int mssvt_vfe_augment(const float *points, int point_stride, long long num_points, const int *order,
                      const int *row_voxel, const int *run_off, int num_rows, int num_voxels, const int *voxel_coords,
                      const float *host_voxel_size3, const float *host_offset3, int num_point_features,
                      int with_cluster_center, int with_voxel_center, int with_distance, float *mean3_scratch, float *out,
                      void *stream);
long long mssvt_vfe_run_parts_floats(int num_rows, int F);
int mssvt_vfe_run_max_forward(const float *x, const int *run_off, int num_rows, int num_voxels, int F, int concat,
                              float *parts, float *out, void *stream);
int mssvt_vfe_run_max_backward(const float *saved, const float *maxima, const float *grad_out, const int *run_off,
                               int num_rows, int num_voxels, int F, int concat, float *parts, float *grad_x, void *stream);

/* BatchNorm2d in TRAINING mode with an optional ReLU behind it (csrc/bn_train.hip; the BatchNorm2d + ReLU pairs of
 * BaseBEVBackbone and HeightCompression) on dense channels-last fp32
 * tensors seen as P = B H W rows of C channels, C in {32, 64, 128, 256}.  Three launches each way, no float atomics, no host
 * read, no host synchronisation; every sum has one fixed order, so results are bit-identical from call to call.
 * The rows are cut into pieces of mssvt_bn_train_piece_rows(C) = 8192 / C rows (a function of C alone; 0: width not covered);
 * a workgroup owns mssvt_bn_train_run_pieces(P, C) = ceil(pieces / 1024) consecutive pieces (0: refused).
 * mssvt_bn_train_workspace_bytes: ((pieces + 2 workgroups) C + 2 C) * 4, or 0 for P < 2, P >= 2^31 or an uncovered width; the
 *   workspace is written before it is read, its contents on entry do not matter.
 * mssvt_bn_train_fwd: x, y (P, C); gamma, beta, running_mean, running_var, save_mean, save_invstd (C).  Per channel: mean and
 *   the biased variance var of the P values (pivot-shifted sums per piece, merged in piece order per workgroup and then in
 *   workgroup order), save_mean = mean,
 *   save_invstd = 1 / sqrt(var + eps) (IEEE division and square root), running_mean = (1 - momentum) running_mean +
 *   momentum mean, running_var = (1 - momentum) running_var + momentum var P / (P - 1), both in place;
 *   y = (x - mean) save_invstd gamma + beta, max(., 0) behind it if relu != 0 (a NaN stays a NaN).
 * mssvt_bn_train_bwd: dy, dx (P, C); dgamma, dbeta (C).  g = dy where relu == 0 or the forward's pre-activation, recomputed
 *   from x bit for bit, is > 0, else 0 (y is not read); dbeta = sum g, dgamma = sum g xhat, xhat = (x - mean) save_invstd,
 *   dx = gamma save_invstd (g - dbeta / P - xhat dgamma / P).  Linear in dy: scaling dy by a power of two scales all three
 *   bit for bit.
 * Null / unaligned (16 bytes) pointers, P < 2, C < 1: MSSVT_E_BADARG; an uncovered width or P >= 2^31: MSSVT_E_TOOLARGE;
 * neither launches anything.                                                                                           */
int mssvt_bn_train_supported(int C);
int mssvt_bn_train_piece_rows(int C);
int mssvt_bn_train_run_pieces(long long P, int C);
long long mssvt_bn_train_workspace_bytes(long long P, int C);
int mssvt_bn_train_fwd(const float *x, long long P, int C, const float *gamma, const float *beta, float eps, float momentum,
                       float *running_mean, float *running_var, int relu, float *y, float *save_mean, float *save_invstd,
                       void *workspace, void *stream);
int mssvt_bn_train_bwd(const float *x, const float *dy, long long P, int C, const float *gamma, const float *beta,
                       const float *save_mean, const float *save_invstd, int relu, float *dx, float *dgamma, float *dbeta,
                       void *workspace, void *stream);

/* ======================================================================== *
 * Part 6 -- timing-only launches (csrc/ceiling.hip; no reference counterpart, nothing reads their output): the byte and
 *           instruction mix of k_ffn_ws / k_attn_kvh on the frame's real tables with every dependency between the
 *           phases removed -- the ceiling of the structure, reported by bench.py as roofline.ceiling_us.
 * ======================================================================== */
int mssvt_ceiling_ffn_ws(int n_rows, const float *x_in, const int *tab_row, const float *tab_w, const float *attn,
                         const void *fragments_256k, float *y, float *y_norm, void *stream);
/* round 6: the same launch with the mix as a parameter -- variant = 100 * mode + filler index; mode 0 no matrix instructions,
 * 1 = 48 v_mfma_f32_16x16x32_f16 per wave and 16-row tile (the product's), 2 = 48 v_mfma_f32_32x32x16_f16 per wave and
 * 32-row tile (the same FLOP per row); filler index -> {0, 72, 144, 216, 288, 400} vector instructions per wave and tile. */
int mssvt_ceiling_ffn_mix(int variant, int n_rows, const float *x_in, const int *tab_row, const float *tab_w,
                          const float *attn, const void *fragments_256k, float *y, float *y_norm, void *stream);
int mssvt_ceiling_attn_kvh(int C, int c0_group0, int c0_group1, int K, const float *xhat, const float *kmeta0,
                           const float *kmeta1, const int *perm, const int *num_active_dev, const int *q_off,
                           const int *nq_valid, int row_capacity, int win_capacity, float *qbuf, void *stream);

/* round 6: variant 1 = the mix of "Wv applied at the end of the window launch" (24 more matrix + ~40 more vector
 * instructions per pass of 4 queries, the hand-off a quarter of the bytes); variant 0 = mssvt_ceiling_attn_kvh.          */
int mssvt_ceiling_attn_kvh_variant(int variant, int C, int c0_group0, int c0_group1, int K, const float *xhat,
                                   const float *kmeta0, const float *kmeta1, const int *perm, const int *num_active_dev,
                                   const int *q_off, const int *nq_valid, int row_capacity, int win_capacity, float *qbuf,
                                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MSSVT_HIP_H */
