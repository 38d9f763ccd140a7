"""mssvt_voxel_tables (csrc/voxel_tables.hip): the interpolation tables built with one lane per (voxel, table) from a finished
plan are the tables mssvt_window_plan_two(num_tabs > 0) builds inside the plan kernel, byte for byte."""
import ctypes

import numpy as np
import pytest
import torch

from mssvt_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
WS = [[3, 3, 5], [7, 7, 7]]


def _block():
    from mssvt_amd.mssvt_backbone import MixedScaleSparseTransformerBlock
    return MixedScaleSparseTransformerBlock(cfg=None, in_channels=32, ff_channels=64, out_channels=32, num_heads=[2, 2],
                                            drop_path=0.0, window_size=WS, max_num_win1=45, max_num_win2=343, cbs_pattern=1,
                                            key_num_sample=32).to(DEV).eval()


def _scene(points, B, seed):
    """Synthetic voxels plus, per sample, the cases the tables must get right: a window with every cell occupied (full
    lists), a window that holds a single voxel far from everything else (one valid query, none in the other list), and
    voxels in the cells the window grid does not cover (x >= 468, z >= 30: in no list)."""
    X, Y, Z = synthetic.GRID_SIZE
    vc, _, _ = synthetic.voxelize_numpy(synthetic.make_batch_points(points, B, seed))
    extra = []
    for b in range(B):
        x0, y0, z0 = 3 * (60 + b), 3 * 70, 5 * 2  # a window of the 3 x 3 x 5 grid
        extra += [(b, z0 + dz, y0 + dy, x0 + dx) for dx in range(3) for dy in range(3) for dz in range(5)]
        extra += [(b, 7, 3 * 150 + 1, 3 * 2 + 1), (b, 31, 200, 200), (b, 30, 201, 201), (b, 3, 100, 469)]
    vc = np.concatenate([vc, np.asarray(extra, dtype=vc.dtype)], 0)
    key = ((vc[:, 0].astype(np.int64) * X + vc[:, 3]) * Y + vc[:, 2]) * Z + vc[:, 1]
    _, first = np.unique(key, return_index=True)  # sorted by (b, x, y, z), duplicates dropped
    return np.ascontiguousarray(vc[first])


def _plan(vc, B):
    from mssvt_amd import fused
    from mssvt_amd.mssvt_utils import SparseTensor
    blk = _block()
    sp = SparseTensor(features=torch.zeros(vc.shape[0], 32, device=DEV), indices=torch.from_numpy(vc).to(DEV),
                      spatial_shape=synthetic.GRID_SIZE, voxel_size=synthetic.VOXEL_SIZE,
                      point_cloud_range=synthetic.POINT_CLOUD_RANGE, batch_size=B, hash_size=200003)
    with torch.no_grad():
        p = fused.two_scale_plan(blk, sp, all_lists=True)
    return blk, sp, p


@pytest.fixture(scope="module", params=[1, 2], ids=["batch1", "batch2"])
def planned(request):
    B = request.param
    vc = _scene(3000 if B == 1 else 2000, B, 17)
    blk, sp, p = _plan(vc, B)
    torch.cuda.synchronize()
    return B, vc, blk, sp, p


def _tab_args(tabs, rows, ws):
    n = len(tabs)
    ia = lambda v: (ctypes.c_int * n)(*[int(x) for x in v])  # noqa: E731
    pa = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
    return (ctypes.c_int(n), ia([t[0] for t in tabs]), ia([t[1] for t in tabs]), ia([900000 + i for i in range(n)]),
            pa([rows[i] for i in range(n)]), pa([ws[i] for i in range(n)]))


# (list: 0 odd / 1 even / 2 win1, interpolation): every list with and without interpolation over the two groups
GROUPS = {"a": [(0, 1), (1, 1), (2, 1), (0, 0)], "b": [(1, 0), (2, 0), (2, 1), (0, 1)]}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_tables_per_voxel_are_the_plan_kernels_tables_byte_for_byte(planned, group):
    from mssvt_amd import _lib
    B, vc, blk, sp, p = planned
    tabs = GROUPS[group]
    N, cap = vc.shape[0], p.cap
    P = _lib.ptr
    # the tables of the plan kernel: rows pre-filled with -1 as its contract asks; weights of untouched voxels stay as they are
    want_row = torch.full((len(tabs), N, 4), -1, dtype=torch.int32, device=DEV)
    want_w = torch.zeros((len(tabs), N, 4), dtype=torch.float32, device=DEV)
    _lib.call("mssvt_window_plan_two", *p._plan_args, *_tab_args(tabs, want_row, want_w), _lib.stream())
    # the per-voxel kernel: vox_win from the plan without tables, then one lane per (voxel, table); rows need no pre-fill
    vox_win = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    _lib.call("mssvt_window_plan_two_vox", *p._plan_args, P(vox_win), _lib.stream())
    got_row = torch.full((len(tabs), N, 4), 7, dtype=torch.int32, device=DEV)
    got_w = torch.zeros((len(tabs), N, 4), dtype=torch.float32, device=DEV)
    f3 = lambda v: (ctypes.c_float * 3)(*[float(x) for x in v])  # noqa: E731
    _lib.call("mssvt_voxel_tables", ctypes.c_int(N), P(sp.indices), P(vox_win), P(p.nq_valid), ctypes.c_int(cap),
              P(p.qmeta_odd), P(p.qmeta_even), P(p.qmeta_win1), ctypes.c_int(blk.max_num_odd), ctypes.c_int(blk.max_num_even),
              ctypes.c_int(blk.max_num_win1), f3(sp.voxel_size), f3(sp.point_cloud_range[0:3]), *_tab_args(tabs, got_row, got_w),
              ctypes.c_int(0), None, None, None, _lib.stream())
    torch.cuda.synchronize()
    nw = int(p.num_wins.item())
    nq = p.nq_valid.cpu().numpy()[:, :nw]
    vw = vox_win.cpu().numpy()
    # the scene holds what it was built to hold
    assert ((nq[2] >= 1) & (nq[2] <= 2)).any(), "a window with one or two valid queries"
    assert (((nq[0] == 0) | (nq[1] == 0)) & (nq[2] > 0)).any(), "a window with none in a list"
    assert (vw < 0).any(), "a voxel in no win1 list"
    assert (nq[2] == blk.max_num_win1).any() and (nq[0] == blk.max_num_odd).any() and (nq[1] == blk.max_num_even).any(), \
        "a window whose list is full"
    assert (vw >= 0).sum() == nq[2].sum() and vw.max() == nw - 1
    assert np.array_equal(got_row.cpu().numpy().view(np.uint8), want_row.cpu().numpy().view(np.uint8))
    assert np.array_equal(got_w.cpu().numpy().view(np.uint8), want_w.cpu().numpy().view(np.uint8))
    # (not vacuous: every table updates voxels, the interpolating ones with three-row entries)
    rows = want_row.cpu().numpy()
    for i, (lst, interp) in enumerate(tabs):
        assert (rows[i, :, 0] >= 0).sum() == (nq[2].sum() if interp else nq[lst].sum())
