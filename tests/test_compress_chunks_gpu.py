"""Chunk ends of k_cmp_ws computed once (mssvt_voxel_tables, csrc/voxel_tables.hip) instead of by every workgroup's own search:
mssvt_compress_ws_chunked writes the rows mssvt_compress_ws writes, bit for bit, and the ends tile the level."""
import ctypes

import numpy as np
import pytest
import torch

from mssvt_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _compress_block(ws, ns):
    from mssvt_amd.mssvt_backbone import MixedScaleSparseTransformerCompressBlock
    torch.manual_seed(0)
    return MixedScaleSparseTransformerCompressBlock(cfg=None, in_channels=128, ff_channels=256, out_channels=128, num_heads=[8],
                                                    drop_path=0.0, window_size=[list(ws)], max_num_win1=ns).to(DEV).eval()


def _voxels(points, B, seed, extra=()):
    X, Y, Z = synthetic.GRID_SIZE
    vc, _, _ = synthetic.voxelize_numpy(synthetic.make_batch_points(points, B, seed))
    if extra:
        vc = np.concatenate([vc, np.asarray(extra, dtype=vc.dtype)], 0)
    key = ((vc[:, 0].astype(np.int64) * X + vc[:, 3]) * Y + vc[:, 2]) * Z + vc[:, 1]
    _, first = np.unique(key, return_index=True)  # sorted by (b, x, y, z)
    return np.ascontiguousarray(vc[first])


def _run_both(vc, B, ws, ns, monkeypatch):
    """Runs the fused CompressBlock attention; at its mssvt_compress_ws call also computes the chunk ends and runs the chunked
    entry point on the same arguments.  Returns (rows of the search form, rows of the chunked form, ends, pair_win, nw, G)."""
    from mssvt_amd import fused
    from mssvt_amd.mssvt_utils import SparseTensor
    blk = _compress_block(ws, ns)
    feats = torch.randn(vc.shape[0], 128, generator=torch.Generator().manual_seed(5))
    sp = SparseTensor(features=feats.to(DEV), indices=torch.from_numpy(vc).to(DEV), spatial_shape=synthetic.GRID_SIZE,
                      voxel_size=synthetic.VOXEL_SIZE, point_cloud_range=synthetic.POINT_CLOUD_RANGE, batch_size=B,
                      hash_size=200003)
    out = {}
    real_call = fused._lib.call

    def call_spy(name, *a):
        if name != "mssvt_compress_ws":
            return real_call(name, *a)
        N, cap = (int(getattr(v, "value", v)) for v in (a[5], a[7]))  # (plain ints or ctypes objects)
        G = int(fused._lib.lib().mssvt_compress_ws_groups(cap))
        ends = torch.full((G + 1, 2), -7, dtype=torch.int32, device=DEV)
        real_call("mssvt_voxel_tables", ctypes.c_int(N), None, None, None, ctypes.c_int(0), None, None, None, ctypes.c_int(0),
                  ctypes.c_int(0), ctypes.c_int(0), None, None, ctypes.c_int(0), None, None, None, None, None, ctypes.c_int(G),
                  a[6], a[10], fused._lib.ptr(ends), a[23])
        got = torch.full((cap, 128), float("nan"), dtype=torch.float32, device=DEV)
        real_call("mssvt_compress_ws_chunked", *a[:22], fused._lib.ptr(got), fused._lib.ptr(ends), ctypes.c_int(G), a[23])
        out.update(N=N, G=G, ends=ends, got=got)
        return real_call(name, *a)
    monkeypatch.setattr(fused._lib, "call", call_spy)
    grabbed = {}
    real_tail = fused._compress_fused_tail

    def tail_spy(block, sp_, p, new):
        grabbed["new"], grabbed["p"] = new.clone(), p
        return real_tail(block, sp_, p, new)
    monkeypatch.setattr(fused, "_compress_fused_tail", tail_spy)
    with torch.no_grad():
        xhat = fused._norm1(blk, sp, sp.features)
        fused._compress_forward_fused(blk, sp, xhat, sp.features.contiguous())
    torch.cuda.synchronize()
    monkeypatch.setattr(fused._lib, "call", real_call)
    monkeypatch.setattr(fused, "_compress_fused_tail", real_tail)
    assert out, "the level did not take the one-launch form"
    p = grabbed["p"]
    nw = int(p.num_wins.item())
    return (grabbed["new"][:nw].cpu().numpy(), out["got"][:nw].cpu().numpy(), out["ends"].cpu().numpy(),
            p.pair_win.cpu().numpy()[:out["N"]], nw, out["G"])


def _check_ends(ends, pair_win, nw, G):
    n = pair_win.shape[0]
    assert ends.shape == (G + 1, 2)
    assert tuple(ends[0]) == (0, 0) and tuple(ends[G]) == (nw, n)
    assert (np.diff(ends[:, 0]) >= 0).all() and (np.diff(ends[:, 1]) >= 0).all()
    first_row = np.full(nw + 1, n, dtype=np.int64)  # first row of every window (windows are numbered in row order)
    listed = np.nonzero(pair_win >= 0)[0]
    np.minimum.at(first_row, pair_win[listed], listed)
    for w, r in ends[1:G]:
        assert (w, r) == (nw, n) or (0 <= w < nw and first_row[w] == r), (w, r)
    return np.unique(ends, axis=0).shape[0] - 1  # chunks that hold work


CASES = {
    # n not a multiple of 16, more 16-window groups than compute units
    "odd_rows": dict(points=20000, B=1, ws=(1, 1, 32), ns=32),
    # fewer 16-window groups than compute units: a workgroup per 16 windows of capacity
    "few_groups": dict(points=2500, B=1, ws=(1, 1, 32), ns=32),
    # pillar windows of 12 cells: cells z >= 24 lie above the window grid; the level begins and ends with such rows
    "unlisted_ends": dict(points=12000, B=1, ws=(1, 1, 12), ns=12, extra=[(0, 30, 0, 0), (0, 31, 0, 0), (0, 29, 469, 469)]),
    "batch2": dict(points=8000, B=2, ws=(1, 1, 32), ns=32),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_chunked_compress_writes_the_rows_of_the_searching_kernel(case, monkeypatch):
    c = CASES[case]
    vc = _voxels(c["points"], c["B"], 31, c.get("extra", ()))
    if vc.shape[0] % 16 == 0:
        vc = np.ascontiguousarray(np.delete(vc, vc.shape[0] // 2, 0))
    n = vc.shape[0]
    want, got, ends, pair_win, nw, G = _run_both(vc, c["B"], c["ws"], c["ns"], monkeypatch)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n % 16 != 0 and nw > 0
    if case == "few_groups":
        assert G == (n + 15) // 16 < cus
    else:
        assert G == cus
    if case == "unlisted_ends":
        assert pair_win[0] < 0 and pair_win[-1] < 0 and (pair_win >= 0).any()
    if case == "batch2":
        assert set(np.unique(vc[:, 0])) == {0, 1}
    busy = _check_ends(ends, pair_win, nw, G)
    assert busy >= min(G, nw // 16) // 2, "the ends leave most workgroups without work"
    assert np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
