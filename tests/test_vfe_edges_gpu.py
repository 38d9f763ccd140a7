"""DynamicVFE's inference kernels (csrc/voxelize.hip, csrc/vfe.hip, csrc/pfn_fused.hip, csrc/pfn_sorted.hip) through the C
ABI against the float64 statements of tests/vfe_ref.py, on hand-built run layouts at the sizes where their code paths switch.

Every buffer a call writes or uses as scratch is filled with 0xFF bytes first (NaN as floats, -1 as ints) and carries spare
rows behind its end: nothing of the fill may reach a result, and the spare rows must come back untouched.
Each of the two PFN entry points is held to the statement ON ITS OWN (tests/test_vfe_gpu.py compares them with each other).
The bounds are derived in tests/vfe_ref.py; the integer family is exact (equal values) and the cluster centres bit for bit.
Worst |err| / bound measured on an MI355X (each test prints its own), the same for both paths: x1 0.43, m1 0.40, out 0.04
for the unit, 2^30 and signed families and 0.48 for the 2^-30 family."""
import numpy as np
import pytest
import torch

from mssvt_amd import _lib, synthetic
from tests import vfe_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
RANGE, VS, GRID = synthetic.POINT_CLOUD_RANGE, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE
OFF = [VS[k] / 2 + RANGE[k] for k in range(3)]
DY_VS, DY_MIN, DY_GRID, DY_OFF = ref.DY_VS, ref.DY_MIN, ref.DY_GRID, ref.DY_OFF  # the integer family's dyadic geometry
PRM_KEYS = ("W1", "b1", "g1", "h1", "mu1", "var1", "eps1", "W2", "b2", "g2", "h2", "mu2", "var2", "eps2")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ff(*shape, dtype=torch.float32, word=-1):
    """A device tensor of 0xFF bytes (or of another 32-bit word)."""
    n = int(np.prod(shape)) * (2 if dtype == torch.int64 else 1)
    return torch.full((max(n, 1),), word, dtype=torch.int32, device=DEV).view(dtype)[:int(np.prod(shape))].view(*shape)


def untouched(t, word=-1):
    return bool((t.contiguous().view(torch.int32) == word).all())


HUGE = 0x7F7F7F7F  # 3.39e38 as a float, a large positive int: what an integer atomic max on a row nobody zeroed would keep


def geometry(kind):
    return (DY_VS, DY_MIN, DY_GRID, DY_OFF) if kind == "int" else (VS, RANGE[:3], GRID, OFF)


def case(runs, outside, kind, seed, spread=3):
    vs, lo, grid, off = geometry(kind)
    pts, pv, coords = ref.layout_points(runs, outside, seed, vs, lo, grid, dyadic=kind == "int", spread=spread)
    return dict(pts=pts, pv=pv, coords=coords, N=len(runs), vs=vs, off=off, prm=ref.params(kind, seed + 100), kind=kind)


def _layer_args(prm_d, prm):
    return [prm[k] if k.startswith("eps") else _lib.ptr(prm_d[k]) for k in PRM_KEYS]


def run_sorted(c, out_word=-1):
    P, N = len(c["pv"]), c["N"]
    prm_d = {k: dev(v) for k, v in c["prm"].items() if not k.startswith("eps")}
    pts, pv, coords = dev(c["pts"]), dev(c["pv"]), dev(c["coords"])
    n_ws = int(_lib.lib().mssvt_pfn_sorted_workspace_ints(P, N))
    ws, x1, m1, out = ff(n_ws + 4, dtype=torch.int32), ff(P + 8, 64), ff(N + 1, 64), ff(N + 1, 128, word=out_word)
    _lib.call("mssvt_pfn_sorted_64_128", _lib.ptr(pts), 6, P, _lib.ptr(pv), N, _lib.ptr(coords), _lib.f3(c["vs"]), _lib.f3(c["off"]),
              *_layer_args(prm_d, c["prm"]), _lib.ptr(ws), _lib.ptr(x1), _lib.ptr(m1), _lib.ptr(out), _lib.stream())
    torch.cuda.synchronize()
    assert untouched(ws[n_ws:]) and untouched(x1[P:]) and untouched(m1[N:]) and untouched(out[N:], out_word)
    return dict(out=out[:N], m1=m1[:N])


def run_fused(c):
    P, N = len(c["pv"]), c["N"]
    prm_d = {k: dev(v) for k, v in c["prm"].items() if not k.startswith("eps")}
    pts, pv, coords = dev(c["pts"]), dev(c["pv"]), dev(c["coords"])
    mean, cnt, scratch = ff(N + 1, 3), ff(N + 1, dtype=torch.int32), ff(3 * N + 3, dtype=torch.int64)
    _lib.call("mssvt_voxel_mean_xyz", _lib.ptr(pts), 6, P, _lib.ptr(pv), N, _lib.ptr(mean), _lib.ptr(cnt), _lib.ptr(scratch), _lib.stream())
    x1, m1, x2, out = ff(P + 1, 64), ff(N + 1, 64), ff(P + 1, 128), ff(N + 1, 128)
    _lib.call("mssvt_pfn_fused_64_128", _lib.ptr(pts), 6, P, _lib.ptr(pv), N, _lib.ptr(mean), _lib.ptr(coords), _lib.f3(c["vs"]),
              _lib.f3(c["off"]), *_layer_args(prm_d, c["prm"]), _lib.ptr(x1), _lib.ptr(m1), _lib.ptr(x2), _lib.ptr(out), _lib.stream())
    torch.cuda.synchronize()
    for t, n in ((mean, N), (cnt, N), (scratch, 3 * N), (x1, P), (m1, N), (x2, P), (out, N)):
        assert untouched(t[n:])
    outside = dev(c["pv"] < 0)
    # STRICTER than the C ABI promises (x1 / x2 are scratch): today the rows of points outside the grid are never written, and
    # a kernel that stored them would be doing work nobody reads.  A change that writes them on purpose may drop this line.
    assert untouched(x1[:P][outside]) and untouched(x2[:P][outside])
    return dict(out=out[:N], m1=m1[:N], x1=x1[:P], mean3=mean[:N], count=cnt[:N])


def hold(got, want, lim, kind, what):
    """got (device or numpy) against the statement: for the integer family EQUAL VALUES (no rounding anywhere; -0.0 == +0.0,
    the statement does not define the sign of a zero behind the ReLU), else inside the bound."""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert np.isfinite(got).all(), what
    if kind == "int":
        assert np.array_equal(got.astype(np.float64), want), what
        return 0.0
    ratio = float((np.abs(got.astype(np.float64) - want) / np.maximum(lim, 1e-300)).max())
    print("%s: worst |err| / bound = %.3f" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)
    return ratio


def check_both_paths(c, what):
    keep = c["pv"] >= 0
    st = ref.pfn_statement(c["pts"][keep], c["pv"][keep], c["N"], c["coords"], c["vs"], c["off"], c["prm"])
    if c["kind"] == "int":  # the operands ARE exact: a float32 evaluation in kernel order gives the statement's bits
        emu = ref.pfn_emulated(c["pts"][keep], c["pv"][keep], c["N"], c["coords"], c["vs"], c["off"], c["prm"])
        assert all(np.array_equal(e.astype(np.float64), st[k]) for e, k in zip(emu, ("x1", "m1", "out"))), what
    s = run_sorted(c)
    hold(s["out"], st["out"], st["b_out"], c["kind"], what + " sorted out")
    hold(s["m1"], st["m1"], st["b_m1"], c["kind"], what + " sorted m1")
    # the rows that take integer atomic max must be the rows k_ps_place zeroed: on any other row this fill would survive
    hold(run_sorted(c, HUGE)["out"], st["out"], st["b_out"], c["kind"], what + " sorted out (out pre-filled with 0x7F bytes)")
    f = run_fused(c)
    assert np.array_equal(f["mean3"].cpu().numpy().view(np.int32), st["mean3"].view(np.int32)), what  # exact, bit for bit
    assert np.array_equal(f["count"].cpu().numpy(), np.bincount(c["pv"][keep], minlength=c["N"])), what
    hold(f["out"], st["out"], st["b_out"], c["kind"], what + " fused out")
    hold(f["m1"], st["m1"], st["b_m1"], c["kind"], what + " fused m1")
    hold(f["x1"].cpu().numpy()[keep], st["x1"], st["b_x1"], c["kind"], what + " fused x1")


# ---------------------------------------------------------------------------------------------------------
# the PFN entry points
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ref.FAMILIES)
@pytest.mark.parametrize("layout", sorted(ref.LAYOUTS))
def test_run_layouts(layout, kind):
    runs, outside = ref.LAYOUTS[layout]
    check_both_paths(case(runs, outside, kind, 3 + len(layout)), "%s/%s" % (layout, kind))


@pytest.mark.parametrize("per_voxel", [1, 2])
@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 2049])
def test_voxel_counts_at_the_scan_edges(N, per_voxel):
    """k_ps_scan1 scans 1024 counts per block (four per thread), k_ps_scan2 the block totals: one block short by one, full,
    one over, and three blocks of which the last holds one count."""
    check_both_paths(case([per_voxel] * N, (2, 5, 2), "unit", N + per_voxel), "N=%d x %d" % (N, per_voxel))
    if N in (1025, 2049):
        check_both_paths(case([per_voxel] * N, (0, 3, 0), "int", N, spread=1), "N=%d x %d int" % (N, per_voxel))


def test_second_pass_of_the_block_total_scan():
    """N = 1024 x 1024 + 1 voxels: the smallest count at which k_ps_scan2 takes a second pass of 1024 block totals (with its
    carry).  One point per voxel but for runs of two on either side of voxel 1024 x 1024; the statement on sampled voxels
    (first, last, around every multiple of 1024 x 1024 and around multiples of 1024), isfinite on the device for the rest.
    Sorted path only: k_ps_scan2 is its kernel (about 1 GB of device memory, one launch sequence)."""
    M = 1024 * 1024
    N = M + 1
    runs = np.ones(N, np.int64)
    runs[[5, M - 3, M - 1, M]] = 2
    c = case(runs, (1, 6, 1), "unit", 77, spread=3)
    near = np.arange(-2, 3)
    picks = [np.arange(4), np.arange(N - 4, N), M + near[near <= 0], M - 3 + near]
    picks += [k * 1024 + near[1:4] for k in (1, 2, 3, 511, 512, 513, 1000, 1022, 1023)]
    picks += [np.random.default_rng(0).integers(0, N, 150)]
    voxels = np.unique(np.clip(np.concatenate(picks), 0, N - 1))
    rows, local = ref.subset(c["pv"], voxels)
    st = ref.pfn_statement(c["pts"][rows], local, len(voxels), c["coords"][voxels], c["vs"], c["off"], c["prm"])
    s = run_sorted(c)
    assert bool(torch.isfinite(s["out"]).all()) and bool(torch.isfinite(s["m1"]).all())
    idx = dev(voxels)
    hold(s["out"][idx], st["out"], st["b_out"], "unit", "N=2^20+1 sorted out")
    hold(s["m1"][idx], st["m1"], st["b_m1"], "unit", "N=2^20+1 sorted m1")


def test_more_than_one_task_per_wave():
    """More sorted rows than 16 waves x 16 rows x CU count: k_ps_pfn2's waves take a second window (the one-task-ahead
    prefetch branch runs) and k_pfn2_h's a second tile.  Mixed run lengths, so that windows are cut at every offset."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    target = cus * 256 + 300 + 7
    pattern = [1, 2, 3, 17, 1, 40, 5, 16, 1, 1, 9, 33, 2, 15, 8, 1, 64, 7]
    runs = (pattern * (target // sum(pattern) + 1))
    tot = np.cumsum(runs)
    n = int(np.searchsorted(tot, target))
    runs = runs[:n] + ([target - int(tot[n - 1])] if target > tot[n - 1] else [])
    assert sum(runs) == target and target > 16 * 16 * cus
    check_both_paths(case(runs, (3, 200, 3), "unit", 5), "rows=%d (%d CUs)" % (target, cus))


# ---------------------------------------------------------------------------------------------------------
# the generic reductions of csrc/vfe.hip
# ---------------------------------------------------------------------------------------------------------

def _voxel_max(feat, pv, N):
    P, F = feat.shape
    out, feat_d, pv_d = ff(N + 1, F), dev(feat), dev(pv)
    _lib.call("mssvt_voxel_max", _lib.ptr(feat_d) if P else None, F, P, _lib.ptr(pv_d) if P else None, N, _lib.ptr(out), _lib.stream())
    torch.cuda.synchronize()
    assert untouched(out[N:])
    return out[:N].cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.int32), np.asarray(b, np.float32).view(np.int32))


@pytest.mark.parametrize("F", [1, 63, 64, 65, 130])
def test_voxel_max_and_mean_vs_statement(F):
    """Channels either side of the 64 lanes a point's wave strides by; voxels with no point (-inf, mean 0, count 0); points
    outside the grid; values of both signs, both zeros and both infinities."""
    rng = np.random.default_rng(F)
    P, N = 777, 61
    pv = rng.integers(-1, N, P).astype(np.int32)
    pv[pv == 7] = 8  # voxel 7 stays empty
    pv[pv == N - 1] = -1  # and the last one
    feat = rng.standard_normal((P, F)).astype(np.float32)
    feat[rng.random((P, F)) < 0.1] = -0.0
    feat[rng.random((P, F)) < 0.05] = 0.0
    feat[3, 0], feat[4, 0] = np.inf, -np.inf
    feat[pv == 9] = -np.abs(feat[pv == 9]) - 1  # a voxel of negative values only
    got = _voxel_max(feat, pv, N)
    assert _same_bits(got, ref.voxel_max(feat, pv, N))
    assert np.all(got[7] == -np.inf) and np.all(got[N - 1] == -np.inf)
    pts = np.concatenate([np.zeros((P, 1)), rng.uniform(-75, 75, (P, 3))], 1).astype(np.float32)
    mean, cnt, scratch = ff(N + 1, 3), ff(N + 1, dtype=torch.int32), ff(3 * N + 3, dtype=torch.int64)
    pts_d, pv_d = dev(pts), dev(pv)
    _lib.call("mssvt_voxel_mean_xyz", _lib.ptr(pts_d), 4, P, _lib.ptr(pv_d), N, _lib.ptr(mean), _lib.ptr(cnt), _lib.ptr(scratch), _lib.stream())
    torch.cuda.synchronize()
    want, wcnt = ref.cluster_centre(pts[pv >= 0, 1:4], pv[pv >= 0], N)
    assert _same_bits(mean[:N].cpu().numpy(), want) and np.array_equal(cnt[:N].cpu().numpy(), wcnt)
    assert wcnt[7] == 0 and np.all(want[7] == 0) and untouched(mean[N:]) and untouched(cnt[N:]) and untouched(scratch[3 * N:])


@pytest.mark.parametrize("P", [0, 40])
def test_voxel_reductions_without_a_point_inside(P):
    """P = 0, and every point outside the grid: -inf, mean 0, count 0 in every voxel."""
    N, F = 5, 65
    feat, pv = np.ones((P, F), np.float32), np.full(P, -1, np.int32)
    assert np.all(_voxel_max(feat, pv, N) == -np.inf)
    mean, cnt, scratch = ff(N + 1, 3), ff(N + 1, dtype=torch.int32), ff(3 * N + 3, dtype=torch.int64)
    pts_d, pv_d = dev(np.ones((P, 4), np.float32)), dev(pv)
    _lib.call("mssvt_voxel_mean_xyz", _lib.ptr(pts_d) if P else None, 4, P, _lib.ptr(pv_d) if P else None, N, _lib.ptr(mean),
              _lib.ptr(cnt), _lib.ptr(scratch), _lib.stream())
    torch.cuda.synchronize()
    assert bool((mean[:N] == 0).all()) and bool((cnt[:N] == 0).all()) and untouched(mean[N:]) and untouched(cnt[N:])


def test_voxel_max_orders_negative_zero():
    """-0.0 is a value like any other: a voxel whose only value is -0.0 holds -0.0 (not the -inf fill), {-1.0, -0.0} gives
    -0.0, {-0.0, +0.0} gives +0.0 in either arrival order.  (Routed by `v >= 0.0f` to the signed integer maximum, -0.0 -- bits
    INT_MIN -- lost to the bits of -inf and of every negative float: -inf and -1.0 came out.)"""
    feat = np.array([[-0.0], [-1.0], [-0.0], [-0.0], [0.0], [0.0], [-0.0], [-3.0]], np.float32)
    pv = np.array([0, 1, 1, 2, 2, 3, 3, 4], np.int32)
    got = _voxel_max(feat, pv, 6)[:, 0]
    want = np.array([-0.0, -0.0, 0.0, 0.0, -3.0, -np.inf], np.float32)
    assert _same_bits(got, want), got.tolist()
    assert _same_bits(ref.voxel_max(feat, pv, 6)[:, 0], want)


# ---------------------------------------------------------------------------------------------------------
# the voxelizer
# ---------------------------------------------------------------------------------------------------------

def _voxelize(pts, lo, vs, grid, B, capacity):
    P = len(pts)
    X, Y, Z = grid
    n_ws = int(_lib.lib().mssvt_voxelize_workspace_ints(B, X, Y, Z))
    ws, coords, pv, n_dev = ff(n_ws + 4, dtype=torch.int32), ff(capacity + 2, 4, dtype=torch.int32), ff(P + 1, dtype=torch.int32), ff(2, dtype=torch.int32)
    pts_d = dev(pts)
    _lib.call("mssvt_voxelize", _lib.ptr(pts_d), pts.shape[1], P, B, _lib.f3(lo), _lib.f3(vs), X, Y, Z, capacity, _lib.ptr(coords),
              _lib.ptr(pv), _lib.ptr(n_dev), _lib.ptr(ws), _lib.stream())
    torch.cuda.synchronize()
    assert untouched(ws[n_ws:]) and untouched(coords[capacity:]) and untouched(pv[P:]) and untouched(n_dev[1:])
    return coords[:capacity].cpu().numpy(), pv[:P].cpu().numpy(), int(n_dev[0])


def _points_in_cells(cell, lo, vs, grid, rng):
    """A point inside each cell (flat index over (b, x, y, z), z fastest), rows [b, x, y, z]."""
    X, Y, Z = grid
    cell = np.asarray(cell, np.int64)
    c = np.stack([(cell // (Y * Z)) % X, (cell // Z) % Y, cell % Z], 1)
    xyz = np.asarray(lo, np.float64) + (c + rng.uniform(0.2, 0.8, c.shape)) * np.asarray(vs, np.float64)
    return np.concatenate([(cell // (X * Y * Z))[:, None].astype(np.float64), xyz], 1).astype(np.float32)


def test_voxelizer_at_the_scan_block_boundaries_of_five_samples():
    """The project grid at batch size 5: 1,104,500 bitmap words, 1079 scan blocks -- k_vox_scan2 takes a second pass of 1024
    block totals (with its carry).  Points in the cells of words 0 and 1023 of blocks 0, 1, 1022 .. 1025 and the last one, bits
    0 and 31, and in the first and last cell of every sample; some cells twice; some points outside."""
    B, (X, Y, Z) = 5, GRID
    per = X * Y * Z
    nwords = (B * per + 31) // 32
    nblocks = (nwords + 1023) // 1024
    assert nblocks > 1025
    words = [b * 1024 + w for b in (0, 1, 1022, 1023, 1024, 1025, nblocks - 1) for w in (0, 1, 1022, 1023) if b * 1024 + w < nwords]
    cell = [w * 32 + bit for w in words for bit in (0, 31) if w * 32 + bit < B * per]
    cell += [s * per + k for s in range(B) for k in (0, per - 1)] + [B * per - 1]
    rng = np.random.default_rng(4)
    cell = np.asarray(cell + cell[::3], np.int64)  # every third cell holds two points
    pts = _points_in_cells(cell, RANGE[:3], VS, GRID, rng)
    junk = pts[:9].copy()
    junk[:3, 1] += 500.0
    junk[3:6, 0] = 5  # a sample id outside the batch
    junk[6:, 3] = -2.5
    pts = np.concatenate([junk[:4], pts, junk[4:]])[rng.permutation(len(pts) + 9)]
    want_c, want_pv = ref.voxelize(pts, RANGE[:3], VS, GRID, B)
    keep, _, key = ref.cells(pts, RANGE[:3], VS, GRID, B)
    assert set(key[keep].tolist()) == set(cell.tolist()) and int((~keep).sum()) == 9  # the statement's float32 cells are the intended ones
    got_c, got_pv, n = _voxelize(pts, RANGE[:3], VS, GRID, B, len(pts))
    assert n == len(want_c) == len(set(cell.tolist()))
    np.testing.assert_array_equal(got_c[:n], want_c)
    np.testing.assert_array_equal(got_pv, want_pv)


def test_voxelizer_tiny_grid_faces_and_capacity():
    """A (7, 5, 3) grid, two samples: 210 cells, so the seventh bitmap word is partial.  Every cell occupied, plus points
    exactly on voxel faces, on the range minimum and maximum and one float below / above them: the float32 expression of the
    statement decides where they fall.  Then a capacity below N: the count still reports N, the first rows are right, memory
    behind them is untouched."""
    grid, B = [7, 5, 3], 2
    lo, vs = [-1.12, -0.8, -0.28], [0.32, 0.32, 0.1875]
    rng = np.random.default_rng(2)
    inside = _points_in_cells(np.arange(B * 105), lo, vs, grid, rng)
    lo32, vs32 = np.asarray(lo, np.float32), np.asarray(vs, np.float32)
    faces = []
    for axis in range(3):
        for k in range(grid[axis] + 1):
            on = (lo32[axis] + np.float32(k) * vs32[axis]).astype(np.float32)
            for v in (on, np.nextafter(on, np.float32(-np.inf)), np.nextafter(on, np.float32(np.inf))):
                p = inside[(7 * k + axis) % len(inside)].copy()
                p[1 + axis] = v
                faces.append(p)
    pts = np.concatenate([inside, np.asarray(faces, np.float32)])[rng.permutation(len(inside) + len(faces))]
    pts = np.concatenate([pts, rng.uniform(0, 1, (len(pts), 2)).astype(np.float32)], 1)  # stride 6
    want_c, want_pv = ref.voxelize(pts, lo, vs, grid, B)
    N = len(want_c)
    assert N == 210 and int((want_pv < 0).sum()) >= 3  # (one float below the minimum on each axis, at the least)
    got_c, got_pv, n = _voxelize(pts, lo, vs, grid, B, len(pts))
    assert n == N
    np.testing.assert_array_equal(got_c[:n], want_c)
    np.testing.assert_array_equal(got_pv, want_pv)
    cap = 100
    got_c, got_pv, n = _voxelize(pts, lo, vs, grid, B, cap)  # (_voxelize asserts the rows behind `cap` untouched)
    assert n == N
    np.testing.assert_array_equal(got_c, want_c[:cap])
    np.testing.assert_array_equal(got_pv, want_pv)
