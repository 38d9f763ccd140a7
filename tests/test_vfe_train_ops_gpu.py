"""The VFE run operators on the MI355X (csrc/vfe_train.hip through mssvt_amd/vfe_train.py) against their numpy float64
statement (tests/vfe_train_ref.py), values and gradients, on hand-built run tables: lengths 0, 1, 2, 3, 15, 16, 17, 63, 64, 65,
CHUNK - 1, CHUNK, CHUNK + 1, 3 CHUNK + 5 and 1 000 mixed in one table (two long runs side by side), a table of a single run
(short and long), a table of length-1 runs; widths 4, 20, 32, 64, 128, 256.  Planted: exact two- and three-way ties from
duplicated rows (the gradient must be split), a column that is zero across a run, mixed +0 / -0, runs of negative values,
magnitudes of 1e30.  Non-finite inputs are not covered.

Tolerances are derived, not measured.  A maximum is a selection: the forward must EQUAL (``==``, so a zero's sign is free) the
statement on the same float32 inputs.  A gradient element that is a sum of n float32 terms t may differ by
(n - 1) 2^-24 sum|t| + 2^-23 |value| (the division by the tie count); the statement computes that bound per element and
every element is compared."""
import warnings

import numpy as np
import pytest
import torch

from mssvt_amd import vfe_train
from mssvt_amd.vfe_train import run_max, run_max_concat
from tests import vfe_train_ref as ref

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the MI355X")]
DEV = "cuda"


def dev(a, grad=False):
    return torch.from_numpy(np.array(a)).to(DEV).requires_grad_(grad)  # (a copy: the cases are read-only)


def poison(shape):
    """a NaN-filled tensor of an output's size goes back to the caching allocator: the next allocation of that size gets it"""
    t = torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
    del t


def compute(c, stale=False):
    """both operators and their gradients on case c"""
    x, off = dev(c["x"], grad=True), dev(c["run_off"])
    g_cat, g_max = dev(c["g_cat"]), dev(c["g_max"])
    rows, F = c["x"].shape
    N = len(c["run_off"]) - 1
    out = {}
    if stale:
        poison((rows, 2 * F))
    out["cat"] = run_max_concat(x, off)
    if stale:
        poison((rows, F))
    (out["gx_cat"],) = torch.autograd.grad(out["cat"], x, g_cat)
    if stale:
        poison((N, F))
    out["max"] = run_max(x, off)
    if stale:
        poison((rows, F))
    (out["gx_max"],) = torch.autograd.grad(out["max"], x, g_max)
    return {k: v.detach() for k, v in out.items()}


def assert_matches(got, c):
    for k in ("cat", "max"):
        a = got[k].cpu().numpy()
        assert a.shape == c[k].shape and a.dtype == np.float32
        assert (a.astype(np.float64) == c[k]).all(), (k, int((a.astype(np.float64) != c[k]).sum()))
    for k in ("gx_cat", "gx_max"):
        a = got[k].cpu().numpy().astype(np.float64)
        want, bound = c[k], c["bound" + k[2:]]
        assert a.shape == want.shape
        err = np.abs(a - want)
        worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
        print("%s: %d elements, max err / bound %.3g" % (k, err.size, worst))
        assert np.isfinite(a).all(), k
        assert (err <= bound).all(), (k, worst, int((err > bound).sum()))


@pytest.mark.parametrize("table,F", ref.CASES)
def test_values_and_gradients_match_the_statement(table, F):
    c = ref.make_case(table, F)
    assert_matches(compute(c), c)


@pytest.mark.parametrize("table,F", [("mixed", 64), ("mixed", 20), ("single_long", 64), ("ones", 4)])
def test_stale_memory_does_not_leak_into_any_output(table, F):
    c = ref.make_case(table, F)
    got = compute(c, stale=True)
    for k, v in got.items():
        assert not torch.isnan(v).any(), k
    assert_matches(got, c)


@pytest.mark.parametrize("table,F", [("mixed", 64), ("mixed", 256), ("single_long", 20)])
def test_bit_identical_across_calls_and_streams(table, F):
    c = ref.make_case(table, F)
    first = compute(c)
    again = compute(c)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        other = compute(c)
    side.synchronize()
    for k in first:
        assert torch.equal(first[k], again[k]), k
        assert torch.equal(first[k], other[k]), k


def upload_points(n, N, seed):
    rng = np.random.default_rng(seed)
    pts = np.concatenate((np.zeros((n, 1)), rng.uniform(-2, 2, (n, 5))), axis=1).astype(np.float32)
    return pts, rng.integers(0, 25, (N, 4)).astype(np.int32)


@pytest.mark.parametrize("name", sorted(ref.grouping_cases()))
def test_grouping_is_the_stable_sort(name):
    pv, N = ref.grouping_cases()[name]
    want_order, want_off = ref.group(pv, N)
    g = vfe_train.group_points(dev(pv), N)
    sizes = g.sizes.cpu().numpy()
    assert sizes.tolist() == [N, len(want_order)]
    np.testing.assert_array_equal(g.run_off.cpu().numpy(), want_off)
    np.testing.assert_array_equal(g.order.cpu().numpy()[:sizes[1]], want_order)
    np.testing.assert_array_equal(g.row_voxel.cpu().numpy()[:sizes[1]], pv[want_order])
    # with the voxel count left on the device (the module's form): tables sized for one voxel per point
    g2 = vfe_train.group_points(dev(pv), torch.tensor([N], dtype=torch.int32, device=DEV)) if N <= len(pv) else None
    if g2 is not None:
        assert g2.sizes.cpu().numpy().tolist() == [N, len(want_order)]
        np.testing.assert_array_equal(g2.run_off.cpu().numpy()[:N + 1], want_off)
        assert (g2.run_off.cpu().numpy()[N:] == len(want_order)).all()
        np.testing.assert_array_equal(g2.order.cpu().numpy()[:sizes[1]], want_order)
    again = vfe_train.group_points(dev(pv), N)
    assert torch.equal(again.order, g.order) and torch.equal(again.run_off, g.run_off)


@pytest.mark.parametrize("cluster,centre,distance,npf", [(True, True, False, 5), (True, True, True, 4), (False, True, False, 5),
                                                         (True, False, True, 3), (False, False, False, 5)])
def test_augmentation_matches_the_statement(cluster, centre, distance, npf):
    """float32 against float64: the cluster centre is exact to 2^-20 m plus one rounding, every column one or two float32
    operations on values below 16 -> 1e-5 absolute is 10 times the worst case (2^-20 + 3 2^-24 16)"""
    pv, N = ref.grouping_cases()["mixed"]
    pts, coords = upload_points(len(pv), N, 5)
    vs, off = [0.3, 0.2, 0.5], [-2.85, -2.9, -0.75]
    order, run_off = ref.group(pv, N)
    want = ref.augment(pts, order, run_off, coords, vs, off, npf, cluster, centre, distance)
    g = vfe_train.group_points(dev(pv), N)
    poison(want.shape)
    got = vfe_train.augment(dev(pts), g, len(order), N, dev(coords), vs, off, npf, cluster, centre, distance)
    assert got.shape == want.shape
    assert not torch.isnan(got).any()
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-5)
    again = vfe_train.augment(dev(pts), g, len(order), N, dev(coords), vs, off, npf, cluster, centre, distance)
    assert torch.equal(got, again)


def test_grouping_and_augmentation_are_bit_identical_on_a_side_stream():
    """every launch of group_points (the key pass, the library sort, the offsets) and of augment (cluster centre, rows) must go
    to the CURRENT stream: on a side stream, with the default stream kept busy, the results equal the default stream's."""
    pv, N = ref.grouping_cases()["large"]
    pts, coords = upload_points(len(pv), N, 9)
    rows = len(ref.group(pv, N)[0])
    pv_d, pts_d, coords_d = dev(pv), dev(pts), dev(coords)
    n_dev = torch.tensor([N], dtype=torch.int32, device=DEV)
    vs, off = [0.3, 0.2, 0.5], [-2.85, -2.9, -0.75]

    def run():
        g = vfe_train.group_points(pv_d, N)
        g2 = vfe_train.group_points(pv_d, n_dev)
        aug = vfe_train.augment(pts_d, g, rows, N, coords_d, vs, off, 5, True, True, True)
        return dict(order=g.order, run_off=g.run_off, sizes=g.sizes, row_voxel=g.row_voxel, aug=aug,
                    order2=g2.order, run_off2=g2.run_off, sizes2=g2.sizes, row_voxel2=g2.row_voxel)

    first = run()
    torch.cuda.synchronize()  # the inputs and the default stream's results are complete
    side = torch.cuda.Stream()
    # work on the default stream that a launch gone astray to it would queue behind, while its consumers on the side
    # stream go ahead
    busy = torch.randn((2048, 2048), device=DEV)
    for _ in range(8):
        busy = busy @ busy * 1e-3
    with torch.cuda.stream(side):
        other = run()
    side.synchronize()
    torch.cuda.synchronize()
    assert first["sizes"].tolist() == [N, rows]
    for k in first:
        assert torch.equal(first[k], other[k]), k


def test_the_operator_wrappers_do_not_wait_for_the_host():
    c = ref.make_case("mixed", 64)
    pv, N = ref.grouping_cases()["mixed"]
    pts, coords = upload_points(len(pv), N, 5)
    rows = len(ref.group(pv, N)[0])
    x, off, g_cat, g_max = dev(c["x"], grad=True), dev(c["run_off"]), dev(c["g_cat"]), dev(c["g_max"])
    pv_d, pts_d, coords_d = dev(pv), dev(pts), dev(coords)
    compute(c)  # the library is loaded
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=DEV).item()  # the mode is live
        cat = run_max_concat(x, off)
        (gx_cat,) = torch.autograd.grad(cat, x, g_cat)
        mx = run_max(x, off)
        (gx_max,) = torch.autograd.grad(mx, x, g_max)
        g = vfe_train.group_points(pv_d, N)
        aug = vfe_train.augment(pts_d, g, rows, N, coords_d, [0.3, 0.2, 0.5], [-2.85, -2.9, -0.75], 5)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    assert_matches(dict(cat=cat.detach(), max=mx.detach(), gx_cat=gx_cat, gx_max=gx_max), c)
    assert aug.shape == (rows, 11)


def test_the_fused_step_reads_the_host_once():
    from mssvt_amd import synthetic
    from mssvt_amd.dynamic_vfe import DynamicVFE
    torch.manual_seed(0)
    vfe = DynamicVFE(dict(NUM_FILTERS=[32, 64], FUSED_TRAIN=True), 5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE,
                     synthetic.POINT_CLOUD_RANGE).to(DEV).train()
    assert vfe.fused_train
    pts = torch.from_numpy(synthetic.make_batch_points(1500, 2, 0)).to(DEV)
    vfe(dict(points=pts, batch_size=2))["voxel_features"].sum().backward()  # warm: the library and the BatchNorm kernels
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            out = vfe(dict(points=pts, batch_size=2))
            out["voxel_features"].sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    reads = [str(w.message) for w in seen if "synchroniz" in str(w.message)]
    assert len(reads) == 1, reads


def test_arguments_are_status_codes():
    from mssvt_amd import _lib
    x = torch.zeros((8, 30), device=DEV)
    off = torch.tensor([0, 8], dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.MssvtHipError):
        run_max(x, off)  # a width that is no multiple of 4
    with pytest.raises(_lib.MssvtHipError):
        run_max_concat(torch.zeros((8, 260), device=DEV), off)
    empty = run_max(torch.zeros((0, 8), device=DEV), torch.zeros(3, dtype=torch.int32, device=DEV))
    assert empty.shape == (2, 8) and (empty == 0).all()
    assert run_max_concat(torch.zeros((0, 8), device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)).shape == (0, 16)
