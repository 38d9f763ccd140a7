"""tests/vfe_ref.py held to three things on the CPU: the restatement oracle/vfe_ref.py, the reference project's own runs
(tests/golden/dynamic_vfe_*.npz: fp32 library arithmetic, so inside the any-order fp32 bound), and a float32 evaluation in
kernel order with the split-fp16 halves emulated by truncation (inside the kernel bound on every operand family; the integer
family bit for bit)."""
import os

import numpy as np
import pytest

from mssvt_amd import synthetic
from oracle import vfe_ref as oracle_vfe
from tests import vfe_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RANGE, VS, GRID = synthetic.POINT_CLOUD_RANGE, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE
OFF = [VS[k] / 2 + RANGE[k] for k in range(3)]
DY_VS, DY_MIN, DY_GRID, DY_OFF = ref.DY_VS, ref.DY_MIN, ref.DY_GRID, ref.DY_OFF


def _worst(got, want, lim, what):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(lim, 1e-300)).max()) if err.size else 0.0
    print("%s: worst |err| / bound = %.3f" % (what, ratio))
    return ratio


def _statement_of_scene(points, B, sd, eps, range_, vs, grid, off=None):
    coords, pv = ref.voxelize(points, range_[:3], vs, grid, B)
    keep = pv >= 0
    off = [vs[k] / 2 + range_[k] for k in range(3)] if off is None else off
    prm = ref.params_from_state_dict(sd, eps)
    # the float mean of the reference (float64 accumulation rounded once, oracle/vfe_ref.py) in place of the fixed-point one
    return coords, ref.pfn_statement(points[keep], pv[keep], len(coords), coords, vs, off, prm, any_order=True, centre_slack=True)


def _random_sd(filters, seed):
    rng = np.random.default_rng(seed)
    sd, cin = {}, 11
    for i, c in enumerate(filters):
        p = "pfn.%d." % i
        sd[p + "0.weight"] = (rng.standard_normal((c, cin)) / cin ** 0.5).astype(np.float32)
        sd[p + "0.bias"] = (rng.standard_normal(c) * 0.1).astype(np.float32)
        sd[p + "1.weight"] = rng.standard_normal(c).astype(np.float32)
        sd[p + "1.bias"] = (rng.standard_normal(c) * 0.2).astype(np.float32)
        sd[p + "1.running_mean"] = (rng.standard_normal(c) * 0.3).astype(np.float32)
        sd[p + "1.running_var"] = rng.uniform(0.5, 1.5, c).astype(np.float32)
        cin = 2 * c
    return sd


@pytest.mark.parametrize("filters", [[64, 128], [16]])
def test_statement_against_the_restatement(filters):
    p = synthetic.make_batch_points(3000, 2, 5)
    p[::41, 1] += 500.0
    p[7:60, 1:4] = p[7, 1:4] + np.random.default_rng(0).uniform(-0.02, 0.02, (53, 3)).astype(np.float32)  # a crowded voxel
    p[7:60, 0] = p[7, 0]
    sd = _random_sd(filters, 3)
    want_f, want_c = oracle_vfe.dynamic_vfe_forward(sd, p, 5, VS, GRID, RANGE, len(filters))
    # (the restatement adds voxel_size / 2 + range_min in float32; the reference and the kernels' callers in Python floats)
    off = np.asarray(VS, np.float32) / 2 + np.asarray(RANGE[:3], np.float32)
    coords, st = _statement_of_scene(p, 2, sd, 1e-5, RANGE, VS, GRID, off)
    np.testing.assert_array_equal(coords, want_c)
    out, lim = (st["out"], st["b_out"]) if len(filters) == 2 else (st["m1"], st["b_m1"])
    assert _worst(want_f, out, lim, "restatement %s" % filters) <= 1.0
    assert np.isfinite(lim).all()


@pytest.mark.parametrize("name", ["dynamic_vfe_64_128", "dynamic_vfe_16"])
def test_statement_against_the_reference_run(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    sd = {k[3:]: d[k] for k in d.files if k.startswith("sd.")}
    coords, st = _statement_of_scene(d["points"], int(d["batch_size"]), sd, 1e-5, d["point_cloud_range"].tolist(),
                                     d["voxel_size"].tolist(), d["grid_size"].tolist())
    np.testing.assert_array_equal(coords, d["voxel_coords"])
    out, lim = (st["out"], st["b_out"]) if len(d["num_filters"]) == 2 else (st["m1"], st["b_m1"])
    assert _worst(d["voxel_features"], out, lim, name) <= 1.0


def test_cluster_centre_is_the_float64_mean_to_2_pow_minus_21():
    rng = np.random.default_rng(1)
    xyz = rng.uniform(-75, 75, (5000, 3)).astype(np.float32)
    v = rng.integers(0, 700, 5000)
    mean, cnt = ref.cluster_centre(xyz, v, 701)  # voxel 700 is empty
    s = np.zeros((701, 3))
    np.add.at(s, v, xyz.astype(np.float64))
    want = s[:700] / cnt[:700, None]
    assert np.all(np.abs(mean[:700] - want) <= 2.0 ** -21 + 2 * ref.U32 * np.abs(want))
    assert cnt[700] == 0 and np.all(mean[700] == 0)
    # order independent by construction: a permutation of the points gives the same bits
    perm = rng.permutation(5000)
    assert np.array_equal(ref.cluster_centre(xyz[perm], v[perm], 701)[0], mean)


@pytest.mark.parametrize("kind", [k for k in ref.FAMILIES if k != "int"])
def test_kernel_order_float32_evaluation_stays_inside_the_bound(kind):
    runs = [1, 7, 8, 9, 15, 16, 17, 40, 300, 1, 2, 3] + [1, 2] * 150
    pts, pv, coords = ref.layout_points(runs, (3, 20, 3), 11, VS, RANGE[:3], GRID)
    keep = pv >= 0
    prm = ref.params(kind, 7)
    st = ref.pfn_statement(pts[keep], pv[keep], len(runs), coords, VS, OFF, prm)
    x1, m1, out = ref.pfn_emulated(pts[keep], pv[keep], len(runs), coords, VS, OFF, prm)
    for name, got in (("x1", x1), ("m1", m1), ("out", out)):
        assert np.isfinite(st["b_" + name]).all()
        assert _worst(got, st[name], st["b_" + name], "%s (%s)" % (name, kind)) <= 1.0
    scale = {"big": 2.0 ** 30, "small": 2.0 ** -30}.get(kind, 1.0)
    assert scale < float(np.abs(st["x1"]).max()) < scale * 256  # the family is at the scale it is named for


def test_integer_family_is_exact():
    """Small integer weights on dyadic points: every sum of the statement is exact in float32, so the kernel-order
    evaluation, whatever its order, equals the float64 statement bit for bit -- and so must the kernels."""
    runs = [1, 7, 8, 9, 15, 16, 17, 40, 300, 1, 2, 3] + [1, 2] * 150
    pts, pv, coords = ref.layout_points(runs, (3, 20, 3), 13, DY_VS, DY_MIN, DY_GRID, dyadic=True)
    keep = pv >= 0
    prm = ref.params("int", 9)
    st = ref.pfn_statement(pts[keep], pv[keep], len(runs), coords, DY_VS, DY_OFF, prm)
    # the cluster centre is the dyadic point the layout put it at
    corner = coords[:, [3, 2, 1]] * np.asarray(DY_VS) + np.asarray(DY_MIN)
    assert np.array_equal(st["mean3"].astype(np.float64), corner + [0.125, 0.0625, 0.125])
    x1, m1, out = ref.pfn_emulated(pts[keep], pv[keep], len(runs), coords, DY_VS, DY_OFF, prm)
    for name, got in (("x1", x1), ("m1", m1), ("out", out)):
        assert np.array_equal(got.astype(np.float64), st[name]), name
    # every partial sum is a multiple of 2^-4 below 2^20: 24 bits hold it in any order
    f64 = st["f"].astype(np.float64)
    assert np.array_equal(f64 * 16, np.rint(f64 * 16))
    row = np.concatenate([st["x1"], st["m1"][pv[keep]]], 1)
    mag2 = np.abs(row) @ np.abs(prm["W2"].astype(np.float64)).T + np.abs(prm["b2"])
    assert float(mag2.max()) * 16 < 2 ** 24 and float(np.abs(st["out"]).max()) > 0


def test_layouts_are_what_their_names_say():
    for name, (runs, outside) in ref.LAYOUTS.items():
        pts, pv, coords = ref.layout_points(runs, outside, 1, VS, RANGE[:3], GRID)
        assert len(pv) == sum(runs) + sum(outside) and np.array_equal(np.bincount(pv[pv >= 0]), runs), name
        # the points lie in the cells the coordinates name (float32 cells of the voxelizer's statement), in key order
        c2, pv2 = ref.voxelize(pts[pv >= 0], RANGE[:3], VS, GRID, 1)
        assert np.array_equal(c2, coords) and np.array_equal(pv2, pv[pv >= 0]), name
        lead, mid, trail = outside
        assert np.all(pv[:lead] == -1) and (trail == 0 or np.all(pv[-trail:] == -1))
    totals = {n: sum(ref.LAYOUTS[n][0]) % 16 for n in ("total_mod16_0", "total_mod16_1", "total_mod16_15")}
    assert totals == {"total_mod16_0": 0, "total_mod16_1": 1, "total_mod16_15": 15}


def test_voxel_max_statement_orders_the_zeros():
    f = np.array([[-0.0], [-1.0], [-0.0], [0.0], [-0.0], [5.0]], np.float32)
    v = np.array([0, 1, 1, 2, 2, -1])
    out = ref.voxel_max(f, v, 4)
    assert out[:3, 0].tolist() == [0.0, 0.0, 0.0] and np.signbit(out[:, 0]).tolist() == [True, True, False, True]
    assert out[3, 0] == -np.inf
