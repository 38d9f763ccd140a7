"""The reference of tests/test_window_plan_forms_gpu.py (tests/window_plan_ref.py), checked without a GPU before it judges
a kernel:

  record      on a small synthetic scene and on the scenes of the golden files, the lists, sampled keys, masks and the 3-NN
              indices / distances equal what oracle/block_ref.block_forward records while it runs (the golden files: what the
              reference's own Block.forward recorded);
  coordinates `centres` is block_ref.with_coords, bit for bit;
  features    applying the reference's tab_row / tab_w to a random attention buffer reproduces block_ref's interpolated rows
              (block_ref.py:248-273 restated on that buffer), and its scattered attention rows without interpolation;
  weights     the float32 evaluation in the reference's own order stays inside the bound the kernel's weights are held to;
  levels      every hand-built level holds the fills it claims, window by window, and the sampler forms they reach;
  contract    the statement of mssvt_plan_order's contract accepts a correct answer and refuses broken ones.
"""
import os

import numpy as np
import pytest
import torch

from mssvt_amd import synthetic
from oracle import block_ref, cref
from tests import window_plan_ref as R

GOLDEN = ["block_odd_interp", "block_trunc", "block_evenwin_odd_interp"]


def _golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"), allow_pickle=False)
    d = {k: z[k] for k in z.files}
    return d, {k[3:]: v for k, v in d.items() if k.startswith("sd.")}, {k[3:]: v for k, v in d.items() if k.startswith("qt.")}


def _against_record(ref, rec, nq_list, interp):
    for k in ("win_ind", "ind_odd", "ind_even", "ind_win1", "ind_win2", "fps1", "fps2", "k_ind1", "k_ind2"):
        np.testing.assert_array_equal(ref[k], rec[k], err_msg=k)
    for g in (1, 2):
        np.testing.assert_array_equal(ref["k_mask%d" % g].astype(bool), rec["k_mask%d" % g])
    if interp:
        tab = ref["tabs"][0]
        np.testing.assert_array_equal(tab["nn_idx"], rec["nn_idx"])
        with np.errstate(invalid="ignore"):
            dist = np.maximum(np.sqrt(tab["nn_d2"]), np.float32(1e-10))
        np.testing.assert_array_equal(dist, rec["nn_dist"])


@pytest.mark.parametrize("name", GOLDEN)
def test_reference_equals_block_ref_record_and_the_reference_run(golden_dir, name):
    d, sd, tables = _golden(golden_dir, name)
    B, H = int(d["batch_size"]), int(d["hash_size"])
    sp = block_ref.SparseState(d["voxel_features"], d["voxel_coords"], d["grid_size"].tolist(), d["voxel_size"].tolist(),
                               d["point_cloud_range"].tolist(), B, H)
    ws, m1, m2, K = d["window_size"].tolist(), int(d["max_num_win1"]), int(d["max_num_win2"]), int(d["key_num_sample"])
    pattern, interp = int(d["cbs_pattern"]), bool(d["use_feature_interpolation"])
    rec = {}
    block_ref.block_forward(sd, "", sp, ws, d["num_heads"].tolist(), m1, m2, pattern, K, interp, tables=tables, record=rec)
    lst = {1: 0, 0: 1, 2: 2}[pattern]
    ref = R.plan_reference(d["voxel_coords"], B, sp.spatial_shape, sp.voxel_size, sp.point_cloud_range, ws[0], tables, m1, m2, K,
                           tabs=[(lst, int(interp), 10 ** 6)], hash_size=H)
    _against_record(ref, rec, lst, interp)
    # ... and what the reference's own Block.forward recorded
    np.testing.assert_array_equal(ref["win_ind"], d["rec.get_non_empty_window_center.0.win_ind"])
    for k in ("ind_odd", "ind_even", "ind_win1", "ind_win2"):
        np.testing.assert_array_equal(ref[k], d["rec.gather_two_window_voxels.0." + k])
    np.testing.assert_array_equal(ref["fps1"], d["rec.farthest_point_sample.0.fps_ind"])
    np.testing.assert_array_equal(ref["fps2"], d["rec.farthest_point_sample.1.fps_ind"])
    if interp:
        np.testing.assert_array_equal(ref["tabs"][0]["nn_idx"], d["rec.three_nn.0.idx"])


@pytest.fixture(scope="module")
def scene():
    B = 2
    vc, _, _ = synthetic.voxelize_numpy(synthetic.make_batch_points(1500, B, 5))
    rng = np.random.default_rng(3)
    return B, np.ascontiguousarray(vc, np.int32), rng.standard_normal((vc.shape[0], 32)).astype(np.float32)


@pytest.mark.parametrize("pattern,interp,m1,m2", [(1, True, 45, 343), (0, True, 45, 343), (2, False, 45, 343), (1, True, 6, 20)])
def test_reference_equals_block_ref_record_on_a_synthetic_scene(golden_dir, scene, pattern, interp, m1, m2):
    _, sd, _ = _golden(golden_dir, "block_odd_interp")
    B, vc, feats = scene
    ws, K = [[3, 3, 5], [7, 7, 7]], 32
    sp = block_ref.SparseState(feats, vc, synthetic.GRID_SIZE, synthetic.VOXEL_SIZE, synthetic.POINT_CLOUD_RANGE, B, R.HASH_SIZE)
    rec = {}
    block_ref.block_forward(sd, "", sp, ws, [2, 2], m1, m2, pattern, K, interp, record=rec)
    lst = {1: 0, 0: 1, 2: 2}[pattern]
    ref = R.plan_reference(vc, B, synthetic.GRID_SIZE, synthetic.VOXEL_SIZE, synthetic.POINT_CLOUD_RANGE, ws[0],
                           R.standard_tables(*ws), m1, m2, K, tabs=[(lst, int(interp), 10 ** 6)])
    _against_record(ref, rec, lst, interp)


def test_centres_are_with_coords_bit_for_bit(scene):
    _, vc, _ = scene
    a = R.centres(vc[:, [3, 2, 1]], synthetic.VOXEL_SIZE, synthetic.POINT_CLOUD_RANGE[0:3])
    b = block_ref.with_coords(vc, synthetic.POINT_CLOUD_RANGE, synthetic.VOXEL_SIZE)
    assert a.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    wsm = [synthetic.VOXEL_SIZE[i] * [3, 3, 5][i] for i in range(3)]
    a = R.centres(vc[:, [3, 2, 1]] // np.array([3, 3, 5]), wsm, synthetic.POINT_CLOUD_RANGE[0:3])
    w = vc.copy()
    w[:, 1:] = vc[:, 1:] // np.array([5, 3, 3])
    assert np.array_equal(a.view(np.int32), block_ref.with_coords(w, synthetic.POINT_CLOUD_RANGE, wsm).view(np.int32))


@pytest.mark.parametrize("lst,interp", [(0, 1), (1, 1), (2, 1), (0, 0), (1, 0), (2, 0)])
def test_tables_reproduce_block_refs_feature_rows(lst, interp):
    """block_ref.py:248-273 on a random attention buffer against  sum_j tab_w[v, j] * attn[tab_row[v, j]]  (cut lists: empty
    query slots, windows with fewer than three queries)."""
    cfg = R.configs()["w335_cut"]
    L = R.build_level(cfg)
    nq = [cfg.tables["odd"].shape[0], cfg.tables["even"].shape[0], cfg.max1][lst]
    C, N = 8, L.vc.shape[0]
    nw = R.reference_of(L)["nw"]
    zero_row = nw * nq  # the row behind the attention rows
    ref = R.reference_of(L, tabs=[(lst, interp, zero_row)])
    tab = ref["tabs"][0]
    rng = np.random.default_rng(7)
    q_ind, ind_w1 = [ref["ind_odd"], ref["ind_even"], ref["ind_win1"]][lst], ref["ind_win1"]
    attn = rng.standard_normal((nw, nq, C)).astype(np.float32) * (q_ind >= 0)[..., None]  # (masked query rows are zero)
    x_in = rng.standard_normal((N, C)).astype(np.float32)
    v_cnt, k_cnt = cref.bs_cnt(L.vc, L.B), cref.bs_cnt(ref["win_ind"], L.B)
    vcoord = block_ref.with_coords(L.vc, cfg.range, cfg.voxel_size)
    n1 = ind_w1.shape[1]
    if interp:
        known = np.ascontiguousarray(cref.grouping_operation(vcoord, v_cnt, q_ind, k_cnt).transpose(0, 2, 1))
        unknown = np.ascontiguousarray(cref.grouping_operation(vcoord, v_cnt, ind_w1, k_cnt).transpose(0, 2, 1))
        dist, idx = cref.three_nn(unknown, known)
        dist = np.maximum(dist, np.float32(1e-10))
        w = (np.float32(1.0) / dist).astype(np.float32)
        w = w / w.sum(-1, keepdims=True)
        grouped = cref.group_points(np.ascontiguousarray(attn.transpose(0, 2, 1)), idx)
        w1_fea = (torch.from_numpy(grouped) * torch.from_numpy(w).unsqueeze(1)).sum(-1).numpy()
        w1_fea = np.ascontiguousarray(w1_fea.transpose(0, 2, 1)).reshape(-1, C)
    attn_flat = attn.reshape(-1, C)
    want = x_in.copy()
    vs = ks = 0
    for b in range(L.B):
        nv, nk = int(v_cnt[b]), int(k_cnt[b])
        sel = np.concatenate([x_in[vs:vs + nv], np.zeros((1, C), np.float32)], axis=0)
        if interp:
            sel[ind_w1[ks:ks + nk].reshape(-1).astype(np.int64)] = w1_fea[ks * n1:(ks + nk) * n1]
        else:
            sel[q_ind[ks:ks + nk].reshape(-1).astype(np.int64)] = attn_flat[ks * nq:(ks + nk) * nq]
        want[vs:vs + nv] = sel[:-1]
        vs += nv
        ks += nk
    buf = np.concatenate([attn_flat, np.zeros((1, C), np.float32)], 0).astype(np.float64)
    upd = tab["updated"]
    got = x_in.astype(np.float64)
    got[upd] = (buf[tab["row"][upd, :3]] * tab["w"][upd, :3, None]).sum(1)
    assert upd.sum() == ((ind_w1 >= 0).sum() if interp else (q_ind >= 0).sum()) and (~upd).any()
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6 * float(np.abs(attn).max()))
    if interp:
        assert (tab["row"][upd, :3] == zero_row).any(), "an empty slot among the neighbours"
        assert (ref["nq_valid"][lst] < 3).any(), "a window with fewer than three queries"


@pytest.mark.parametrize("name", sorted(R.configs()))
def test_float32_weights_in_the_references_order_stay_inside_the_bound(name):
    cfg = R.configs()[name]
    ref = R.reference_of(R.build_level(cfg), tabs=[(0, 1, 0), (1, 1, 0), (2, 1, 0)])
    worst = 0.0
    for tab in ref["tabs"]:
        w64, w32 = R.weights_f64(tab["nn_d2"]), R.weights_f32(tab["nn_d2"]).astype(np.float64)
        ok = w64 > 0
        worst = max(worst, float((np.abs(w32 - w64)[ok] / w64[ok]).max()) / R.W_BOUND)
        assert (w32[w64 == 0] == 0).all() and (w32[w64 == 1] == 1).all()  # (1 - 5e-10 in float64 is 1 in float32: one way only)
    print("%s: worst float32 weight error / bound = %.3f" % (name, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", sorted(R.configs()))
def test_levels_hold_the_fills_they_claim(name):
    cfg = R.configs()[name]
    L = R.build_level(cfg)
    ref = R.reference_of(L)
    nv1, nv2 = ref["nq_valid"][2], ref["nv2"]
    assert np.array_equal(L.vc[:L.per_sample, 1:], L.vc[L.per_sample:, 1:]) and set(L.vc[:, 0]) == {0, 2}
    key = ((L.vc[:, 0].astype(np.int64) * cfg.grid[0] + L.vc[:, 3]) * cfg.grid[1] + L.vc[:, 2]) * cfg.grid[2] + L.vc[:, 1]
    assert (np.diff(key) > 0).all(), "sorted by (b, x, y, z), no duplicate"
    names = {n["name"] for n in L.named}
    for n in L.named:
        for b in (0, 2):
            w = R.window_of(ref, b, n["w"])
            assert nv1[w] == n["nv1"] and nv2[w] == n["nv2"], (n, nv1[w], nv2[w])
    assert set(L.fills1) <= {n["nv1"] for n in L.named} and set(L.fills2) <= {n["nv2"] for n in L.named}
    assert {"h1=all", "h=all", "centre", "centre_only", "no_centre", "pattern", "mirror_x", "mirror_y", "mirror_z", "corner_000",
            "edge_00", "face_x0", "corner_last", "face_top", "face_bottom"} <= names
    by = {n["name"]: n for n in L.named}
    assert by["centre"]["centre"] and by["centre_only"]["centre"] and not by["no_centre"]["centre"]
    assert by["h1=all"]["h2"] == 0 and by["h1=all"]["nv2"] == min(by["h1=all"]["h1"], cfg.max2)  # lives through its first scale only
    assert by["h=all"]["nv2"] == cfg.max2 and by["h=all"]["nv1"] == cfg.max1
    # voxels of the cells beyond the last full window are in no list
    assert bool(L.stray) == any(cfg.grid[i] % cfg.win1[i] for i in range(3))
    for p in L.stray:
        v = np.nonzero((L.vc[:, [3, 2, 1]] == np.array(p)).all(1))[0]
        assert v.shape[0] == 2
        for k in ("odd", "even", "win1"):
            assert (ref["owner_" + k][v] == -1).all()
    # the switches of the samplers, from the fills and the block sizes
    forms = R.sampler_forms(cfg, nv1, nv2)
    for n, bs, nv in ((cfg.max1, cfg.bs1, nv1), (cfg.max2, cfg.bs2, nv2)):
        for f in (bs - 1, bs, bs + 1, n - 1, n):
            assert f < 1 or f > n or (nv == f).any(), (n, bs, f)
    assert ("fast<false,4>" in forms) == (cfg.K > 64 and cfg.bs2 >= 2)
    for n, bs in ((cfg.max1, cfg.bs1), (cfg.max2, cfg.bs2)):  # a list that can outgrow the fast sampler reaches the register form
        assert ("regs<%d>" % max(1, bs // 64) in forms) or (n <= min(bs, 64) and bs >= 2)
    # windows with fewer entries than K: the "all further rounds tie" exit and the voxel-0 quirk keys
    assert (nv2 < cfg.K).any() and ref["quirk2"].any()
    # the empty middle sample: the same lists in samples 0 and 2, the feature rows apart by the sample's offset
    half = ref["nw"] // 2
    assert (ref["win_ind"][:half, 0] == 0).all() and (ref["win_ind"][half:, 0] == 2).all()
    for k in ("ind_odd", "ind_even", "ind_win1", "k_ind1", "k_ind2", "k_mask1", "k_mask2"):
        assert np.array_equal(ref[k][:half], ref[k][half:]), k
    for k in ("qmeta_odd_bits", "qmeta_even_bits", "qmeta_win1_bits", "kmeta1_bits", "kmeta2_bits"):
        a, b = ref[k][:half], ref[k][half:]
        assert np.array_equal(a[..., :3], b[..., :3])
        assert np.array_equal(np.where(a[..., 3] >= 0, a[..., 3] + L.per_sample, -1), b[..., 3]), k
    assert (ref["win_vstart"][:half] == 0).all() and (ref["win_vstart"][half:] == L.per_sample).all()


def test_plan_order_contract_accepts_the_answer_and_refuses_broken_ones():
    rng = np.random.default_rng(1)
    nw, nq = 40, 300
    nqv = rng.integers(0, 301, nw)
    nqv[3] = 0
    qm = np.zeros((nw, nq, 4), np.int32)
    qm[..., 3] = -1
    for w in range(nw):
        s = np.sort(rng.permutation(nq)[:nqv[w]])
        qm[w, s, 3] = 1000 * w + s
        qm[w, s, 0] = s
    total = int(nqv.sum())
    q_off = np.cumsum(nqv) - nqv
    act = np.nonzero(nqv > 0)[0]
    perm = act[np.argsort(-np.minimum(nqv[act], 256), kind="stable")][::1]
    w, s = np.nonzero(qm[..., 3] >= 0)
    src = np.stack([w, w * nq + s], 1)
    meta = qm[w, s]
    R.check_plan_order(nqv, nw, nq, qm, total, perm, act.shape[0], q_off, total, src, meta)
    # inside a bucket (here: >= 256 queries) the order is free
    big = np.nonzero(np.minimum(nqv, 256)[perm] == 256)[0]
    assert big.shape[0] >= 2
    p2 = perm.copy()
    p2[big[0]], p2[big[-1]] = perm[big[-1]], perm[big[0]]
    R.check_plan_order(nqv, nw, nq, qm, total, p2, act.shape[0], q_off, total, src, meta)
    # a capacity that cuts: the straddling window and all behind it are dropped
    cap = int(q_off[20] + 1)
    R.check_plan_order(nqv, nw, nq, qm, cap, perm, act.shape[0], q_off, int(q_off[20]), src, meta)
    bad = [dict(perm=perm[::-1]), dict(n_act=act.shape[0] - 1), dict(q_off=q_off + 1), dict(n_rows=total - 1),
           dict(src=src[::-1]), dict(meta=meta + 1)]
    for b in bad:
        a = dict(perm=perm, n_act=act.shape[0], q_off=q_off, n_rows=total, src=src, meta=meta)
        a.update(b)
        with pytest.raises(AssertionError):
            R.check_plan_order(nqv, nw, nq, qm, total, a["perm"], a["n_act"], a["q_off"], a["n_rows"], a["src"], a["meta"])
