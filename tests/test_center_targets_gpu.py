"""mssvt_center_targets (csrc/center_targets.hip) through ``center_targets`` and ``CenterHead.assign_targets`` against the
host path of ``assign_targets`` on .cpu() copies (the statement of the semantics that tests/test_head_train_cpu.py pins to
the reference run), and against the reference's own targets of tests/golden/det_head_train.npz.

Tolerances: inds / masks and the columns of target_boxes that are basic IEEE operations or copies (0-2, 8...) are equal;
columns 3-7 (log / cos / sin: device vs host library, an ulp apart) atol 1e-6, the bound of test_head_train_cpu.py; heat
maps atol 1.2e-7 = one float ulp below 1.0 (both sides round a double exp to float once)."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the MI355X")]

CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]
YAML_HEADS = [["Vehicle", "Pedestrian", "Cyclist"]]
MULTI = {"ped_first": [["Pedestrian"], ["Vehicle", "Cyclist"]], "cyc_veh": [["Cyclist", "Vehicle"], ["Pedestrian"]]}
KEYS = ("heatmaps", "target_boxes", "inds", "masks")


def make_head(heads=YAML_HEADS, hw=(64, 64), stride=1, voxel=0.32, num_max_objs=500):
    from mssvt_amd.center_head import CenterHead
    H, W = hw
    cfg = dict(CLASS_NAMES_EACH_HEAD=heads, SHARED_CONV_CHANNEL=8, USE_BIAS_BEFORE_NORM=True, NUM_HM_CONV=2,
               SEPARATE_HEAD_CFG=dict(HEAD_ORDER=["center", "center_z", "dim", "rot"],
                                      HEAD_DICT=dict(center=dict(out_channels=2, num_conv=2), center_z=dict(out_channels=1, num_conv=2),
                                                     dim=dict(out_channels=3, num_conv=2), rot=dict(out_channels=2, num_conv=2))),
               TARGET_ASSIGNER_CONFIG=dict(FEATURE_MAP_STRIDE=stride, NUM_MAX_OBJS=num_max_objs, GAUSSIAN_OVERLAP=0.1, MIN_RADIUS=2))
    x, y = W * stride * voxel / 2, H * stride * voxel / 2
    head = CenterHead(cfg, 8, len(CLASSES), CLASSES, np.array([W * stride, H * stride, 32]), np.array([-x, -y, -2.0, x, y, 4.0]),
                      [voxel, voxel, 0.1875], predict_boxes_when_training=False)
    head.hw = hw
    return head


def random_boxes(head, B, N, seed, D=8, outside=0.05):
    """(B, N, D) float32: centres up to `outside` of the range beyond it (clamping, clipped patches), sizes from below a
    cell to several cells, labels 0..3 (0 = padding, anywhere in the list)."""
    rng = np.random.default_rng(seed)
    x, y = float(head.point_cloud_range[3]), float(head.point_cloud_range[4])
    gt = np.zeros((B, N, D), np.float32)
    gt[..., 0] = rng.uniform(-x * (1 + outside), x * (1 + outside), (B, N))
    gt[..., 1] = rng.uniform(-y * (1 + outside), y * (1 + outside), (B, N))
    gt[..., 2] = rng.uniform(-1.5, 3.0, (B, N))
    gt[..., 3] = rng.uniform(0.2, 6.0, (B, N))
    gt[..., 4] = rng.uniform(0.2, 3.0, (B, N))
    gt[..., 5] = rng.uniform(0.5, 2.5, (B, N))
    gt[..., 6] = rng.uniform(-np.pi, np.pi, (B, N))
    if D > 8:
        gt[..., 7:D - 1] = rng.normal(0, 3, (B, N, D - 8))
    gt[..., D - 1] = rng.integers(0, len(CLASSES) + 1, (B, N))
    return gt


def host_targets(head, gt):
    """the oracle: the host path of assign_targets on CPU boxes"""
    return head.assign_targets(torch.as_tensor(gt).cpu(), feature_map_size=head.hw)


def device_targets(head, gt_dev):
    """the operator, one call per head, without the wiring of assign_targets"""
    from mssvt_amd.center_head import center_targets
    tcfg = head.model_cfg["TARGET_ASSIGNER_CONFIG"]
    tables = torch.from_numpy(np.ascontiguousarray(head.label_tables().T)).to(gt_dev.device)
    out = {k: [] for k in KEYS}
    for h, names in enumerate(head.class_names_each_head):
        res = center_targets(gt_dev, tables[h], len(names), head.hw, head.point_cloud_range, head.voxel_size,
                             tcfg["FEATURE_MAP_STRIDE"], tcfg["NUM_MAX_OBJS"], tcfg["GAUSSIAN_OVERLAP"], tcfg["MIN_RADIUS"])
        for k, t in zip(KEYS, res):
            out[k].append(t)
    return out


def check(got, want, what=""):
    assert len(got["heatmaps"]) == len(want["heatmaps"])
    for h in range(len(want["heatmaps"])):
        g = {k: got[k][h].cpu().numpy() for k in KEYS}
        w = {k: np.asarray(want[k][h]) for k in KEYS}
        for k in KEYS:
            assert g[k].shape == w[k].shape, (what, k, g[k].shape, w[k].shape)
        np.testing.assert_array_equal(g["inds"], w["inds"], err_msg="%s inds head %d" % (what, h))
        np.testing.assert_array_equal(g["masks"], w["masks"], err_msg="%s masks head %d" % (what, h))
        tb, wb = g["target_boxes"], w["target_boxes"]
        np.testing.assert_array_equal(tb[..., 0:3], wb[..., 0:3], err_msg="%s target_boxes[0:3] head %d" % (what, h))
        np.testing.assert_array_equal(tb[..., 8:], wb[..., 8:], err_msg="%s target_boxes[8:] head %d" % (what, h))
        np.testing.assert_allclose(tb[..., 3:8], wb[..., 3:8], rtol=0, atol=1e-6, err_msg="%s target_boxes[3:8] head %d" % (what, h))
        np.testing.assert_allclose(g["heatmaps"], w["heatmaps"], rtol=0, atol=1.2e-7, err_msg="%s heatmaps head %d" % (what, h))
        assert g["heatmaps"].dtype == np.float32 and g["inds"].dtype == np.int64 and g["masks"].dtype == np.int64
        if g["masks"].any():
            assert float(g["heatmaps"].max()) == 1.0, (what, h)
        else:
            assert float(g["heatmaps"].max()) == 0.0, (what, h)


def run_case(head, gt, what=""):
    want = host_targets(head, gt)
    got = device_targets(head, torch.from_numpy(gt).cuda())
    check(got, {k: [t.numpy() for t in want[k]] for k in KEYS}, what)
    return got, want


def test_golden_targets_of_the_reference_run(golden_dir):
    from mssvt_amd.center_head import CenterHead, center_targets
    d = np.load(os.path.join(golden_dir, "det_head_train.npz"))
    cfg = json.loads(str(d["cfg_json"]))
    head = CenterHead(cfg["HEAD"], cfg["input_channels"], len(cfg["CLASSES"]), cfg["CLASSES"], np.array(cfg["GRID"]),
                      np.array(cfg["PCR"]), cfg["VOXEL"], predict_boxes_when_training=False)
    tcfg = cfg["HEAD"]["TARGET_ASSIGNER_CONFIG"]
    table = torch.from_numpy(np.ascontiguousarray(head.label_tables().T)).cuda()
    H, W = d["target0.heatmaps"].shape[2:]
    res = center_targets(torch.from_numpy(d["gt_boxes"]).cuda(), table[0], len(head.class_names_each_head[0]), (H, W),
                         head.point_cloud_range, head.voxel_size, tcfg["FEATURE_MAP_STRIDE"], tcfg["NUM_MAX_OBJS"],
                         tcfg["GAUSSIAN_OVERLAP"], tcfg["MIN_RADIUS"])
    for k, t in zip(KEYS, res):
        got = t.cpu().numpy()
        if k in ("inds", "masks"):
            np.testing.assert_array_equal(got, d["target0." + k], err_msg=k)
        else:
            np.testing.assert_allclose(got, d["target0." + k], rtol=0, atol=1e-6, err_msg=k)
    assert int(res[3].sum()) == 25 and float(res[0].max()) == 1.0


@pytest.mark.parametrize("hw,stride,voxel", [((33, 47), 2, 0.4), ((40, 52), 1, 0.32), ((8, 8), 1, 0.32)])
def test_map_shapes_that_do_not_divide_into_tiles(hw, stride, voxel):
    """W = 47: scalar stores; W = 52: 16-byte stores with a clipped last tile; 8 x 8: smaller than most patches."""
    head = make_head(hw=hw, stride=stride, voxel=voxel)
    run_case(head, random_boxes(head, 2, 24, seed=hw[0]), str(hw))


def _box(cx, cy, dx_cells, dy_cells, label, voxel=0.32, half=48, z=0.5):
    """a box whose centre lands on map coordinate (cx, cy) of a 96 x 96 map and whose extent is given in cells"""
    return [cx * voxel - half * voxel, cy * voxel - half * voxel, z, dx_cells * voxel, dy_cells * voxel, 1.6, 0.3, label]


def test_patches_across_tiles_and_on_top_of_each_other():
    head = make_head(hw=(96, 96))
    rows = [
        _box(32.0, 32.0, 6, 6, 1),     # centred on the corner that four tiles share
        _box(48.5, 48.5, 45, 45, 2),   # radius 19: the patch is 39 cells wide and spans three tiles each way
        _box(70.5, 20.5, 12, 12, 1),   # two objects of one class with overlapping patches
        _box(73.5, 22.5, 12, 12, 1),
        _box(10.5, 80.5, 5, 5, 3),     # two of one class in one cell, different sizes
        _box(10.7, 80.2, 14, 14, 3),
        _box(60.5, 80.5, 8, 8, 1),     # two classes in one cell
        _box(60.5, 80.5, 8, 8, 2),
    ]
    gt = np.array([rows], np.float32)
    got, _ = run_case(head, gt, "tiles")
    hm = got["heatmaps"][0][0].cpu().numpy()
    assert np.count_nonzero(hm[1, 48, :]) == 39 and np.count_nonzero(hm[1, :, 48]) == 39  # the three-tile patch is whole
    assert hm[0, 32, 32] == 1.0 and hm[0, 31, 31] > 0 and hm[0, 33, 31] > 0 and hm[0, 31, 33] > 0 and hm[0, 33, 33] > 0
    assert hm[0, 80, 60] == 1.0 and hm[1, 80, 60] == 1.0 and hm[2, 80, 60] == 0.0


def test_more_selected_rows_than_slots_and_padding_in_the_middle():
    head = make_head(hw=(40, 52), num_max_objs=7)
    gt = random_boxes(head, 2, 24, seed=11)
    gt[0, 2:5, 7] = 0  # padding rows between objects
    assert ((gt[..., 7] > 0).sum(axis=1) > 7).all()
    got, _ = run_case(head, gt, "M = 7")
    assert got["masks"][0].shape == (2, 7)


def test_zero_extent_box_keeps_its_slot_with_a_zero_row():
    head = make_head(hw=(40, 52))
    gt = random_boxes(head, 1, 12, seed=3)
    gt[0, :, 7] = np.maximum(gt[0, :, 7], 1)
    gt[0, 4, 3] = 0.0
    got, _ = run_case(head, gt, "zero extent")
    assert int(got["masks"][0][0, 4]) == 0 and float(got["target_boxes"][0][0, 4].abs().sum()) == 0.0
    assert int(got["masks"][0][0, 5]) == 1 and int(got["masks"][0][0].sum()) == 11


@pytest.mark.parametrize("N", [300, 600])
def test_row_counts_across_the_chunk_and_beyond_the_slots(N):
    """300 rows cross the 256-row chunk; 600 rows leave more selected rows than M = 500 (three chunks)."""
    head = make_head(hw=(40, 52))
    gt = random_boxes(head, 2, N, seed=N)
    if N == 600:
        gt[..., 7] = np.maximum(gt[..., 7], 1)
        gt[0, 100:140, 7] = 0  # 560 selected rows in sample 0, 600 in sample 1
    got, _ = run_case(head, gt, "N = %d" % N)
    if N == 600:
        assert int(got["masks"][0].sum()) == 1000


def test_no_boxes_and_a_single_sample():
    head = make_head(hw=(33, 47))
    got, _ = run_case(head, np.zeros((2, 0, 8), np.float32), "N = 0")
    assert float(got["heatmaps"][0].abs().sum()) == 0.0 and int(got["masks"][0].sum()) == 0
    run_case(head, random_boxes(head, 1, 24, seed=21), "B = 1")


def test_velocity_columns_are_copied():
    head = make_head(hw=(40, 52))
    gt = random_boxes(head, 2, 24, seed=8, D=10)
    got, _ = run_case(head, gt, "D = 10")
    assert got["target_boxes"][0].shape == (2, 500, 10)
    assert float(got["target_boxes"][0][..., 8:].abs().sum()) > 0


@pytest.mark.parametrize("layout", sorted(MULTI))
def test_multi_head_relabelling(layout):
    head = make_head(heads=MULTI[layout], hw=(40, 52))
    run_case(head, random_boxes(head, 2, 40, seed=13), layout)


def test_non_contiguous_and_float64_boxes():
    """Both are brought to contiguous float32 on the device; the oracle runs on the float32 values."""
    head = make_head(hw=(40, 52))
    wide = random_boxes(head, 2, 48, seed=17, D=10)
    wide[..., 7] = wide[..., 9]
    view = torch.from_numpy(wide).cuda()[:, ::2, :8]
    assert not view.is_contiguous()
    gt = np.ascontiguousarray(wide[:, ::2, :8])
    want = host_targets(head, gt)
    want = {k: [t.numpy() for t in want[k]] for k in KEYS}
    check(device_targets(head, view), want, "view")
    check(device_targets(head, torch.from_numpy(gt).double().cuda()), want, "float64")


def test_nan_rows_and_unknown_labels_get_no_target():
    """A documented difference: the host path raises on a NaN label or a label beyond the class list.  On the device a
    row with a non-finite value keeps its slot without a target (as a zero-extent box does), a NaN or unknown label takes
    no slot (as padding does), and every other row is unchanged."""
    head = make_head(hw=(40, 52))
    gt = random_boxes(head, 2, 24, seed=29)
    gt[..., 7] = np.maximum(gt[..., 7], 1)
    bad, clean = gt.copy(), gt.copy()
    bad[0, 3, 0] = np.nan
    clean[0, 3, 3] = 0.0
    bad[0, 9, 6] = np.inf
    clean[0, 9, 3] = 0.0
    bad[1, 5, 7] = np.nan
    clean[1, 5, 7] = 0
    bad[0, 12, 7] = 99
    clean[0, 12, 7] = 0
    bad[1, 7, 7] = -3
    clean[1, 7, 7] = 0
    want = host_targets(head, clean)
    got = device_targets(head, torch.from_numpy(bad).cuda())
    check(got, {k: [t.numpy() for t in want[k]] for k in KEYS}, "bad rows")
    assert bool(torch.isfinite(got["target_boxes"][0]).all()) and int(got["masks"][0].sum()) == 2 * 24 - 5


def test_assign_targets_uses_the_operator_and_reads_nothing_back(monkeypatch):
    head = make_head(heads=MULTI["ped_first"], hw=(40, 52))
    gt = random_boxes(head, 2, 40, seed=31)
    gt_dev = torch.from_numpy(gt).cuda()
    keep = gt_dev.clone()
    want = device_targets(head, gt_dev)
    torch.cuda.synchronize()

    def refuse(*args, **kwargs):
        raise AssertionError("the device path of assign_targets read something back")

    with monkeypatch.context() as m:
        for name in ("cpu", "item", "tolist", "numpy", "nonzero"):
            m.setattr(torch.Tensor, name, refuse)
        first = head.assign_targets(gt_dev, feature_map_size=head.hw)
        second = head.assign_targets(gt_dev, feature_map_size=head.hw)
    assert torch.equal(gt_dev, keep)  # the caller's boxes are not re-labelled
    assert sorted(first) == ["heatmap_masks", "heatmaps", "inds", "masks", "target_boxes"]
    for k in KEYS:
        assert len(first[k]) == 2
        for h in range(2):
            assert first[k][h].is_cuda and first[k][h].dtype == want[k][h].dtype
            assert torch.equal(first[k][h], want[k][h]), (k, h)
            assert torch.equal(first[k][h], second[k][h]), (k, h)
    host = host_targets(head, gt)
    for k in KEYS:
        for h in range(2):
            assert first[k][h].dtype == host[k][h].dtype and first[k][h].shape == host[k][h].shape, (k, h)


def test_the_yaml_shape():
    """mssvt.yaml's own call: B = 4, 3 classes, 470 x 470, M = 500, 200 objects per sample."""
    head = make_head(hw=(470, 470))
    gt = random_boxes(head, 4, 200, seed=41)
    gt[..., 7] = np.maximum(gt[..., 7], 1)
    run_case(head, gt, "yaml")
