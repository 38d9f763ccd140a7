"""The numpy statement of CenterHead's padded inference path (tests/center_decode_ref.py) against what is already pinned:
the reference-run golden (tests/golden/det_bev_head.npz) and ``CenterHead.generate_predicted_boxes`` on the CPU with the
oracle NMS; and the CPU-visible part of the padded path's interface (it has no CPU path)."""
import json
import os

import numpy as np
import pytest
import torch

from mssvt_amd import _lib
from mssvt_amd.center_head import CenterHead
from mssvt_amd.config import Config
from tests import center_decode_ref as ref
from tests.test_detector_cpu import _oracle_nms


def golden_cfg(golden_dir):
    d = np.load(os.path.join(golden_dir, "det_bev_head.npz"))
    return d, json.loads(str(d["cfg_json"]))


def make_head(cfg, head_cfg=None, classes=None):
    classes = classes or cfg["CLASSES"]
    return CenterHead(Config.wrap(head_cfg or cfg["HEAD"]), 8, len(classes), classes, np.array(cfg["GRID"]),
                      np.array(cfg["PCR"]), cfg["VOXEL"], predict_boxes_when_training=False).eval()


def ref_from_cfg(heads, head):
    post = head.model_cfg["POST_PROCESSING"]
    nms = post["NMS_CONFIG"]
    return ref.head_major(heads, [m.numpy() for m in head._class_maps], post["MAX_OBJ_PER_SAMPLE"], head.feature_map_stride,
                          head.voxel_size, head.point_cloud_range, post["POST_CENTER_LIMIT_RANGE"], post["SCORE_THRESH"],
                          nms["NMS_THRESH"], nms["NMS_PRE_MAXSIZE"], nms["NMS_POST_MAXSIZE"],
                          normal=nms["NMS_TYPE"] == "nms_normal_gpu")


def test_helper_reproduces_the_reference_run(golden_dir):
    d, cfg = golden_cfg(golden_dir)
    head = make_head(cfg)
    raw = {k: d["raw." + k] for k in ("hm", "center", "center_z", "dim", "rot")}
    got = ref_from_cfg([raw], head)
    for b in range(int(d["batch_size"])):
        want_boxes, want_scores = d["final%d.pred_boxes" % b], d["final%d.pred_scores" % b]
        g = got[b]
        assert g["pred_boxes"].shape == want_boxes.shape
        np.testing.assert_allclose(g["pred_scores"], want_scores, rtol=1e-4, atol=2e-5)
        rows = lambda bx, lb: np.concatenate([bx, lb[:, None].astype(np.float32)], 1)  # noqa: E731
        gr, wr = rows(g["pred_boxes"], g["pred_labels"]), rows(want_boxes, d["final%d.pred_labels" % b])
        gr, wr = gr[np.lexsort((gr[:, 1], gr[:, 0]))], wr[np.lexsort((wr[:, 1], wr[:, 0]))]
        np.testing.assert_allclose(gr, wr, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("names_each_head,V,nms_type", [([["Vehicle", "Pedestrian", "Cyclist"]], 0, "nms_gpu"),
                                                        ([["Pedestrian"], ["Vehicle", "Cyclist"]], 2, "nms_normal_gpu")])
def test_helper_equals_the_list_path_on_distinct_logits(golden_dir, names_each_head, V, nms_type):
    _, cfg = golden_cfg(golden_dir)
    hc = json.loads(json.dumps(cfg["HEAD"]))
    hc["CLASS_NAMES_EACH_HEAD"] = names_each_head
    hc["POST_PROCESSING"].update(MAX_OBJ_PER_SAMPLE=60, SCORE_THRESH=0.3,
                                 POST_CENTER_LIMIT_RANGE=[-17.0, -18.0, -0.8, -8.0, -12.5, 0.9])
    hc["POST_PROCESSING"]["NMS_CONFIG"].update(NMS_TYPE=nms_type, NMS_THRESH=0.2, NMS_PRE_MAXSIZE=40, NMS_POST_MAXSIZE=15)
    if V:
        hc["SEPARATE_HEAD_CFG"]["HEAD_ORDER"].append("vel")
        hc["SEPARATE_HEAD_CFG"]["HEAD_DICT"]["vel"] = dict(out_channels=V, num_conv=2)
    head = make_head(cfg, hc)
    if nms_type == "nms_gpu":
        head.nms_fn = _oracle_nms
    else:
        from oracle import nms_ref
        head.nms_fn = lambda boxes, scores, thresh, **kw: (torch.from_numpy(np.asarray(
            nms_ref.nms_normal(boxes.numpy(), scores.numpy(), float(thresh)), dtype=np.int64)), None)
    B, H, W = 2, 13, 21
    heads = ref.random_heads(np.random.default_rng(5), B, [len(n) for n in names_each_head], H, W, V)
    want = head.generate_predicted_boxes(B, [{k: torch.from_numpy(v) for k, v in pd.items()} for pd in heads])
    got = ref_from_cfg(heads, head)
    for b in range(B):
        assert got[b]["margin"] > 1e-4  # no score / centre on a filter bound
        assert 0 < got[b]["pred_boxes"].shape[0] <= 15 * len(names_each_head)
        ref.assert_rows_close(got[b]["pred_boxes"], got[b]["pred_scores"], want[b]["pred_boxes"].numpy(),
                              want[b]["pred_scores"].numpy())
        np.testing.assert_array_equal(got[b]["pred_labels"], want[b]["pred_labels"].numpy())


def test_selection_rule_of_the_helper():
    hm = np.array([0.5, -0.0, 0.5, np.nan, 0.0, 1.0, -np.inf, 0.5], np.float32).reshape(2, 2, 2)
    order, nans = ref.select(hm, 100)
    assert order.tolist() == [5, 0, 2, 7, 1, 4, 6, 3] and nans == 1
    assert ref.select(hm, 3)[0].tolist() == [5, 0, 2]
    assert ref.select(np.full((1, 3, 4), -2.19, np.float32), 5)[0].tolist() == [0, 1, 2, 3, 4]


def test_padded_path_has_no_cpu_path_and_is_opt_in(golden_dir):
    d, cfg = golden_cfg(golden_dir)
    head = make_head(cfg)
    assert head.padded_predictions is False
    raw = {k: torch.from_numpy(d["raw." + k]) for k in ("hm", "center", "center_z", "dim", "rot")}
    with pytest.raises(_lib.MssvtHipError):
        head.generate_predicted_boxes_padded(int(d["batch_size"]), [raw])


def test_center_decode_refuses_cpu_tensors():
    from mssvt_amd import center_head
    z = torch.zeros(1, 1, 2, 2)
    with pytest.raises(_lib.MssvtHipError):
        center_head.center_decode(z, z.repeat(1, 2, 1, 1), z, z.repeat(1, 3, 1, 1), z.repeat(1, 2, 1, 1),
                                  point_cloud_range=[0, 0, 0], voxel_size=[1, 1, 1], feature_map_stride=1, K=1,
                                  post_center_limit_range=[-1, -1, -1, 1, 1, 1])


def test_the_4096_box_nms_set_sits_on_no_threshold():
    """tests/test_center_decode_gpu.py sets a few boxes of its 4096-box set apart (NMS_SET_APART) so that no pair's oracle
    IoU lies within 1e-4 of 0.1 or 0.7, rotated or axis-aligned: checked here, pair by pair, on the CPU."""
    from tests import test_center_decode_gpu as g
    full = g.nms_sample(g.K_LIMIT)[0]
    assert full.shape == (4096, 9)
    assert g.near_pair_iou_margin(full, False, (0.1, 0.7)) > 1e-4
    assert g.near_pair_iou_margin(full, True, (0.1, 0.7)) > 1e-4


def test_the_sparse_walk_is_the_plain_walk_on_the_500_box_set():
    """the GPU tests hold the batched NMS to nms_ref.nms_sparse; on their 500-box set that walk keeps what nms_ref.nms,
    which evaluates every pair, keeps"""
    from oracle import nms_ref
    from tests import test_center_decode_gpu as g
    full = g.nms_sample(500)[0]
    rank = np.arange(500, 0, -1).astype(np.float64)
    for thresh in (0.1, 0.7):
        assert nms_ref.nms_sparse(full[:, :7], rank, thresh).tolist() == nms_ref.nms(full[:, :7], rank, thresh).tolist()
