"""Rotated-box IoU operators and recall bookkeeping, the parts that need no GPU: the public names and signatures of
iou3d_nms_utils / iou3d_nms_compat (the reference's), the argument checks of mssvt_boxes_pairwise / mssvt_nms_normal
(status codes before any HIP call), and CenterPoint.generate_recall_record on CPU tensors with the numpy oracle as IoU."""
import ctypes
import inspect

import numpy as np
import torch

from oracle import nms_ref


def iou3d_oracle(a, b):
    """numpy restatement of boxes_iou3d_gpu (ref iou3d_nms_utils.py:48-81) over the oracle's BEV overlap, float32."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    out = np.zeros((a.shape[0], b.shape[0]), np.float32)
    for i in range(a.shape[0]):
        for j in range(b.shape[0]):
            h = max(min(a[i, 2] + a[i, 5] / 2, b[j, 2] + b[j, 5] / 2) - max(a[i, 2] - a[i, 5] / 2, b[j, 2] - b[j, 5] / 2),
                    np.float32(0))
            ov3 = np.float32(nms_ref.box_overlap(a[i], b[j]) * h)
            va, vb = a[i, 3] * a[i, 4] * a[i, 5], b[j, 3] * b[j, 4] * b[j, 5]
            out[i, j] = ov3 / max(va + vb - ov3, np.float32(1e-6))
    return out


def test_public_names_and_signatures_are_the_references():
    from mssvt_amd import iou3d_nms_compat, iou3d_nms_utils
    for name in ("boxes_iou_bev", "boxes_iou3d_gpu", "boxes_overlap_bev"):
        assert list(inspect.signature(getattr(iou3d_nms_utils, name)).parameters) == ["boxes_a", "boxes_b"], name
    p = inspect.signature(iou3d_nms_utils.nms_normal_gpu).parameters
    assert list(p) == ["boxes", "scores", "thresh", "kwargs"] and p["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    p = inspect.signature(iou3d_nms_utils.nms_gpu).parameters
    assert list(p)[:4] == ["boxes", "scores", "thresh", "pre_maxsize"]
    for name in ("boxes_overlap_bev_gpu", "boxes_iou_bev_gpu", "nms_gpu", "nms_normal_gpu"):  # iou3d_nms_api.cpp:12-15
        assert len(inspect.signature(getattr(iou3d_nms_compat, name)).parameters) == 3, name


def test_argument_errors_of_the_new_entry_points_are_status_codes():
    from mssvt_amd import build
    lib = ctypes.CDLL(build.build())
    null, i, f = ctypes.c_void_p(0), ctypes.c_int, ctypes.c_float
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    pw = lib.mssvt_boxes_pairwise
    assert pw(i(7), i(3), p, i(7), i(3), p, i(7), p, null) == -1       # unknown mode
    assert pw(i(-1), i(3), p, i(7), i(3), p, i(7), p, null) == -1
    assert pw(i(1), i(-1), p, i(7), i(3), p, i(7), p, null) == -1      # negative count
    assert pw(i(1), i(3), p, i(7), i(-1), p, i(7), p, null) == -1
    assert pw(i(1), i(3), p, i(6), i(3), p, i(7), p, null) == -1       # a stride that cannot hold a box
    assert pw(i(1), i(3), p, i(7), i(3), p, i(6), p, null) == -1
    assert pw(i(1), i(3), null, i(7), i(3), p, i(7), p, null) == -1    # null boxes with a non-zero count
    assert pw(i(1), i(3), p, i(7), i(3), null, i(7), p, null) == -1
    assert pw(i(1), i(3), p, i(7), i(3), p, i(7), null, null) == -1
    for mode in range(4):                                              # nothing to do: success without a launch
        assert pw(i(mode), i(0), null, i(7), i(0), null, i(7), null, null) == 0
        assert pw(i(mode), i(0), null, i(7), i(3), p, i(7), null, null) == 0
        assert pw(i(mode), i(3), p, i(7), i(0), null, i(7), null, null) == 0
    nn = lib.mssvt_nms_normal
    assert nn(i(-1), p, f(0.5), p, p, p, null) == -1
    assert nn(i(3), p, f(0.5), p, null, p, null) == -1                 # null keep
    assert nn(i(3), p, f(0.5), p, p, null, null) == -1
    assert lib.mssvt_hip_abi_version() == 100


def test_nms_sparse_keeps_what_the_all_pairs_oracle_keeps():
    """nms_ref.nms_sparse (only pairs whose centres are within reach) against nms_ref.nms (every pair), on the cases of
    tests/test_detector_gpu.py::test_hip_nms_keeps_what_the_oracle_keeps, with and without pre_maxsize."""
    from tests.test_detector_gpu import _random_boxes
    for n, thresh, seed in [(1, 0.5, 0), (70, 0.1, 1), (130, 0.5, 2), (130, 0.7, 3), (193, 0.25, 4)]:
        bx, scores = _random_boxes(n, seed)
        for pre in (None, 40):
            want = nms_ref.nms(bx, scores, thresh, pre)
            got = nms_ref.nms_sparse(bx, scores, thresh, pre)
            assert got.dtype == want.dtype and got.tolist() == want.tolist(), (n, thresh, seed, pre)
        if n > 1:
            assert 1 < len(want) < min(n, 40)  # pre_maxsize = 40: boxes are kept and boxes are removed


def test_nms_normal_oracle_keeps_what_greedy_nms_over_the_iou_normal_matrix_keeps():
    """nms_ref.nms_normal (one row per kept box) against the greedy walk over the whole iou_normal matrix, on the cases
    of tests/test_box_iou_gpu.py::test_nms_normal_keeps_what_greedy_nms_over_iou_normal_keeps."""
    from tests.test_box_iou_gpu import _random_boxes, greedy_nms, iou_normal_np
    for n, thresh, seed in [(1, 0.5, 0), (130, 0.5, 2), (193, 0.25, 4)]:
        bx, scores = _random_boxes(n, seed)
        want = greedy_nms(iou_normal_np(bx, bx), scores, thresh)
        assert nms_ref.nms_normal(bx, scores, thresh).tolist() == want, (n, thresh, seed)
        if n > 1:
            assert 1 < len(want) < n


A = [0, 0, 0, 4, 2, 1.5, 0]


def _moved(x):
    return [x] + A[1:]


def _recall_batch():
    """The hand-derived batch: sample 0 -- predictions [A, A at x = -50], ground truth [A, A at x = +2, A at x = +50] and
    two padding rows: best IoUs 1, 1/3 (overlap 2 x 2 x 1.5 = 6 of a union of 18), 0; sample 1 -- no predictions, two
    ground-truth boxes; sample 2 -- one prediction, ground truth all padding (counts ONE box: row 0 is never trimmed)."""
    gt = np.zeros((3, 5, 8), np.float32)
    gt[0, 0, :7], gt[0, 1, :7], gt[0, 2, :7] = A, _moved(2), _moved(50)
    gt[0, :3, 7] = 1
    gt[1, 0, :7], gt[1, 1, :7] = _moved(10), _moved(20)
    gt[1, :2, 7] = 1
    preds = [np.array([A, _moved(-50)], np.float32), np.zeros((0, 7), np.float32), np.array([A], np.float32)]
    return torch.from_numpy(gt), [torch.from_numpy(p) for p in preds]


def _run(data_dict, preds, seen=None):
    from mssvt_amd.centerpoint import CenterPoint

    def iou_fn(a, b):
        m = iou3d_oracle(a.numpy(), b.numpy())
        assert np.isfinite(m).all()  # a zero-size (padding) box scores IoU 0, not NaN
        if seen is not None:
            seen.append(m)
        return torch.from_numpy(m)

    recall = {}
    for index, p in enumerate(preds):
        recall = CenterPoint.generate_recall_record(box_preds=p, recall_dict=recall, batch_index=index, data_dict=data_dict,
                                                    thresh_list=[0.3, 0.5, 0.7], iou_fn=iou_fn)
    return recall


def test_recall_bookkeeping_hand_derived_batch():
    gt, preds = _recall_batch()
    seen = []
    recall = _run(dict(gt_boxes=gt, batch_size=3), preds, seen)
    assert recall == {"gt": 6, "rcnn_0.3": 2, "rcnn_0.5": 1, "rcnn_0.7": 1, "roi_0.3": 0, "roi_0.5": 0, "roi_0.7": 0}
    assert all(type(v) is int for v in recall.values())
    assert len(seen) == 2  # no IoU call for the sample without predictions
    best = seen[0].max(axis=0)
    assert abs(best[0] - 1) < 1e-6 and abs(best[1] - 1 / 3) < 1e-6 and best[2] == 0 and np.all(best[3:] == 0)
    assert np.all(seen[1] == 0)


def test_recall_bookkeeping_sample_by_sample():
    from mssvt_amd.centerpoint import CenterPoint
    gt, preds = _recall_batch()
    d = dict(gt_boxes=gt)
    fn = lambda a, b: torch.from_numpy(iou3d_oracle(a.numpy(), b.numpy()))  # noqa: E731
    r = CenterPoint.generate_recall_record(preds[0], {}, 0, d, [0.3, 0.5, 0.7], iou_fn=fn)
    assert r == {"gt": 3, "rcnn_0.3": 2, "rcnn_0.5": 1, "rcnn_0.7": 1, "roi_0.3": 0, "roi_0.5": 0, "roi_0.7": 0}
    r = CenterPoint.generate_recall_record(preds[1], r, 1, d, [0.3, 0.5, 0.7], iou_fn=fn)
    assert r["gt"] == 5 and r["rcnn_0.3"] == 2 and r["rcnn_0.7"] == 1  # no predictions: only 'gt' grows
    r = CenterPoint.generate_recall_record(preds[2], r, 2, d, [0.3, 0.5, 0.7], iou_fn=fn)
    assert r["gt"] == 6 and r["rcnn_0.3"] == 2                         # all padding: one box (row 0), not recalled


def test_recall_bookkeeping_without_ground_truth_and_with_rois():
    gt, preds = _recall_batch()
    assert _run(dict(batch_size=3), preds) == {}
    rois = torch.zeros((3, 2, 7))
    rois[0], rois[2, 0] = preds[0], preds[2][0]
    rois[1] = torch.tensor([_moved(-70), _moved(-80)])
    recall = _run(dict(gt_boxes=gt, rois=rois, batch_size=3), preds)
    assert recall["gt"] == 6
    for t in ("0.3", "0.5", "0.7"):
        assert recall["roi_" + t] == recall["rcnn_" + t] > 0


def test_strict_threshold_and_key_spelling():
    """A ground-truth box is recalled at t only when the best IoU EXCEEDS t; the keys carry str() of the yaml's floats."""
    from mssvt_amd.centerpoint import CenterPoint
    gt = torch.zeros((1, 2, 8))
    gt[0, 0, :7] = torch.tensor(A)
    gt[0, 1, :7] = torch.tensor(_moved(9))
    fn = lambda a, b: torch.tensor([[0.5, 0.25]])  # noqa: E731
    r = CenterPoint.generate_recall_record(torch.tensor([A]), {}, 0, dict(gt_boxes=gt), [0.25, 0.5], iou_fn=fn)
    assert r == {"gt": 2, "roi_0.25": 0, "rcnn_0.25": 1, "roi_0.5": 0, "rcnn_0.5": 0}


def test_post_processing_without_ground_truth_returns_an_empty_dict():
    """Pins behaviour that does NOT change with the recall bookkeeping (it passes before it too): no ground truth, no dict."""
    from mssvt_amd.centerpoint import CenterPoint
    final = [dict(pred_boxes=torch.zeros((0, 7)))]
    out = CenterPoint.post_processing(None, dict(final_box_dicts=final, batch_size=1))
    assert out[0] is final and out[1] == {}
