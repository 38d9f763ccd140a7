"""Stand-in for the reference's pybind module ``iou3d_nms_cuda`` -- its four GPU functions (ref:
pcdet/ops/iou3d_nms/src/iou3d_nms_api.cpp:12-15; bodies iou3d_nms.cpp:49-188), on ``libmssvt_hip.so``
(include/mssvt_hip.h, the post-processing block):

    # pcdet/ops/iou3d_nms/iou3d_nms_utils.py:9
    from mssvt_amd import iou3d_nms_compat as iou3d_nms_cuda

Same names, argument order and in-place conventions: the (N, M) answer is allocated by the caller and filled here, ``keep``
is a host int64 tensor that receives the kept positions and the count is returned.  With it the reference's own
``iou3d_nms_utils.py`` runs unchanged; ``mssvt_amd.iou3d_nms_utils`` is the direct route (no host round trip of ``keep``).
``boxes_iou_bev_cpu`` (the GT-database sampler's; datasets are out of scope) has no stand-in.
"""
import torch

from . import _lib, iou3d_nms_utils


def _answer(ans, boxes_a, boxes_b):
    if ans.dtype != torch.float32 or tuple(ans.shape) != (boxes_a.shape[0], boxes_b.shape[0]):
        raise _lib.MssvtHipError("the answer tensor must be float32 of shape (N, M)")
    return ans


def boxes_overlap_bev_gpu(boxes_a, boxes_b, ans_overlap):
    iou3d_nms_utils.boxes_pairwise(iou3d_nms_utils.BOX_OVERLAP_BEV, boxes_a, boxes_b, out=_answer(ans_overlap, boxes_a, boxes_b))
    return 1


def boxes_iou_bev_gpu(boxes_a, boxes_b, ans_iou):
    iou3d_nms_utils.boxes_pairwise(iou3d_nms_utils.BOX_IOU_BEV, boxes_a, boxes_b, out=_answer(ans_iou, boxes_a, boxes_b))
    return 1


def _nms(boxes, keep, thresh, entry, who):
    """boxes (N, 7) in descending score order; keep (>= N) int64 on the host <- kept positions; returns their number."""
    if keep.is_cuda or keep.dtype != torch.int64 or not keep.is_contiguous():
        raise _lib.MssvtHipError("%s: keep must be a contiguous int64 tensor on the host" % who)
    order = torch.arange(boxes.shape[0], device=boxes.device)
    kept = iou3d_nms_utils._nms_ordered(boxes, order, float(thresh), entry, who)
    keep[:kept.numel()] = kept.cpu()
    return int(kept.numel())


def nms_gpu(boxes, keep, thresh):
    return _nms(boxes, keep, thresh, "mssvt_nms_bev", "nms_gpu")


def nms_normal_gpu(boxes, keep, thresh):
    return _nms(boxes, keep, thresh, "mssvt_nms_normal", "nms_normal_gpu")

