"""Rotated-box IoU operators and NMS on MI355X -- the GPU functions of the reference's
``pcdet.ops.iou3d_nms.iou3d_nms_utils`` (:31-116), same names, parameter names, asserts and return values:

* ``nms_gpu`` / ``nms_normal_gpu`` -- what ``model_nms_utils.class_agnostic_nms`` resolves by name
  (``getattr(iou3d_nms_utils, nms_config.NMS_TYPE)``, ref: pcdet/models/model_utils/model_nms_utils.py:27-30).  The
  suppression matrix AND the greedy walk run on the device (csrc/nms_bev.hip), one host sync for the number of boxes kept.
* ``boxes_iou_bev`` / ``boxes_iou3d_gpu`` (and ``boxes_overlap_bev``, the matrix the reference's pybind module fills for
  the 3-D IoU) -- (N, M) pair matrices from one launch of csrc/box_iou.hip; the 3-D IoU's height / volume arithmetic is
  fused into it and rounds like the reference's torch composition.  Column slices of wider tensors (``preds[:, 0:7]``)
  are read in place through the row stride.

``boxes_bev_iou_cpu`` (the GT-database sampler's, datasets are out of scope) is not provided."""
import torch

from . import _lib


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """boxes (N, 7) [x, y, z, dx, dy, dz, heading], scores (N) -> (indices of the kept boxes, best first; None)."""
    assert boxes.shape[1] == 7
    order = scores.sort(0, descending=True)[1]
    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    return _nms_ordered(boxes, order, thresh, "mssvt_nms_bev", "nms_gpu"), None


def nms_normal_gpu(boxes, scores, thresh, **kwargs):
    """As `nms_gpu` with the axis-aligned BEV IoU (heading ignored): (indices of the kept boxes, best first; None)."""
    assert boxes.shape[1] == 7
    order = scores.sort(0, descending=True)[1]
    return _nms_ordered(boxes, order, thresh, "mssvt_nms_normal", "nms_normal_gpu"), None


def _nms_ordered(boxes, order, thresh, entry, who):
    """The indices of `order` (into `boxes`, descending score) that greedy NMS through `entry` keeps."""
    n = int(order.shape[0])
    if n == 0:
        return order
    if n > NMS_MAX_BOXES:
        # beyond one launch's capacity (the reference takes any N): score-ordered chunks, the boxes kept so far put in
        # front of the next chunk -- they outrank it and do not suppress each other, so greedy NMS keeps them and
        # applies them to the chunk: the same result as one pass
        kept = order[:0]
        for lo in range(0, n, NMS_MAX_BOXES // 2):
            chunk = order[lo:lo + NMS_MAX_BOXES // 2]
            if kept.numel() + chunk.numel() > NMS_MAX_BOXES:
                raise _lib.MssvtHipError("%s: more than %d boxes survive" % (who, NMS_MAX_BOXES // 2))
            cand = torch.cat([kept, chunk])
            kept = cand[_nms_sorted(boxes[cand].float().contiguous(), thresh, entry)]
        return kept.contiguous()
    b = boxes[order].float().contiguous()
    return order[_nms_sorted(b, thresh, entry)].contiguous()


NMS_MAX_BOXES = 16384  # csrc/nms_bev.hip: one launch

BOX_OVERLAP_BEV, BOX_IOU_BEV, BOX_IOU_3D, BOX_IOU_NORMAL = 0, 1, 2, 3  # include/mssvt_hip.h MSSVT_BOX_*


def _rows(t):
    """(tensor whose rows the kernel can read in place, row stride in floats): fp32 on the GPU with unit column stride
    -- a contiguous tensor or a column slice of a wider one -- goes as it is, anything else through a contiguous copy."""
    if not t.is_cuda:
        raise _lib.MssvtHipError("mssvt_amd ops need tensors on the GPU (no CPU path)")
    if t.dtype != torch.float32 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < 7):
        t = t.float().contiguous()
    return t, (int(t.stride(0)) if t.shape[0] > 1 else 7)


def boxes_pairwise(mode, boxes_a, boxes_b, out=None):
    """out[i, j] = measure `mode` (BOX_*) of boxes_a[i] and boxes_b[j]; (N, 7+) and (M, 7+) rows -> (N, M) float32."""
    assert boxes_a.dim() == 2 and boxes_b.dim() == 2 and boxes_a.shape[1] >= 7 and boxes_b.shape[1] >= 7
    a, sa = _rows(boxes_a)
    b, sb = _rows(boxes_b)
    n, m = int(a.shape[0]), int(b.shape[0])
    if out is None:
        out = torch.empty((n, m), dtype=torch.float32, device=a.device)  # fully written by the kernel
    if not (a.device == b.device == out.device) or out.dtype != torch.float32 or tuple(out.shape) != (n, m):
        raise _lib.MssvtHipError("boxes_pairwise: boxes_a, boxes_b and a float32 (N, M) out must share one device")
    if n and m:
        _lib.call("mssvt_boxes_pairwise", mode, n, a.data_ptr(), sa, m,
                  b.data_ptr(), sb, _lib.ptr(out), _lib.stream())
    return out


def boxes_overlap_bev(boxes_a, boxes_b):
    """boxes_a (N, 7), boxes_b (M, 7) [x, y, z, dx, dy, dz, heading] -> (N, M) overlap areas in the bird's-eye view."""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return boxes_pairwise(BOX_OVERLAP_BEV, boxes_a, boxes_b)


def boxes_iou_bev(boxes_a, boxes_b):
    """boxes_a (N, 7), boxes_b (M, 7) [x, y, z, dx, dy, dz, heading] -> ans_iou (N, M), rotated BEV IoU."""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return boxes_pairwise(BOX_IOU_BEV, boxes_a, boxes_b)


def boxes_iou3d_gpu(boxes_a, boxes_b):
    """boxes_a (N, 7), boxes_b (M, 7) [x, y, z, dx, dy, dz, heading] -> ans_iou (N, M), 3-D IoU (BEV overlap x height
    overlap over the union of the volumes)."""
    assert boxes_a.shape[1] == boxes_b.shape[1] == 7
    return boxes_pairwise(BOX_IOU_3D, boxes_a, boxes_b)


def padded_outputs(batch_size, rows, row_floats, device):
    """The zeroed padded outputs that ``nms_padded`` appends into: pred_boxes (B, rows, row_floats) f32, pred_scores
    (B, rows) f32, pred_labels (B, rows) i64, num (B) i32."""
    return dict(pred_boxes=torch.zeros((batch_size, rows, row_floats), dtype=torch.float32, device=device),
                pred_scores=torch.zeros((batch_size, rows), dtype=torch.float32, device=device),
                pred_labels=torch.zeros((batch_size, rows), dtype=torch.int64, device=device),
                num=torch.zeros((batch_size,), dtype=torch.int32, device=device))


def nms_padded(cand_boxes, cand_scores, cand_labels, cand_num, class_map, thresh, pre_maxsize, post_maxsize, normal=False,
               out=None):
    """Greedy NMS of a batch of padded candidate lists (the outputs of ``center_head.center_decode``: rows in descending
    score order, cand_num (B) i32 of them valid) with the counts on the device: two launches, no host synchronisation
    (csrc/nms_bev_batched.hip).  Per sample the first min(cand_num, pre_maxsize) rows meet; the first post_maxsize kept rows
    are APPENDED to `out` (``padded_outputs``; made with post_maxsize rows when None) behind its ``num`` rows, labels as
    class_map[label] + 1 (class_map (C) i64 on the device); `normal`: the axis-aligned IoU of ``nms_normal_gpu``.
    Returns `out`."""
    if not (cand_boxes.is_cuda and cand_boxes.dim() == 3 and cand_boxes.shape[2] >= 7):
        raise _lib.MssvtHipError("nms_padded needs (B, K, 7+) candidate boxes on the GPU (no CPU path)")
    B, K, D = (int(v) for v in cand_boxes.shape)
    dev = cand_boxes.device
    if out is None:
        out = padded_outputs(B, int(post_maxsize), D, dev)
    P = int(out["pred_boxes"].shape[1])
    ok = (cand_boxes.dtype == torch.float32 and cand_scores.dtype == torch.float32 and cand_labels.dtype == torch.int32 and
          cand_num.dtype == torch.int32 and class_map.dtype == torch.int64 and tuple(cand_scores.shape) == (B, K) and
          tuple(cand_labels.shape) == (B, K) and tuple(cand_num.shape) == (B,) and class_map.dim() == 1 and
          tuple(out["pred_boxes"].shape) == (B, P, D) and out["pred_boxes"].dtype == torch.float32 and
          tuple(out["pred_scores"].shape) == (B, P) and out["pred_scores"].dtype == torch.float32 and
          tuple(out["pred_labels"].shape) == (B, P) and out["pred_labels"].dtype == torch.int64 and
          tuple(out["num"].shape) == (B,) and out["num"].dtype == torch.int32 and
          all(t.device == dev for t in (cand_scores, cand_labels, cand_num, class_map, *out.values())))
    if not ok:
        raise _lib.MssvtHipError("nms_padded: candidates f32 (B, K, D) / f32 (B, K) / i32 (B, K) / i32 (B), class_map i64 (C) "
                                 "and outputs f32 (B, P, D) / f32 (B, P) / i64 (B, P) / i32 (B) must share one device")
    if B == 0 or K == 0:
        return out
    nbytes = int(_lib.lib().mssvt_nms_bev_batched_workspace_bytes(B, K, int(pre_maxsize)))
    if nbytes <= 0:
        raise _lib.MssvtHipError("nms_padded: beyond the kernel's limits (B <= 65535, K <= 4096, pre_maxsize >= 1): "
                                 "B=%d K=%d pre_maxsize=%d" % (B, K, int(pre_maxsize)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.call("mssvt_nms_bev_batched", B, K, D, _lib.ptr(cand_boxes), _lib.ptr(cand_scores), _lib.ptr(cand_labels),
              _lib.ptr(cand_num), _lib.ptr(class_map), int(class_map.numel()), int(pre_maxsize), int(post_maxsize),
              float(thresh), 1 if normal else 0, _lib.ptr(ws), P, _lib.ptr(out["pred_boxes"]), _lib.ptr(out["pred_scores"]),
              _lib.ptr(out["pred_labels"]), _lib.ptr(out["num"]), _lib.stream())
    return out


def _nms_sorted(b, thresh, entry="mssvt_nms_bev"):
    """Indices (into `b`, best first) that greedy NMS keeps among boxes already sorted by descending score."""
    n = int(b.shape[0])
    ws = torch.empty(int(_lib.lib().mssvt_nms_workspace_bytes(n)) // 8 + 1, dtype=torch.int64, device=b.device)
    keep = torch.empty(n, dtype=torch.int32, device=b.device)
    cnt = torch.empty(1, dtype=torch.int32, device=b.device)
    _lib.call(entry, n, _lib.ptr(b), float(thresh), _lib.ptr(ws), _lib.ptr(keep),
              _lib.ptr(cnt), _lib.stream())
    return keep[:int(cnt.item())].long()
