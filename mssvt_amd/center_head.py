"""``CenterHead`` -- the dense head of the CenterPoint detector that mssvt.yaml configures.

Drop-in for the reference's pcdet/models/dense_heads/center_head.py: ``SeparateHead`` (:11-46) and ``CenterHead``
(:49-103, forward :350-381, ``generate_predicted_boxes`` :252-331) with the same constructor arguments, config keys
and **state-dict keys** (``shared_conv.{0,1}.*``, ``heads_list.{i}.{hm,center,center_z,dim,rot[,vel]}.{k}...``), so a
reference checkpoint loads by key.  Decoding follows centernet_utils.decode_bbox_from_heatmap (:154-216): top-K peaks of
the sigmoid heat map, sub-cell centre offsets, exp() sizes, atan2 heading, centre-range and score filters; then the
class-agnostic rotated NMS of model_nms_utils.class_agnostic_nms (:6-38) on the device (mssvt_amd/iou3d_nms_utils.py).
Training (``.train()``): ``assign_targets`` (:103-214: Gaussian heat maps with CornerNet's radius, sub-cell offsets, log sizes,
cos / sin headings, flat cell indices, masks) and ``get_loss`` (:220-250: CenterNet focal loss on the clamped sigmoid + masked
L1 on the gathered regression maps, ``code_weights`` / ``loc_weight``) -- pinned to a training step of the reference's own
module with its own loss classes (tests/golden/det_head_train.npz: targets, loss terms, every parameter gradient).

``fused_convs`` (off by default; yaml key ``FUSED_CONVS``): in eval mode with autograd off, an fp32 GPU input and no AMP, the
convolutions of a head that ``head_conv.supported`` covers (every branch ``num_conv == 2`` with at most 16 maps, Cin in {64, 256,
384, 512}, SHARED_CONV_CHANNEL in {32, 64}, BatchNorm2d with running statistics) run on csrc/head_conv.hip -- the stages that
``head_conv.ROUTED`` names -- and produce the same ``pred_dicts``; decoding is unchanged.  Under any other condition, and for
any other head, the forward is the library's, untouched.

``fused_train`` (off by default; yaml key ``FUSED_TRAIN``): in training mode with autograd on, an fp32 GPU input and no AMP, the
shared layer and the first convolution of every branch of a head that ``head_conv_train.train_supported`` covers (the same
structure and sizes) run forward and backward on csrc/head_conv.hip -- the stages that ``head_conv_train.ROUTED_TRAIN`` names --
through ``head_conv_train.forward_train``; the last convolutions, every BatchNorm2d and every ReLU stay the modules they are.
``fused_bn`` (off by default; yaml key ``FUSED_BN``) takes effect only where and when ``fused_train`` does: the BatchNorm2d +
ReLU pairs behind a routed stage run through ``bn_train.bn_relu`` for the widths of ``head_conv_train.ROUTED_BN``.  Under any
other condition the forward is exactly the library's."""
import copy

import numpy as np
import torch
from torch import nn

from . import _lib, head_conv, head_conv_train, iou3d_nms_utils


def _get(cfg, key, default=None):
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


class SeparateHead(nn.Module):
    def __init__(self, input_channels, sep_head_dict, init_bias=-2.19, use_bias=False):
        super().__init__()
        self.sep_head_dict = sep_head_dict
        for name, spec in sep_head_dict.items():
            layers = []
            for _ in range(int(spec["num_conv"]) - 1):
                layers.append(nn.Sequential(nn.Conv2d(input_channels, input_channels, 3, 1, 1, bias=use_bias),
                                            nn.BatchNorm2d(input_channels), nn.ReLU()))
            layers.append(nn.Conv2d(input_channels, int(spec["out_channels"]), 3, 1, 1, bias=True))
            fc = nn.Sequential(*layers)
            if "hm" in name:
                fc[-1].bias.data.fill_(init_bias)
            else:
                for m in fc.modules():
                    if isinstance(m, nn.Conv2d):
                        nn.init.kaiming_normal_(m.weight.data)
                        if m.bias is not None:
                            nn.init.constant_(m.bias, 0)
            setattr(self, name, fc)

    def forward(self, x):
        return {name: getattr(self, name)(x) for name in self.sep_head_dict}


def class_agnostic_nms(box_scores, box_preds, nms_config, score_thresh=None, idx=None, nms_fn=None):
    """ref model_nms_utils.class_agnostic_nms (:6-38): top NMS_PRE_MAXSIZE by score -> NMS -> first NMS_POST_MAXSIZE."""
    src_scores = box_scores
    scores_mask = None
    if score_thresh is not None:
        scores_mask = box_scores >= score_thresh
        box_scores, box_preds = box_scores[scores_mask], box_preds[scores_mask]
    thr = _get(nms_config, "NMS_THRESH")
    if isinstance(thr, (list, tuple)):
        thr = thr[idx] if idx is not None else thr[0]
    selected = torch.zeros(0, dtype=torch.long, device=box_scores.device)
    if box_scores.shape[0] > 0:
        top_scores, indices = torch.topk(box_scores, k=min(int(_get(nms_config, "NMS_PRE_MAXSIZE")), box_scores.shape[0]))
        fn = nms_fn or getattr(iou3d_nms_utils, _get(nms_config, "NMS_TYPE"))
        keep, _ = fn(box_preds[indices][:, 0:7], top_scores, thr)
        selected = indices[keep[:int(_get(nms_config, "NMS_POST_MAXSIZE"))]]
    if scores_mask is not None:
        selected = scores_mask.nonzero().view(-1)[selected]
    return selected, src_scores[selected]


def decode_bbox_from_heatmap(heatmap, rot_cos, rot_sin, center, center_z, dim, point_cloud_range, voxel_size,
                             feature_map_stride, vel=None, K=100, score_thresh=None, post_center_limit_range=None):
    """ref centernet_utils.decode_bbox_from_heatmap (:154-216); the two-stage top-K of ``_topk`` (:136-151) equals a
    top-K over all (class, cell) pairs."""
    B, ncls, H, W = heatmap.shape
    scores, flat = torch.topk(heatmap.reshape(B, -1), K)
    cls = (flat // (H * W)).int()
    cell = flat % (H * W)
    ys, xs = (cell // W).float(), (cell % W).float()

    def pick(t):  # (B, c, H, W) -> (B, K, c) at the peak cells
        c = t.shape[1]
        return t.permute(0, 2, 3, 1).reshape(B, H * W, c).gather(1, cell.unsqueeze(2).expand(B, K, c))

    ctr, cz, dm = pick(center), pick(center_z), pick(dim)
    angle = torch.atan2(pick(rot_sin), pick(rot_cos))
    x = (xs.unsqueeze(2) + ctr[:, :, 0:1]) * feature_map_stride * voxel_size[0] + point_cloud_range[0]
    y = (ys.unsqueeze(2) + ctr[:, :, 1:2]) * feature_map_stride * voxel_size[1] + point_cloud_range[1]
    parts = [x, y, cz, dm, angle]
    if vel is not None:
        parts.append(pick(vel))
    boxes = torch.cat(parts, dim=-1)
    mask = (boxes[..., :3] >= post_center_limit_range[:3]).all(2) & (boxes[..., :3] <= post_center_limit_range[3:]).all(2)
    if score_thresh is not None:
        mask &= scores > score_thresh
    return [dict(pred_boxes=boxes[b, mask[b]], pred_scores=scores[b, mask[b]], pred_labels=cls[b, mask[b]])
            for b in range(B)]


CENTER_DECODE_MAX_K = 4096  # include/mssvt_hip.h MSSVT_CENTER_DECODE_MAX_K


def center_decode(hm, center, center_z, dim, rot, vel=None, *, point_cloud_range, voxel_size, feature_map_stride, K=100,
                  score_thresh=None, post_center_limit_range):
    """``decode_bbox_from_heatmap`` of ONE head for the whole batch on the device (csrc/center_decode.hip), a fixed number
    of launches and no host synchronisation.  hm (B, C, H, W) RAW logits, dim the raw log sizes, rot [cos, sin]; other
    float dtypes are converted.  The cells are ranked by (logit descending, flat index ascending) -- exact and
    deterministic, a refinement of ``topk(sigmoid(hm))``; a NaN logit never yields a box.  Returns the survivors of the
    centre-range / score filters in rank order, padded: cand_boxes (B, K, 7 + V) f32, cand_scores (B, K) f32,
    cand_labels (B, K) i32 (class inside the head), cand_num (B) i32; the tails are zero."""
    maps = [hm, center, center_z, dim, rot] + ([vel] if vel is not None else [])
    if not all(t.is_cuda and t.dim() == 4 for t in maps):
        raise _lib.MssvtHipError("center_decode needs (B, C, H, W) maps on the GPU (no CPU path)")
    maps = [t.detach().float().contiguous() for t in maps]
    hm, center, center_z, dim, rot = maps[:5]
    vel = maps[5] if vel is not None else None
    B, C, H, W = (int(v) for v in hm.shape)
    V = int(vel.shape[1]) if vel is not None else 0
    for t, c in ((center, 2), (center_z, 1), (dim, 3), (rot, 2)) + (((vel, V),) if V else ()):
        if tuple(t.shape) != (B, c, H, W) or t.device != hm.device:
            raise _lib.MssvtHipError("center_decode: a regression map is not (%d, %d, %d, %d) on the heat map's device" % (B, c, H, W))
    K = int(K)
    if K < 0:
        raise _lib.MssvtHipError("center_decode: K = %d is negative" % K)
    dev = hm.device
    if min(B, C, H, W, K) == 0:  # an empty batch / map / K: nothing to select, no launch
        return (torch.zeros((B, K, 7 + V), dtype=torch.float32, device=dev), torch.zeros((B, K), dtype=torch.float32, device=dev),
                torch.zeros((B, K), dtype=torch.int32, device=dev), torch.zeros((B,), dtype=torch.int32, device=dev))
    nbytes = int(_lib.lib().mssvt_center_decode_workspace_bytes(B, C, H, W, K))
    if nbytes <= 0:
        raise _lib.MssvtHipError("center_decode: shape beyond the kernel's limits (B <= 65535, C <= 255, C H W < 2^24, "
                                 "K <= %d): B=%d C=%d H=%d W=%d K=%d" % (CENTER_DECODE_MAX_K, B, C, H, W, K))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)  # cleared by the call, on this stream
    cand_boxes = torch.empty((B, K, 7 + V), dtype=torch.float32, device=dev)  # all four fully written by the call
    cand_scores = torch.empty((B, K), dtype=torch.float32, device=dev)
    cand_labels = torch.empty((B, K), dtype=torch.int32, device=dev)
    cand_num = torch.empty((B,), dtype=torch.int32, device=dev)
    lim = [float(v) for v in post_center_limit_range]
    _lib.call("mssvt_center_decode", B, C, H, W, V, hm.data_ptr(), center.data_ptr(), center_z.data_ptr(), dim.data_ptr(),
              rot.data_ptr(), _lib.ptr(vel), K, float(feature_map_stride), float(voxel_size[0]), float(voxel_size[1]),
              float(point_cloud_range[0]), float(point_cloud_range[1]), lim[0], lim[1], lim[2], lim[3], lim[4], lim[5],
              0 if score_thresh is None else 1, 0.0 if score_thresh is None else float(score_thresh), _lib.ptr(ws),
              _lib.ptr(cand_boxes), _lib.ptr(cand_scores), _lib.ptr(cand_labels), _lib.ptr(cand_num), _lib.stream())
    return cand_boxes, cand_scores, cand_labels, cand_num


def unpad(padded):
    """The list of per-sample dicts that ``generate_predicted_boxes`` returns, from the padded dict of
    ``generate_predicted_boxes_padded``: ONE read-back (``num``) for the whole batch."""
    nums = padded["num"].tolist()
    return [dict(pred_boxes=padded["pred_boxes"][b, :n], pred_scores=padded["pred_scores"][b, :n],
                 pred_labels=padded["pred_labels"][b, :n]) for b, n in enumerate(nums)]


def gaussian_radius(height, width, min_overlap):
    """CornerNet's radius: the smallest of the three roots that keep a shifted box above `min_overlap` IoU
    (ref centernet_utils.py:9-35); vectorised over the objects."""
    s, p = height + width, height * width
    r1 = (s + (s * s - 4.0 * p * (1.0 - min_overlap) / (1.0 + min_overlap)).sqrt()) / 2.0
    r2 = (2.0 * s + (4.0 * s * s - 16.0 * (1.0 - min_overlap) * p).sqrt()) / 2.0
    b3 = -2.0 * min_overlap * s
    r3 = (b3 + (b3 * b3 - 16.0 * min_overlap * (min_overlap - 1.0) * p).sqrt()) / 2.0
    return torch.min(torch.min(r1, r2), r3)


def splat_gaussian(heatmap, cx, cy, radius):
    """max-merge a (2 r + 1)^2 Gaussian (sigma = (2 r + 1) / 6, evaluated in float64, entries below eps x peak dropped)
    centred on cell (cx, cy) into `heatmap` (H, W), clipped at the borders (ref centernet_utils.py:38-69)."""
    H, W = heatmap.shape
    ax = np.arange(-radius, radius + 1, dtype=np.float64)
    sigma = (2 * radius + 1) / 6.0
    g = np.exp(-(ax[None, :] ** 2 + ax[:, None] ** 2) / (2.0 * sigma * sigma))
    g[g < np.finfo(g.dtype).eps * g.max()] = 0
    left, right = min(cx, radius), min(W - cx, radius + 1)
    top, bottom = min(cy, radius), min(H - cy, radius + 1)
    if right + left <= 0 or bottom + top <= 0:
        return
    patch = torch.from_numpy(g[radius - top:radius + bottom, radius - left:radius + right]).to(heatmap.device).float()
    region = heatmap[cy - top:cy + bottom, cx - left:cx + right]
    if min(patch.shape) > 0 and min(region.shape) > 0:
        torch.max(region, patch, out=region)


def center_targets(gt_boxes, class_of_label, num_classes, feature_map_size, point_cloud_range, voxel_size,
                   feature_map_stride, num_max_objs=500, gaussian_overlap=0.1, min_radius=2):
    """The training targets of ONE head for the whole batch in one launch (csrc/center_targets.hip): what
    ``CenterHead.assign_target_of_single_head`` computes per sample on the host (ref center_head.py:103-158,
    centernet_utils.py:9-69), without a copy or a synchronisation.  gt_boxes (B, N, 8+) on the device, label last;
    class_of_label (C + 1) int32 on the device: the class inside the head of label 0..C or -1 (``CenterHead.label_tables``);
    feature_map_size (H, W).  Returns heatmap (B, num_classes, H, W) f32, target_boxes (B, M, 8+) f32, inds and mask
    (B, M) i64.  Rows with a non-finite value get no target and a label outside 0..C takes no slot (the host path raises)."""
    if not (gt_boxes.is_cuda and gt_boxes.dim() == 3):
        raise _lib.MssvtHipError("center_targets needs (B, N, 8+) boxes on the GPU")
    boxes = gt_boxes.detach().float().contiguous()
    B, N, D = boxes.shape
    H, W = int(feature_map_size[0]), int(feature_map_size[1])
    M, ov = int(num_max_objs), float(gaussian_overlap)
    heatmap = torch.empty((B, int(num_classes), H, W), dtype=torch.float32, device=boxes.device)
    target_boxes = torch.empty((B, M, D), dtype=torch.float32, device=boxes.device)
    inds = torch.empty((B, M), dtype=torch.int64, device=boxes.device)
    mask = torch.empty((B, M), dtype=torch.int64, device=boxes.device)
    # the constants of gaussian_radius: Python-scalar sub-expressions, folded in double and rounded to float32 once
    _lib.call("mssvt_center_targets", B, N, D, boxes.data_ptr(), _lib.ptr(class_of_label), class_of_label.numel(),
              int(num_classes), H, W, M, float(point_cloud_range[0]), float(point_cloud_range[1]), float(voxel_size[0]),
              float(voxel_size[1]), float(feature_map_stride), 1.0 - ov, 1.0 + ov, 16.0 * (1.0 - ov), -2.0 * ov,
              16.0 * ov * (ov - 1.0), int(min_radius), _lib.ptr(heatmap), _lib.ptr(target_boxes), _lib.ptr(inds),
              _lib.ptr(mask), _lib.stream())
    return heatmap, target_boxes, inds, mask


def centernet_focal_loss(pred, gt):
    """ref loss_utils.py:264-299 (CornerNet's penalty-reduced focal loss): pred = clamped sigmoid, gt = Gaussian heat map."""
    pos = gt.eq(1).float()
    neg = gt.lt(1).float()
    pos_term = (torch.log(pred) * torch.pow(1 - pred, 2) * pos).sum()
    neg_term = (torch.log(1 - pred) * torch.pow(pred, 2) * torch.pow(1 - gt, 4) * neg).sum()
    num_pos = pos.sum()
    return -neg_term if num_pos == 0 else -(pos_term + neg_term) / num_pos


def centernet_reg_loss(maps, mask, ind, target):
    """ref loss_utils.py:314-386: L1 between the regression maps gathered at the objects' cells and the targets, per code
    dimension, over the masked objects of the whole batch / their number.  maps (B, D, H, W), ind / mask (B, M), target (B, M, D)."""
    B, D = maps.shape[0], maps.shape[1]
    flat = maps.permute(0, 2, 3, 1).reshape(B, -1, D)
    pred = flat.gather(1, ind.unsqueeze(2).expand(-1, -1, D))
    num = mask.float().sum()
    m = mask.unsqueeze(2).expand_as(target).float() * (~torch.isnan(target)).float()
    per_dim = torch.abs(pred * m - target * m).sum(dim=(0, 1))
    return per_dim / torch.clamp_min(num, 1.0)


CENTER_LOSS_SWEEP = 1024  # include/mssvt_hip.h MSSVT_CENTER_LOSS_SWEEP: elements per workgroup and grid-stride step
CENTER_LOSS_MAX_BLOCKS = 2048  # MSSVT_CENTER_LOSS_MAX_BLOCKS
CENTER_LOSS_MAX_OBJS = 4096  # MSSVT_CENTER_LOSS_MAX_OBJS
CENTER_LOSS_MAX_CODE = 16  # MSSVT_CENTER_LOSS_MAX_CODE
CENTER_LOSS_MAX_MAPS = 6


def _map_args(maps):
    """Six (pointer, channels) pairs: the maps, then NULL / 0."""
    pairs = [(_lib.ptr(t), int(t.shape[1])) for t in maps] + [(None, 0)] * (CENTER_LOSS_MAX_MAPS - len(maps))
    return [v for pair in pairs for v in pair]


class _CenterLoss(torch.autograd.Function):
    """csrc/center_loss.hip under autograd: float32 contiguous device tensors only (``center_loss`` converts)."""

    @staticmethod
    def forward(ctx, hm, heatmap, target_boxes, inds, masks, code_weights, loc_weight, *reg_maps):
        B, C, H, W = (int(v) for v in hm.shape)
        M, DT = int(target_boxes.shape[1]), int(target_boxes.shape[2])
        D = sum(int(t.shape[1]) for t in reg_maps)
        nbytes = int(_lib.lib().mssvt_center_loss_workspace_bytes(B, C, H, W, M, D))
        if nbytes <= 0:
            raise _lib.MssvtHipError("center_loss: shape beyond the kernel's limits (M <= %d, D <= %d, B C H W < 2^31): "
                                     "B=%d C=%d H=%d W=%d M=%d D=%d" % (CENTER_LOSS_MAX_OBJS, CENTER_LOSS_MAX_CODE, B, C, H, W, M, D))
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=hm.device)  # fully written before it is read
        out = torch.empty(4 + D, dtype=torch.float32, device=hm.device)
        m = _map_args(reg_maps)
        _lib.call("mssvt_center_loss_forward", B, C, H, W, M, D, DT, hm.data_ptr(), _lib.ptr(heatmap), m[0], m[1], m[2], m[3],
                  m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11], _lib.ptr(target_boxes), _lib.ptr(inds), _lib.ptr(masks),
                  _lib.ptr(code_weights), float(loc_weight), ws.data_ptr(), out.data_ptr(), _lib.stream())
        ctx.save_for_backward(hm, heatmap, target_boxes, inds, masks, code_weights, out, *reg_maps)
        ctx.loc_weight = float(loc_weight)
        ctx.set_materialize_grads(False)  # an absent upstream gradient stays None: NULL, no zero tensor is built
        hm_loss, loc_loss, per_dim = out[0], out[1], out[4:4 + D]
        ctx.mark_non_differentiable(per_dim)
        return hm_loss, loc_loss, per_dim

    @staticmethod
    def backward(ctx, g_hm, g_loc, _g_per_dim):
        hm, heatmap, target_boxes, inds, masks, code_weights, out = ctx.saved_tensors[:7]
        reg_maps = ctx.saved_tensors[7:]
        B, C, H, W = (int(v) for v in hm.shape)
        M, DT = int(target_boxes.shape[1]), int(target_boxes.shape[2])
        D = sum(int(t.shape[1]) for t in reg_maps)
        # an absent upstream gradient is zero (NULL); a present one is a float32 device scalar
        g_hm = None if g_hm is None else g_hm.float().contiguous()
        g_loc = None if g_loc is None else g_loc.float().contiguous()
        d_hm = None
        if ctx.needs_input_grad[0]:  # on hm's 16-byte phase, so that the pass keeps its 16-byte stores
            phase = (hm.data_ptr() % 16) // 4
            d_hm = torch.empty(hm.numel() + 3, dtype=torch.float32, device=hm.device)[phase:phase + hm.numel()].view(hm.shape)
        d_maps = [torch.empty_like(t) if ctx.needs_input_grad[7 + k] else None for k, t in enumerate(reg_maps)]
        m = _map_args(reg_maps)
        dm = [_lib.ptr(t) for t in d_maps] + [None] * (CENTER_LOSS_MAX_MAPS - len(d_maps))
        _lib.call("mssvt_center_loss_backward", B, C, H, W, M, D, DT, hm.data_ptr(), _lib.ptr(heatmap), m[0], m[1], m[2],
                  m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11], _lib.ptr(target_boxes), _lib.ptr(inds),
                  _lib.ptr(masks), _lib.ptr(code_weights), ctx.loc_weight, out.data_ptr(), _lib.ptr(g_hm), _lib.ptr(g_loc),
                  _lib.ptr(d_hm), dm[0], dm[1], dm[2], dm[3], dm[4], dm[5], _lib.stream())
        return (d_hm, None, None, None, None, None, None) + tuple(d_maps)


def center_loss(hm, reg_maps, heatmap, target_boxes, inds, masks, code_weights, loc_weight):
    """The loss of ONE head on the device (csrc/center_loss.hip): ``centernet_focal_loss`` of the clamped sigmoid of the
    RAW logits hm (B, C, H, W) against heatmap, and loc_weight x sum(code_weights x ``centernet_reg_loss``) of the
    regression maps -- a list of (B, c_k, H, W) tensors in HEAD_ORDER, never concatenated -- at inds / masks (B, M) against
    target_boxes (B, M, D') whose first D = sum(c_k) columns are used.  Returns (hm_loss, loc_loss, per_dim): 0-d, 0-d and
    (D) float32 on the device; differentiable in hm and in every map (two launches forward, at most three backward, no float
    atomics: bit-identical run to run), per_dim detached.  Nothing is read back: the ``num_pos == 0`` branch is taken on
    the device.  A masked-out slot is not read; an unmasked slot whose index lies outside the map counts in the number of
    objects and gives neither loss nor gradient.  Other float dtypes are converted here, under autograd.  code_weights: D
    numbers or a device tensor (a list costs a host-to-device copy: ``CenterHead`` keeps the tensor)."""
    reg_maps = list(reg_maps)
    if not (hm.is_cuda and hm.dim() == 4 and all(t.is_cuda and t.dim() == 4 for t in reg_maps)):
        raise _lib.MssvtHipError("center_loss needs (B, C, H, W) maps on the GPU (no CPU path)")
    if not (heatmap.is_cuda and target_boxes.is_cuda and inds.is_cuda and masks.is_cuda):
        raise _lib.MssvtHipError("center_loss needs its targets on the GPU (no CPU path)")
    if len(reg_maps) > CENTER_LOSS_MAX_MAPS:
        raise _lib.MssvtHipError("center_loss: %d regression maps, the kernel takes %d" % (len(reg_maps), CENTER_LOSS_MAX_MAPS))
    B, C, H, W = (int(v) for v in hm.shape)
    D = sum(int(t.shape[1]) for t in reg_maps)
    dev = hm.device
    for t in reg_maps:
        if (int(t.shape[0]), int(t.shape[2]), int(t.shape[3])) != (B, H, W) or t.device != dev:
            raise _lib.MssvtHipError("center_loss: a regression map is not (%d, c, %d, %d) on the heat map's device" % (B, H, W))
    if tuple(heatmap.shape) != (B, C, H, W) or target_boxes.dim() != 3 or int(target_boxes.shape[0]) != B or \
            tuple(inds.shape) != tuple(target_boxes.shape[:2]) or tuple(masks.shape) != tuple(inds.shape):
        raise _lib.MssvtHipError("center_loss: heatmap must be %s, target_boxes (B, M, D'), inds / masks (B, M)" % ((B, C, H, W),))
    M, DT = int(target_boxes.shape[1]), int(target_boxes.shape[2])
    if DT < D:
        raise _lib.MssvtHipError("center_loss: target_boxes has %d columns, the maps have %d channels" % (DT, D))
    if min(B, C, H, W, M) == 0 or D == 0:
        raise _lib.MssvtHipError("center_loss: empty shape B=%d C=%d H=%d W=%d M=%d D=%d (CenterHead.get_loss keeps the torch "
                                 "expressions for these)" % (B, C, H, W, M, D))
    if not torch.is_tensor(code_weights):
        code_weights = torch.tensor([float(v) for v in code_weights], dtype=torch.float32, device=dev)
    code_weights = code_weights.detach().to(device=dev, dtype=torch.float32).contiguous()
    if code_weights.numel() != D:
        raise _lib.MssvtHipError("center_loss: %d code weights for %d code dimensions" % (code_weights.numel(), D))
    return _CenterLoss.apply(hm.float().contiguous(), heatmap.detach().float().contiguous(),
                             target_boxes.detach().float().contiguous(), inds.detach().long().contiguous(),
                             masks.detach().long().contiguous(), code_weights, float(loc_weight),
                             *[t.float().contiguous() for t in reg_maps])


class CenterHead(nn.Module):
    def __init__(self, model_cfg, input_channels, num_class, class_names, grid_size, point_cloud_range, voxel_size,
                 predict_boxes_when_training=True):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.grid_size, self.point_cloud_range, self.voxel_size = grid_size, point_cloud_range, voxel_size
        self.feature_map_stride = _get(_get(model_cfg, "TARGET_ASSIGNER_CONFIG"), "FEATURE_MAP_STRIDE", None)
        self.class_names = list(class_names)
        self.class_names_each_head, maps = [], []
        for names in _get(model_cfg, "CLASS_NAMES_EACH_HEAD"):
            cur = [x for x in names if x in self.class_names]
            self.class_names_each_head.append(cur)
            maps.append(torch.from_numpy(np.array([self.class_names.index(x) for x in cur], dtype=np.int64)))
        self._class_maps = maps  # moved to the features' device on use (the reference calls .cuda() in the constructor)
        assert sum(len(x) for x in self.class_names_each_head) == len(self.class_names)
        shared = int(_get(model_cfg, "SHARED_CONV_CHANNEL"))
        use_bias = bool(_get(model_cfg, "USE_BIAS_BEFORE_NORM", False))
        self.shared_conv = nn.Sequential(nn.Conv2d(input_channels, shared, 3, stride=1, padding=1, bias=use_bias),
                                         nn.BatchNorm2d(shared), nn.ReLU())
        self.separate_head_cfg = _get(model_cfg, "SEPARATE_HEAD_CFG")
        self.heads_list = nn.ModuleList()
        for cur in self.class_names_each_head:
            head_dict = copy.deepcopy({k: dict(v) for k, v in dict(_get(self.separate_head_cfg, "HEAD_DICT")).items()})
            head_dict["hm"] = dict(out_channels=len(cur), num_conv=int(_get(model_cfg, "NUM_HM_CONV")))
            self.heads_list.append(SeparateHead(shared, head_dict, init_bias=-2.19, use_bias=use_bias))
        self.predict_boxes_when_training = predict_boxes_when_training
        self.forward_ret_dict = {}
        self.nms_fn = None  # test hook: an alternative NMS with the signature of iou3d_nms_utils.nms_gpu
        self._label_tables_dev = {}  # device -> label_tables() as an int32 tensor (heads, C + 1)
        self._class_maps_dev = {}  # device -> _class_maps on that device (generate_predicted_boxes_padded)
        self.padded_predictions = False  # eval forward: final_box_padded (no host sync) instead of final_box_dicts
        self.fused_loss = False  # get_loss on the GPU: center_loss per head, tb_dict as device tensors (no host sync)
        self._code_weights_dev = {}  # device -> LOSS_WEIGHTS.code_weights as a float32 tensor (get_loss with fused_loss)
        # eval forward without autograd, fp32 on the GPU, no AMP (bev_conv.switch_applies) and a head head_conv.supported
        # covers: the convolutions on csrc/head_conv.hip (the stages head_conv.ROUTED names); anything else: the library
        self.fused_convs = bool(_get(model_cfg, "FUSED_CONVS", False))
        # training forward with autograd on, fp32 on the GPU, no AMP and a head head_conv_train.train_supported covers: the
        # shared layer and the trunk through head_conv_train's Functions (the stages ROUTED_TRAIN names); fused_bn: the
        # BatchNorm2d + ReLU pairs behind them through bn_train (the widths ROUTED_BN names), inert without fused_train
        self.fused_train = bool(_get(model_cfg, "FUSED_TRAIN", False))
        self.fused_bn = bool(_get(model_cfg, "FUSED_BN", False))

    def label_tables(self):
        """int array [label 0..C][head]: the class inside the head that a box of that label gets, or -1 when the head
        does not take it.  Simulates the re-labelling of ``assign_targets`` (ref :190-193): a box that head h takes has its
        label overwritten with its index inside h + 1, and the FOLLOWING heads look that number up in the global class
        list again -- with heads [[Pedestrian], [Vehicle, Cyclist]] a Pedestrian also lands in head 1 as class 0."""
        names = ["bg"] + self.class_names
        table = np.full((len(names), len(self.class_names_each_head)), -1, dtype=np.int32)
        for label in range(len(names)):
            cur = label
            for h, head_names in enumerate(self.class_names_each_head):
                if names[cur] in head_names:
                    table[label, h] = head_names.index(names[cur])
                    cur = int(table[label, h]) + 1
        return table

    def _label_table_on(self, device):
        t = self._label_tables_dev.get(device)
        if t is None:
            t = torch.from_numpy(np.ascontiguousarray(self.label_tables().T)).to(device)
            self._label_tables_dev[device] = t
        return t

    def generate_predicted_boxes(self, batch_size, pred_dicts):
        post = _get(self.model_cfg, "POST_PROCESSING")
        nms_cfg = _get(post, "NMS_CONFIG")
        dev = pred_dicts[0]["hm"].device
        limit = torch.tensor(list(_get(post, "POST_CENTER_LIMIT_RANGE")), dtype=torch.float32, device=dev)
        ret = [dict(pred_boxes=[], pred_scores=[], pred_labels=[]) for _ in range(batch_size)]
        has_vel = "vel" in list(_get(self.separate_head_cfg, "HEAD_ORDER"))
        for idx, pd in enumerate(pred_dicts):
            finals = decode_bbox_from_heatmap(
                heatmap=pd["hm"].sigmoid(), rot_cos=pd["rot"][:, 0:1], rot_sin=pd["rot"][:, 1:2], center=pd["center"],
                center_z=pd["center_z"], dim=pd["dim"].exp(), vel=pd["vel"] if has_vel else None,
                point_cloud_range=self.point_cloud_range, voxel_size=self.voxel_size,
                feature_map_stride=self.feature_map_stride, K=int(_get(post, "MAX_OBJ_PER_SAMPLE")),
                score_thresh=_get(post, "SCORE_THRESH"), post_center_limit_range=limit)
            cmap = self._class_maps[idx].to(dev)
            thr = _get(nms_cfg, "NMS_THRESH")
            per_class = isinstance(thr, (list, tuple)) and len(thr) > 1
            for k, fd in enumerate(finals):
                if per_class:  # one threshold per class of this head (ref :283-305)
                    boxes, scores, labels = [], [], []
                    for i in range(len(thr)):
                        sel_c = fd["pred_labels"] == i
                        cb, cs = fd["pred_boxes"][sel_c], fd["pred_scores"][sel_c]
                        cl = cmap[fd["pred_labels"][sel_c].long()]
                        sel, ssc = class_agnostic_nms(cs, cb, nms_cfg, None, idx=i, nms_fn=self.nms_fn)
                        boxes.append(cb[sel]); scores.append(ssc); labels.append(cl[sel])
                    fd = dict(pred_boxes=torch.cat(boxes, 0), pred_scores=torch.cat(scores, 0),
                              pred_labels=torch.cat(labels, 0))
                else:
                    labels = cmap[fd["pred_labels"].long()]
                    sel, ssc = class_agnostic_nms(fd["pred_scores"], fd["pred_boxes"], nms_cfg, None, nms_fn=self.nms_fn)
                    fd = dict(pred_boxes=fd["pred_boxes"][sel], pred_scores=ssc, pred_labels=labels[sel])
                for key in ret[k]:
                    ret[k][key].append(fd[key])
        for k in range(batch_size):
            ret[k]["pred_boxes"] = torch.cat(ret[k]["pred_boxes"], dim=0)
            ret[k]["pred_scores"] = torch.cat(ret[k]["pred_scores"], dim=0)
            ret[k]["pred_labels"] = torch.cat(ret[k]["pred_labels"], dim=0) + 1
        return ret

    def _class_maps_on(self, device):
        maps = self._class_maps_dev.get(device)
        if maps is None:
            maps = [m.to(device).contiguous() for m in self._class_maps]
            self._class_maps_dev[device] = maps
        return maps

    def generate_predicted_boxes_padded(self, batch_size, pred_dicts):
        """``generate_predicted_boxes`` without a host synchronisation or a read-back: per head ``center_decode`` (top-K,
        decode, filters) and ``iou3d_nms_utils.nms_padded`` (NMS with the counts on the device), each head appended behind
        the one before it.  Same config keys; returns pred_boxes (B, P, 7 + V) f32, pred_scores (B, P) f32, pred_labels
        (B, P) i64 (1-based over class_names, 0 in the padding) and num (B) i32 with P = heads x NMS_POST_MAXSIZE;
        ``unpad`` turns them into the list.  Covers NMS_TYPE nms_gpu / nms_normal_gpu with one threshold; per-class
        thresholds, a custom ``nms_fn`` or MAX_OBJ_PER_SAMPLE beyond the kernel's limit stay with the list path."""
        post = _get(self.model_cfg, "POST_PROCESSING")
        nms_cfg = _get(post, "NMS_CONFIG")
        dev = pred_dicts[0]["hm"].device
        if dev.type != "cuda":
            raise _lib.MssvtHipError("generate_predicted_boxes_padded runs on the GPU only (no CPU path); "
                                     "generate_predicted_boxes takes CPU tensors")
        thr = _get(nms_cfg, "NMS_THRESH")
        if isinstance(thr, (list, tuple)):
            if len(thr) != 1:
                raise _lib.MssvtHipError("generate_predicted_boxes_padded: per-class NMS_THRESH (%d entries) is not "
                                         "covered, use generate_predicted_boxes" % len(thr))
            thr = thr[0]
        if self.nms_fn is not None:
            raise _lib.MssvtHipError("generate_predicted_boxes_padded: a custom nms_fn is not covered, use generate_predicted_boxes")
        nms_type = _get(nms_cfg, "NMS_TYPE")
        if nms_type not in ("nms_gpu", "nms_normal_gpu"):
            raise _lib.MssvtHipError("generate_predicted_boxes_padded: NMS_TYPE %s is not covered (nms_gpu, nms_normal_gpu)" % nms_type)
        K = int(_get(post, "MAX_OBJ_PER_SAMPLE"))
        if K > CENTER_DECODE_MAX_K:
            raise _lib.MssvtHipError("generate_predicted_boxes_padded: MAX_OBJ_PER_SAMPLE %d exceeds the kernel's limit %d, "
                                     "use generate_predicted_boxes" % (K, CENTER_DECODE_MAX_K))
        has_vel = "vel" in list(_get(self.separate_head_cfg, "HEAD_ORDER"))
        post_max = int(_get(nms_cfg, "NMS_POST_MAXSIZE"))
        cmaps = self._class_maps_on(dev)
        out = None
        for idx, pd in enumerate(pred_dicts):
            cand = center_decode(
                pd["hm"], pd["center"], pd["center_z"], pd["dim"], pd["rot"], pd["vel"] if has_vel else None,
                point_cloud_range=self.point_cloud_range, voxel_size=self.voxel_size,
                feature_map_stride=self.feature_map_stride, K=K, score_thresh=_get(post, "SCORE_THRESH"),
                post_center_limit_range=list(_get(post, "POST_CENTER_LIMIT_RANGE")))
            if out is None:
                out = iou3d_nms_utils.padded_outputs(int(batch_size), len(pred_dicts) * post_max, cand[0].shape[2], dev)
            iou3d_nms_utils.nms_padded(*cand, cmaps[idx], float(thr), int(_get(nms_cfg, "NMS_PRE_MAXSIZE")), post_max,
                                       normal=nms_type == "nms_normal_gpu", out=out)
        return out

    def assign_target_of_single_head(self, num_classes, gt_boxes, feature_map_size, feature_map_stride, num_max_objs=500,
                                     gaussian_overlap=0.1, min_radius=2):
        """gt_boxes (n, 8+) [x, y, z, dx, dy, dz, heading, ..., class in 1..num_classes] of ONE sample and head ->
        heat map (classes, H, W), target boxes (M, 8+), flat cell indices (M), mask (M)  (ref :103-158)."""
        W, H = int(feature_map_size[0]), int(feature_map_size[1])
        heatmap = gt_boxes.new_zeros(num_classes, H, W)
        ret_boxes = gt_boxes.new_zeros((num_max_objs, gt_boxes.shape[-1]))
        inds = gt_boxes.new_zeros(num_max_objs).long()
        mask = gt_boxes.new_zeros(num_max_objs).long()
        n = min(num_max_objs, gt_boxes.shape[0])
        if n == 0:
            return heatmap, ret_boxes, inds, mask
        g = gt_boxes[:n]
        cx = torch.clamp((g[:, 0] - self.point_cloud_range[0]) / self.voxel_size[0] / feature_map_stride, min=0, max=W - 0.5)
        cy = torch.clamp((g[:, 1] - self.point_cloud_range[1]) / self.voxel_size[1] / feature_map_stride, min=0, max=H - 0.5)
        centre = torch.stack((cx, cy), dim=-1)
        cell = centre.int()
        dx = g[:, 3] / self.voxel_size[0] / feature_map_stride
        dy = g[:, 4] / self.voxel_size[1] / feature_map_stride
        radius = torch.clamp_min(gaussian_radius(dx, dy, gaussian_overlap).int(), min=min_radius)
        ok = (dx > 0) & (dy > 0) & (cell[:, 0] >= 0) & (cell[:, 0] <= W) & (cell[:, 1] >= 0) & (cell[:, 1] <= H)
        cls = (g[:, -1] - 1).long()
        for k in torch.nonzero(ok).flatten().tolist():  # (the Gaussians overlap: max-merged in object order)
            splat_gaussian(heatmap[int(cls[k])], int(cell[k, 0]), int(cell[k, 1]), int(radius[k]))
        inds[:n][ok] = (cell[:, 1].long() * W + cell[:, 0].long())[ok]
        mask[:n] = ok.long()
        cols = [centre - cell.to(g.dtype), g[:, 2:3], g[:, 3:6].log(), torch.cos(g[:, 6:7]), torch.sin(g[:, 6:7])]
        if g.shape[1] > 8:
            cols.append(g[:, 7:-1])
        ret_boxes[:n][ok] = torch.cat(cols, dim=1)[ok]  # (skipped objects keep zero rows)
        return heatmap, ret_boxes, inds, mask

    def assign_targets(self, gt_boxes, feature_map_size=None, **kwargs):
        """gt_boxes (B, M, 8+) with the class id (1-based over class_names, 0 = padding) last; feature_map_size (H, W)
        -> per head: heatmaps (B, c, H, W), target_boxes (B, M', 8+), inds / masks (B, M')  (ref :160-214).  As in the
        reference a box reaches a head with its class re-numbered inside that head, and the re-numbering is written into the
        working copy of the boxes that the FOLLOWING heads read their class names from (ref :190-193).
        On the device the targets of a head are one launch (``assign_targets_device``); ``assign_targets_host`` is the CPU
        statement of the same semantics."""
        if gt_boxes.is_cuda:
            return self.assign_targets_device(gt_boxes, feature_map_size)
        return self.assign_targets_host(gt_boxes, feature_map_size)

    def assign_targets_device(self, gt_boxes, feature_map_size):
        """``center_targets`` per head with the head's column of ``label_tables``: nothing is read back, the caller's boxes
        are only read."""
        tcfg = _get(self.model_cfg, "TARGET_ASSIGNER_CONFIG")
        out = dict(heatmaps=[], target_boxes=[], inds=[], masks=[], heatmap_masks=[])
        tables = self._label_table_on(gt_boxes.device)
        for h, head_names in enumerate(self.class_names_each_head):
            res = center_targets(
                gt_boxes, tables[h], len(head_names), feature_map_size, self.point_cloud_range, self.voxel_size,
                _get(tcfg, "FEATURE_MAP_STRIDE"), num_max_objs=_get(tcfg, "NUM_MAX_OBJS"),
                gaussian_overlap=_get(tcfg, "GAUSSIAN_OVERLAP"), min_radius=_get(tcfg, "MIN_RADIUS"))
            out["heatmaps"].append(res[0].to(gt_boxes.dtype))
            out["target_boxes"].append(res[1].to(gt_boxes.dtype))
            out["inds"].append(res[2])
            out["masks"].append(res[3])
        return out

    def assign_targets_host(self, gt_boxes, feature_map_size):
        """The per-sample host loop of the reference (ref :160-214): boxes of any device, every sample's targets computed
        on the CPU and moved to the boxes' device."""
        size_xy = list(feature_map_size)[::-1]
        tcfg = _get(self.model_cfg, "TARGET_ASSIGNER_CONFIG")
        work = gt_boxes.clone()
        names = ["bg"] + self.class_names
        out = dict(heatmaps=[], target_boxes=[], inds=[], masks=[], heatmap_masks=[])
        for head_names in self.class_names_each_head:
            per_sample = []
            for b in range(work.shape[0]):
                boxes = work[b]
                labels = boxes[:, -1].long().tolist()
                rows = [i for i, c in enumerate(labels) if names[c] in head_names]
                for i in rows:
                    boxes[i, -1] = head_names.index(names[labels[i]]) + 1
                sel = boxes[rows] if rows else boxes[:0]
                per_sample.append(self.assign_target_of_single_head(
                    num_classes=len(head_names), gt_boxes=sel.cpu(), feature_map_size=size_xy,
                    feature_map_stride=_get(tcfg, "FEATURE_MAP_STRIDE"), num_max_objs=_get(tcfg, "NUM_MAX_OBJS"),
                    gaussian_overlap=_get(tcfg, "GAUSSIAN_OVERLAP"), min_radius=_get(tcfg, "MIN_RADIUS")))
            for key, j in (("heatmaps", 0), ("target_boxes", 1), ("inds", 2), ("masks", 3)):
                out[key].append(torch.stack([t[j] for t in per_sample], dim=0).to(gt_boxes.device))
        return out

    def _code_weights_on(self, device):
        t = self._code_weights_dev.get(device)
        if t is None:
            weights = _get(_get(self.model_cfg, "LOSS_CONFIG"), "LOSS_WEIGHTS")
            t = torch.tensor([float(v) for v in weights["code_weights"]], dtype=torch.float32, device=device)
            self._code_weights_dev[device] = t
        return t

    def get_loss_fused(self):
        """``get_loss`` with ``center_loss`` per head (csrc/center_loss.hip): two launches forward and at most three
        backward per head, and no host synchronisation -- the loss terms of tb_dict are detached 0-d device tensors, read
        them back when they are logged.  A head without object slots or with an empty map keeps the torch expressions."""
        weights = _get(_get(self.model_cfg, "LOSS_CONFIG"), "LOSS_WEIGHTS")
        order = list(_get(self.separate_head_cfg, "HEAD_ORDER"))
        td = self.forward_ret_dict["target_dicts"]
        loss, tb = 0, {}
        for idx, pd in enumerate(self.forward_ret_dict["pred_dicts"]):
            if td["inds"][idx].numel() == 0 or pd["hm"].numel() == 0:
                hm = torch.clamp(pd["hm"].sigmoid(), min=1e-4, max=1 - 1e-4)
                hm_loss = centernet_focal_loss(hm, td["heatmaps"][idx])
                reg = centernet_reg_loss(torch.cat([pd[name] for name in order], dim=1), td["masks"][idx], td["inds"][idx],
                                         td["target_boxes"][idx])
                loc_loss = (reg * reg.new_tensor(list(weights["code_weights"]))).sum() * weights["loc_weight"]
            else:
                hm_loss, loc_loss, _ = center_loss(pd["hm"], [pd[name] for name in order], td["heatmaps"][idx],
                                                   td["target_boxes"][idx], td["inds"][idx], td["masks"][idx],
                                                   self._code_weights_on(pd["hm"].device), weights["loc_weight"])
            loss = loss + hm_loss + loc_loss
            tb["hm_loss_head_%d" % idx] = hm_loss.detach()
            tb["loc_loss_head_%d" % idx] = loc_loss.detach()
        tb["rpn_loss"] = loss.detach()
        return loss, tb

    def get_loss(self):
        """ref :220-250: per head the focal loss of the clamped sigmoid heat map + loc_weight x sum(code_weights x L1)."""
        if self.fused_loss and self.forward_ret_dict["pred_dicts"][0]["hm"].is_cuda:
            return self.get_loss_fused()
        weights = _get(_get(self.model_cfg, "LOSS_CONFIG"), "LOSS_WEIGHTS")
        order = list(_get(self.separate_head_cfg, "HEAD_ORDER"))
        loss, tb = 0, {}
        for idx, pd in enumerate(self.forward_ret_dict["pred_dicts"]):
            td = self.forward_ret_dict["target_dicts"]
            hm = torch.clamp(pd["hm"].sigmoid(), min=1e-4, max=1 - 1e-4)
            hm_loss = centernet_focal_loss(hm, td["heatmaps"][idx])
            reg = centernet_reg_loss(torch.cat([pd[name] for name in order], dim=1), td["masks"][idx], td["inds"][idx],
                                     td["target_boxes"][idx])
            loc_loss = (reg * reg.new_tensor(list(weights["code_weights"]))).sum() * weights["loc_weight"]
            loss = loss + hm_loss + loc_loss
            tb["hm_loss_head_%d" % idx] = hm_loss.item()
            tb["loc_loss_head_%d" % idx] = loc_loss.item()
        tb["rpn_loss"] = loss.item()
        return loss, tb

    def forward(self, data_dict):
        if self.fused_convs and head_conv.applies(self, data_dict["spatial_features_2d"]):
            pred_dicts = head_conv.forward(self, data_dict["spatial_features_2d"])
        elif self.fused_train and head_conv_train.applies(self, data_dict["spatial_features_2d"]):
            pred_dicts = head_conv_train.forward_train(self, data_dict["spatial_features_2d"])
        else:
            x = self.shared_conv(data_dict["spatial_features_2d"])
            pred_dicts = [head(x) for head in self.heads_list]
        if self.training:
            self.forward_ret_dict["target_dicts"] = self.assign_targets(
                data_dict["gt_boxes"], feature_map_size=data_dict["spatial_features_2d"].shape[2:])
        self.forward_ret_dict["pred_dicts"] = pred_dicts
        if not self.training or self.predict_boxes_when_training:
            if self.padded_predictions and not self.training:
                with torch.no_grad():
                    data_dict["final_box_padded"] = self.generate_predicted_boxes_padded(data_dict["batch_size"], pred_dicts)
                return data_dict
            with torch.no_grad():
                boxes = self.generate_predicted_boxes(data_dict["batch_size"], pred_dicts)
            if self.training:
                data_dict["pred_box_dicts"] = boxes  # (the reference re-orders them into `rois` for a second stage: not built)
            else:
                data_dict["final_box_dicts"] = boxes
        return data_dict
