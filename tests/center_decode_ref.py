"""numpy statement of CenterHead's padded inference path (TEST INFRASTRUCTURE ONLY): what csrc/center_decode.hip and
csrc/nms_bev_batched.hip compute, per sample, in float32.

* ``select``: the cells of one sample ranked by (logit descending, flat index ascending), -0.0 == +0.0, NaN last; the
  first min(K, N).
* ``decode``: score / box of the selected cells in rank order with one rounded float32 operation per step, the
  centre-range (inclusive) and score (strict) filters, survivors in rank order; also the distance of every selected
  cell's score / centre to the filter bounds (``margin``), so a test can refuse inputs that sit on a bound.
* ``nms_rows``: the greedy walk of oracle.nms_ref over rows that are already in rank order.
* ``head_major``: decode + NMS per head, appended head after head, labels through the class maps (1-based).
"""
import numpy as np

from oracle import nms_ref

F = np.float32


def select(hm, K):
    """hm (C, H, W) of one sample -> (flat indices of the first min(K, N) cells in rank order, how many of them are NaN)."""
    flat = np.asarray(hm, F).reshape(-1)
    nan = np.isnan(flat)
    val = np.where(nan, F(-np.inf), flat)
    val = np.where(val == 0, F(0.0), val)  # -0.0 and +0.0: the index decides
    order = np.lexsort((np.arange(flat.size), -val.astype(np.float64), nan))  # last key first: NaN last, logit, index
    order = order[:min(int(K), flat.size)]
    return order, int(nan[order].sum())


def decode(hm, center, center_z, dim, rot, vel, K, stride, voxel_size, pc_range, limit, score_thresh):
    """One sample: hm (C, H, W), center (2, H, W), center_z (1, H, W), dim (3, H, W), rot (2, H, W), vel (V, H, W) or
    None -> dict(boxes (n, 7 + V), scores (n), labels (n) int32, cells (n) flat indices, selected (K') flat indices,
    margin: the smallest distance of a selected non-NaN cell's score to the threshold / of its centre to a limit)."""
    C, H, W = hm.shape
    order, _ = select(hm, K)
    logit = np.asarray(hm, F).reshape(-1)[order]
    live = ~np.isnan(logit)
    cls = (order // (H * W)).astype(np.int32)
    cell = order % (H * W)
    ys, xs = (cell // W).astype(F), (cell % W).astype(F)
    pick = lambda t: np.asarray(t, F).reshape(t.shape[0], H * W)[:, cell]  # noqa: E731  (c, K')
    ctr, cz, dm, rt = pick(center), pick(center_z), pick(dim), pick(rot)
    with np.errstate(all="ignore"):
        score = (F(1.0) / (F(1.0) + np.exp(-logit, dtype=F))).astype(F)
        x = (((xs + ctr[0]).astype(F) * F(stride)).astype(F) * F(voxel_size[0])).astype(F) + F(pc_range[0])
        y = (((ys + ctr[1]).astype(F) * F(stride)).astype(F) * F(voxel_size[1])).astype(F) + F(pc_range[1])
        cols = [x.astype(F), y.astype(F), cz[0], np.exp(dm[0], dtype=F), np.exp(dm[1], dtype=F), np.exp(dm[2], dtype=F),
                np.arctan2(rt[1], rt[0], dtype=F)]
        if vel is not None:
            cols += list(pick(vel))
        boxes = np.stack(cols, axis=1).astype(F)
        lim = np.asarray(limit, F)
        ok = live & (boxes[:, :3] >= lim[:3]).all(1) & (boxes[:, :3] <= lim[3:]).all(1)
        margin = np.inf
        if live.any():
            margin = float(np.abs(boxes[live, :3].astype(np.float64)[:, None, :] -
                                  lim.astype(np.float64).reshape(2, 3)[None]).min())
        if score_thresh is not None:
            ok &= score > F(score_thresh)
            if live.any():
                margin = min(margin, float(np.abs(score[live].astype(np.float64) - float(F(score_thresh))).min()))
    return dict(boxes=boxes[ok], scores=score[ok], labels=cls[ok], cells=order[ok], selected=order, margin=margin)


def nms_rows(boxes, thresh, pre_max, post_max, normal=False, walk=None):
    """Rows already in rank order -> the positions greedy NMS keeps among the first pre_max, the first post_max of them.
    `walk`: another oracle of the same walk.  The rotated walk is nms_ref.nms_sparse (nms's result without the pairs that
    cannot overlap) for a positive threshold."""
    n = min(boxes.shape[0], int(pre_max))
    if n == 0:
        return np.zeros(0, np.int64)
    rank = np.arange(n, 0, -1).astype(np.float64)  # strictly descending: the walk follows the row order
    fn = walk or (nms_ref.nms_normal if normal else (nms_ref.nms_sparse if thresh > 0 else nms_ref.nms))
    keep = fn(np.ascontiguousarray(boxes[:n, :7], F), rank, float(thresh))
    return np.asarray(keep, np.int64)[:int(post_max)]


def head_major(heads, class_maps, K, stride, voxel_size, pc_range, limit, score_thresh, nms_thresh, pre_max, post_max,
               normal=False):
    """heads: per head a dict of (B, c, H, W) arrays (hm, center, center_z, dim, rot[, vel]); class_maps: per head the
    0-based index into class_names of each class inside the head.  -> per sample dict(pred_boxes, pred_scores, pred_labels
    (1-based, int64), margin), heads appended one after another."""
    B = heads[0]["hm"].shape[0]
    out = []
    for b in range(B):
        bx, sc, lb, margin = [], [], [], np.inf
        for h, pd in enumerate(heads):
            d = decode(pd["hm"][b], pd["center"][b], pd["center_z"][b], pd["dim"][b], pd["rot"][b],
                       pd["vel"][b] if "vel" in pd else None, K, stride, voxel_size, pc_range, limit, score_thresh)
            keep = nms_rows(d["boxes"], nms_thresh, pre_max, post_max, normal)
            bx.append(d["boxes"][keep]); sc.append(d["scores"][keep])
            lb.append(np.asarray(class_maps[h], np.int64)[d["labels"][keep]] + 1)
            margin = min(margin, d["margin"])
        out.append(dict(pred_boxes=np.concatenate(bx, 0), pred_scores=np.concatenate(sc, 0),
                        pred_labels=np.concatenate(lb, 0), margin=margin))
    return out


def assert_rows_close(got_boxes, got_scores, want_boxes, want_scores):
    """Row for row, at the derived tolerances: x, y atol 1.6e-5 (two float32 ulps below 128), z and velocities equal,
    sizes rtol 2e-6, heading and scores atol 1e-6 (device versus host library functions)."""
    got_boxes, want_boxes = np.asarray(got_boxes), np.asarray(want_boxes)
    assert got_boxes.shape == want_boxes.shape, (got_boxes.shape, want_boxes.shape)
    np.testing.assert_allclose(got_boxes[:, 0:2], want_boxes[:, 0:2], rtol=0, atol=1.6e-5)
    np.testing.assert_array_equal(got_boxes[:, 2], want_boxes[:, 2])
    np.testing.assert_allclose(got_boxes[:, 3:6], want_boxes[:, 3:6], rtol=2e-6, atol=0)
    np.testing.assert_allclose(got_boxes[:, 6], want_boxes[:, 6], rtol=0, atol=1e-6)
    np.testing.assert_array_equal(got_boxes[:, 7:], want_boxes[:, 7:])
    np.testing.assert_allclose(np.asarray(got_scores), np.asarray(want_scores), rtol=0, atol=1e-6)


def random_heads(rng, B, channels, H, W, V=0, hm=None):
    """Regression maps of len(channels) heads (centres inside the cell, sizes around 1 m, unit-ish headings); `hm`: per
    head a (B, C, H, W) map, default a random permutation of linspace(-5, 5) per sample (all logits distinct)."""
    heads = []
    for h, C in enumerate(channels):
        n = C * H * W
        m = hm[h] if hm is not None else np.stack([rng.permutation(np.linspace(-5, 5, n)) for _ in range(B)]).reshape(B, C, H, W)
        pd = dict(hm=np.asarray(m, F), center=rng.uniform(0.05, 0.95, (B, 2, H, W)).astype(F),
                  center_z=rng.uniform(-1, 1, (B, 1, H, W)).astype(F), dim=rng.normal(0.3, 0.3, (B, 3, H, W)).astype(F),
                  rot=rng.normal(0, 1, (B, 2, H, W)).astype(F))
        if V:
            pd["vel"] = rng.normal(0, 2, (B, V, H, W)).astype(F)
        heads.append(pd)
    return heads
