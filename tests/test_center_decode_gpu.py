"""CenterHead's padded inference path on the MI355X (csrc/center_decode.hip, csrc/nms_bev_batched.hip) against its numpy
statement (tests/center_decode_ref.py): selection at every size where the kernels change path, the map families that break
a top-K (ties across the K-th place, a constant map, signed zeros, NaN), the filters, the batched NMS against
oracle.nms_ref, head-major append, the golden reference run, the whole detector, no host synchronisation, determinism.

Capacity boundaries of the kernels, each hit by a case below:
  * CD_BLOCK_CELLS = 4096 cells per workgroup of a select pass: N = 4096 (one workgroup), 4097 (two), 80640 (20, the last
    one partial);
  * CD_THREADS = 256 ranks per compaction chunk of k_cd_decode: K' = 256, 257;
  * the bitonic sort's power-of-two padding: K' = 1, 63, 64, 65, 500 (512), 512, 513, 4096 (the limit, no padding);
  * k_nmsb_mask / k_nmsb_walk: 64 columns per mask word and 16 rows in flight: n = 0, 1, 63, 64, 65, 500, 4096 (the limit:
    64 words, one per lane)."""
import json
import os

import numpy as np
import pytest
import torch

from mssvt_amd import _lib, center_head, iou3d_nms_utils, synthetic
from oracle import nms_ref
from tests import center_decode_ref as ref
from tests.test_detector_gpu import _random_boxes

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = np.float32
K_LIMIT = center_head.CENTER_DECODE_MAX_K
GEOM = dict(point_cloud_range=[-30.0, -20.0, -2.0], voxel_size=[0.32, 0.3, 6.0], feature_map_stride=2)
WIDE = [-1e6, -1e6, -1e6, 1e6, 1e7, 1e8]


def make_hm(family, rng, B, C, H, W):
    n = C * H * W
    if family == "distinct":  # the spacing keeps float32 sigmoids distinct
        hm = np.stack([rng.permutation(np.linspace(-5, 5, n)) for _ in range(B)])
    elif family == "ties":  # multiples of 0.5: ties straddle the K-th place
        hm = np.round(rng.normal(0, 1.5, (B, n)) * 2) / 2
    elif family == "constant":  # the untrained head
        hm = np.full((B, n), -2.19)
    elif family == "zeros_nan":  # signed zeros compare equal, NaN is never selected
        hm = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0, np.nan, -np.inf]), (B, n))
    else:
        raise ValueError(family)
    return hm.astype(F).reshape(B, C, H, W)


def make_maps(family, seed, B, C, H, W, V):
    """One head's maps; center_z holds the cell's own index (exact in float32), so an equal z pins the selected cell."""
    rng = np.random.default_rng(seed)
    pd = ref.random_heads(rng, B, [C], H, W, V, hm=[make_hm(family, rng, B, C, H, W)])[0]
    pd["center_z"] = np.broadcast_to(np.arange(H * W, dtype=F).reshape(1, 1, H, W), (B, 1, H, W)).copy()
    return pd


def limits_for(H, W):
    """the first column / row and the last quarter of the cells (by index, through z) fall outside; no bound on a centre"""
    return [-29.0, -19.5, -0.5, 1e6, 1e6, 0.75 * H * W + 0.4]


def score_thresh_for(family, n):
    """a threshold that some selected cells pass and some miss, and that no score sits on: for the distinct maps the
    sigmoid of the midpoint between two neighbouring logits of the linspace (half a step is > 2.5e-4 in score up to
    N = 4097; at N = 80640 only logits above 4.4 are selected)"""
    if family != "distinct":
        return {"ties": 0.1, "constant": 0.1, "zeros_nan": 0.4}[family]
    if n < 2:
        return 0.3
    vals = np.linspace(-5, 5, n)
    i = min(int(0.4 * n), n - 2)
    return float(1.0 / (1.0 + np.exp(-0.5 * (vals[i] + vals[i + 1]))))


def run_decode(pd, K, score_thresh, limit):
    t = {k: torch.from_numpy(v).to(DEV) for k, v in pd.items()}
    out = center_head.center_decode(t["hm"], t["center"], t["center_z"], t["dim"], t["rot"], t.get("vel"), K=K,
                                    score_thresh=score_thresh, post_center_limit_range=limit, **GEOM)
    return [o.cpu().numpy() for o in out]


def check_decode(pd, K, score_thresh, limit, need_margin=True):
    boxes, scores, labels, num = run_decode(pd, K, score_thresh, limit)
    B = pd["hm"].shape[0]
    V = pd["vel"].shape[1] if "vel" in pd else 0
    assert boxes.shape == (B, K, 7 + V) and scores.shape == (B, K) and labels.shape == (B, K) and num.shape == (B,)
    assert boxes.dtype == F and scores.dtype == F and labels.dtype == np.int32 and num.dtype == np.int32
    counts = []
    for b in range(B):
        want = ref.decode(pd["hm"][b], pd["center"][b], pd["center_z"][b], pd["dim"][b], pd["rot"][b],
                          pd["vel"][b] if V else None, K, GEOM["feature_map_stride"], GEOM["voxel_size"],
                          GEOM["point_cloud_range"], limit, score_thresh)
        if need_margin:
            assert want["margin"] > 1e-4, want["margin"]  # the inputs sit on no filter bound: nothing passes by luck
        n = want["boxes"].shape[0]
        print("sample %d: %d selected, %d survive, margin %.3g" % (b, want["selected"].size, n, want["margin"]))
        assert int(num[b]) == n
        np.testing.assert_array_equal(labels[b, :n], want["labels"])
        ref.assert_rows_close(boxes[b, :n], scores[b, :n], want["boxes"], want["scores"])  # z (the cell), vel: equal
        assert not boxes[b, n:].any() and not scores[b, n:].any() and not labels[b, n:].any()  # the tails are zero
        counts.append(n)
    return counts


# (C, H, W, K, B, V): N = C H W
SHAPES = [
    (1, 1, 1, 1, 1, 0),        # N = 1
    (1, 1, 1, 100, 3, 2),      # N = 1, K > N
    (1, 7, 9, 100, 3, 0),      # N = 63, K > N
    (2, 4, 8, 100, 1, 2),      # N = 64, K > N
    (1, 5, 13, 1, 3, 0),       # N = 65, K = 1
    (1, 5, 13, 64, 1, 0),      # K' = 64 of 65
    (2, 10, 25, 500, 3, 2),    # N = 500 = K
    (3, 1, 167, 500, 1, 0),    # N = 501, K = 500: one cell is left out
    (3, 1, 167, K_LIMIT, 3, 0),  # K = limit > N
    (2, 64, 32, 256, 1, 0),    # N = 4096: one workgroup per pass; K' = 256: one full compaction chunk
    (2, 64, 32, K_LIMIT, 3, 2),  # N = 4096 = K = limit: everything is selected, the sort is full
    (1, 17, 241, 257, 3, 0),   # N = 4097: two workgroups per pass; K' = 257: a second chunk of one
    (1, 17, 241, 513, 1, 2),   # K' = 513: the sort pads to 1024
    (3, 160, 168, 500, 3, 2),  # N = 80640: 20 workgroups per pass
    (3, 160, 168, 100, 1, 0),
    (3, 160, 168, K_LIMIT, 1, 0),  # K = limit < N
]


@pytest.mark.parametrize("family", ["distinct", "ties", "constant", "zeros_nan"])
@pytest.mark.parametrize("C,H,W,K,B,V", SHAPES)
def test_selection_decode_and_filters(family, C, H, W, K, B, V):
    pd = make_maps(family, 1000 + C * H * W + K, B, C, H, W, V)
    check_decode(pd, K, score_thresh_for(family, C * H * W), limits_for(H, W))


@pytest.mark.parametrize("C,H,W,K,B,V", [SHAPES[3], SHAPES[7], SHAPES[11], SHAPES[13]])
def test_constant_map_selects_the_first_flat_indices(C, H, W, K, B, V):
    pd = make_maps("constant", 7, B, C, H, W, V)
    boxes, scores, labels, num = run_decode(pd, K, 0.1, WIDE)
    kk = min(K, C * H * W)
    for b in range(B):
        assert int(num[b]) == kk
        np.testing.assert_array_equal(labels[b, :kk].astype(np.int64) * (H * W) + boxes[b, :kk, 2].astype(np.int64), np.arange(kk))


@pytest.mark.parametrize("C,H,W,K,B,V", [SHAPES[6], SHAPES[11], SHAPES[13]])
def test_ties_select_the_multiset_that_topk_selects(C, H, W, K, B, V):
    pd = make_maps("ties", 11, B, C, H, W, V)
    boxes, scores, labels, num = run_decode(pd, K, None, WIDE)  # score_thresh=None: no score filter
    kk = min(K, C * H * W)
    top = torch.topk(torch.from_numpy(pd["hm"]).to(DEV).sigmoid().reshape(B, -1), kk)[0].cpu().numpy()
    for b in range(B):
        assert int(num[b]) == kk
        assert (np.diff(scores[b, :kk]) <= 0).all()  # rank order
        np.testing.assert_allclose(np.sort(scores[b, :kk]), np.sort(top[b]), rtol=0, atol=1e-6)
    check_decode(pd, K, None, WIDE, need_margin=False)  # (nothing to sit on: no threshold, limits far away)


@pytest.mark.parametrize("C,H,W,K,B,V", [SHAPES[2], SHAPES[11], SHAPES[13]])
def test_nothing_survives(C, H, W, K, B, V):
    pd = make_maps("distinct", 13, B, C, H, W, V)
    for thresh, limit in ((0.999, WIDE), (0.1, [1000.0, 1000.0, -1e6, 2000.0, 2000.0, 1e6])):
        boxes, scores, labels, num = run_decode(pd, K, thresh, limit)
        assert not num.any() and not boxes.any() and not scores.any() and not labels.any()
    pd["hm"][:] = np.nan  # nothing but NaN logits: no box either, with or without a threshold
    for thresh in (None, 0.1):
        boxes, scores, labels, num = run_decode(pd, K, thresh, WIDE)
        assert not num.any() and not boxes.any() and not scores.any()


def test_signed_zeros_and_nan_without_a_threshold():
    C, H, W, K, B, V = 2, 9, 37, 300, 3, 2
    pd = make_maps("zeros_nan", 17, B, C, H, W, V)
    check_decode(pd, K, None, limits_for(H, W))
    boxes, scores, labels, num = run_decode(pd, C * H * W, None, WIDE)  # K = N: every non-NaN cell, no NaN cell
    for b in range(B):
        assert int(num[b]) == int((~np.isnan(pd["hm"][b])).sum())
        cells = labels[b, :num[b]].astype(np.int64) * (H * W) + boxes[b, :num[b], 2].astype(np.int64)
        assert not np.isnan(pd["hm"][b].reshape(-1)[cells]).any()


def test_other_dtypes_limits_and_cpu_tensors():
    pd = make_maps("distinct", 19, 1, 1, 5, 13, 0)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in pd.items()}
    a = center_head.center_decode(t["hm"], t["center"], t["center_z"], t["dim"], t["rot"], K=10, score_thresh=0.3,
                                  post_center_limit_range=WIDE, **GEOM)
    d = center_head.center_decode(*(t[k].double() for k in ("hm", "center", "center_z", "dim", "rot")), K=10, score_thresh=0.3,
                                  post_center_limit_range=WIDE, **GEOM)
    for x, y in zip(a, d):
        assert torch.equal(x, y)
    nc = center_head.center_decode(t["hm"].permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), t["center"], t["center_z"],
                                   t["dim"], t["rot"], K=10, score_thresh=0.3, post_center_limit_range=WIDE, **GEOM)
    for x, y in zip(a, nc):
        assert torch.equal(x, y)
    with pytest.raises(_lib.MssvtHipError):
        center_head.center_decode(t["hm"], t["center"], t["center_z"], t["dim"], t["rot"], K=K_LIMIT + 1,
                                  post_center_limit_range=WIDE, **GEOM)
    with pytest.raises(_lib.MssvtHipError):
        center_head.center_decode(t["hm"].cpu(), t["center"], t["center_z"], t["dim"], t["rot"], K=10,
                                  post_center_limit_range=WIDE, **GEOM)
    lib = _lib.lib()
    assert lib.mssvt_center_decode_workspace_bytes(1, 256, 4, 4, 10) == 0 and lib.mssvt_center_decode_workspace_bytes(1, 1, 4096, 4096, 10) == 0
    # an empty batch or K = 0 is no limit violation: empty / zero outputs, nothing launched
    e = center_head.center_decode(*(t[k][:0] for k in ("hm", "center", "center_z", "dim", "rot")), K=10,
                                  post_center_limit_range=WIDE, **GEOM)
    assert [tuple(x.shape) for x in e] == [(0, 10, 7), (0, 10), (0, 10), (0,)]
    z = center_head.center_decode(t["hm"], t["center"], t["center_z"], t["dim"], t["rot"], K=0, post_center_limit_range=WIDE, **GEOM)
    assert [tuple(x.shape) for x in z] == [(1, 0, 7), (1, 0), (1, 0), (1,)] and int(z[3][0]) == 0


# ---- batched NMS -----------------------------------------------------------------------------------------------------
NMS_SEEDS = {0: 0, 1: 21, 63: 22, 64: 23, 65: 24, 500: 29, K_LIMIT: 26}  # n -> seed of its clustered boxes
# Among 4096 clustered boxes some pair always has an IoU within 1e-4 of 0.1 or 0.7 (tens of thousands of overlapping
# pairs).  The later box (in score order) of each such pair of seed 26 -- every pair within 2e-4, either measure -- is set
# apart on a row of its own at y = 500, where it overlaps nothing; after that the set's margin is 2.06e-4 for both measures
# (found and checked with near_pair_iou_margin, CPU arithmetic only, about ten seconds per measure: not repeated per run).
NMS_SET_APART = [354, 1242, 1271, 1383, 1458, 1601, 1687, 1760, 2058, 2120, 2251, 2623, 2633, 2983, 3090, 3248, 3405, 3409,
                 3458, 3484, 3670, 3690, 3780, 3910, 3958, 3960, 4080]
_NMS_CACHE = {}


def nms_sample(n):
    """(boxes (n, 9) in descending score order with two velocity columns, scores, labels 0..1)"""
    if n not in _NMS_CACHE:
        boxes, scores = _random_boxes(n, NMS_SEEDS[n], spread=75.0 if n > 1000 else 20.0)
        order = np.argsort(-scores.astype(np.float64), kind="stable")
        rng = np.random.default_rng(n)
        full = np.concatenate([boxes[order], rng.normal(0, 1, (n, 2)).astype(F)], 1)
        if n == K_LIMIT:
            for k, j in enumerate(NMS_SET_APART):
                full[j, 0], full[j, 1] = 500.0 + 10.0 * k, 500.0
        _NMS_CACHE[n] = (full, scores[order], rng.integers(0, 2, n).astype(np.int32), {})
    return _NMS_CACHE[n]


def near_pair_iou_margin(boxes, normal, thresholds):
    """smallest |IoU - t| over the pairs that can overlap at all (the others have IoU 0, away from every t > 0)"""
    b = boxes[:, :7].astype(F)
    x, y = b[:, 0].astype(np.float64), b[:, 1].astype(np.float64)
    reach = 0.5 * np.hypot(b[:, 3].astype(np.float64), b[:, 4].astype(np.float64)) + 0.02
    best = min(thresholds)
    for i in range(b.shape[0] - 1):
        near = np.flatnonzero(np.hypot(x[i + 1:] - x[i], y[i + 1:] - y[i]) <= reach[i] + reach[i + 1:]) + i + 1
        for j in near:
            if normal:
                v = float(nms_normal_iou(b[i], b[j]))
            else:
                v = float(nms_ref.iou_bev(b[i], b[j]))
            best = min(best, min(abs(v - t) for t in thresholds))
    return best


def nms_normal_iou(a, b):
    left, right = max(a[0] - a[3] / F(2), b[0] - b[3] / F(2)), min(a[0] + a[3] / F(2), b[0] + b[3] / F(2))
    top, bottom = max(a[1] - a[4] / F(2), b[1] - b[4] / F(2)), min(a[1] + a[4] / F(2), b[1] + b[4] / F(2))
    inter = max(right - left, F(0)) * max(bottom - top, F(0))
    return inter / max(a[3] * a[4] + b[3] * b[4] - inter, nms_ref.EPS)


def oracle_keep(n, thresh, pre_max, post_max, normal):
    full, _, _, cache = nms_sample(n)
    key = (thresh, pre_max, normal)
    if key not in cache:
        cache[key] = ref.nms_rows(full, thresh, pre_max, 1 << 30, normal, walk=None if normal else nms_ref.nms_sparse)
    return cache[key][:post_max]


def pad_batch(ns, K):
    B = len(ns)
    boxes, scores = np.zeros((B, K, 9), F), np.zeros((B, K), F)
    labels, num = np.zeros((B, K), np.int32), np.array(ns, np.int32)
    for b, n in enumerate(ns):
        full, sc, lb, _ = nms_sample(n)
        boxes[b, :n], scores[b, :n], labels[b, :n] = full, sc, lb
    return boxes, scores, labels, num


@pytest.mark.parametrize("normal", [False, True])
@pytest.mark.parametrize("thresh", [0.1, 0.7])
@pytest.mark.parametrize("ns,K,pre_max,post_max", [
    ([500, 0, 63, 1, 65, 64], 500, 1000, 1000),   # everything meets, everything kept is written
    ([65, 500, 64, 0, 1, 63], 500, 300, 40),      # pre_max < n, post_max < kept
    ([500, K_LIMIT, 0, 65], K_LIMIT, K_LIMIT, 500),  # the limit beside short lists: post_max < kept
])
def test_batched_nms_keeps_what_the_oracle_keeps(ns, K, pre_max, post_max, thresh, normal):
    boxes, scores, labels, num = pad_batch(ns, K)
    class_map = torch.tensor([2, 0], dtype=torch.int64, device=DEV)
    out = iou3d_nms_utils.nms_padded(*(torch.from_numpy(a).to(DEV) for a in (boxes, scores, labels, num)), class_map,
                                     thresh, pre_max, post_max, normal=normal)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    P = post_max
    assert got["pred_boxes"].shape == (len(ns), P, 9) and got["pred_labels"].dtype == np.int64 and got["num"].dtype == np.int32
    for b, n in enumerate(ns):
        keep = oracle_keep(n, thresh, pre_max, post_max, normal)
        print("n=%d: %d kept" % (n, keep.size))
        assert int(got["num"][b]) == keep.size
        np.testing.assert_array_equal(got["pred_boxes"][b, :keep.size], boxes[b, keep])
        np.testing.assert_array_equal(got["pred_scores"][b, :keep.size], scores[b, keep])
        np.testing.assert_array_equal(got["pred_labels"][b, :keep.size], np.array([2, 0])[labels[b, keep]] + 1)
        assert not got["pred_boxes"][b, keep.size:].any() and not got["pred_scores"][b, keep.size:].any() and \
            not got["pred_labels"][b, keep.size:].any()


def test_batched_nms_against_the_plain_walk():
    """the oracle above skips pairs that cannot overlap, as the kernel does with a margin of its own; here the first 160
    rows of the 500-box set against nms_ref.nms, which evaluates EVERY pair (the whole set, 125 000 pairs of the Python
    oracle, is held to nms_ref.nms in tests/test_center_decode_ref_cpu.py)"""
    boxes, scores, labels, num = pad_batch([500], 500)
    for thresh in (0.1, 0.7):
        keep = ref.nms_rows(boxes[0], thresh, 160, 1000, walk=nms_ref.nms)
        out = iou3d_nms_utils.nms_padded(*(torch.from_numpy(a).to(DEV) for a in (boxes, scores, labels, num)),
                                         torch.tensor([0, 1], dtype=torch.int64, device=DEV), thresh, 160, 1000)
        assert int(out["num"][0]) == keep.size
        np.testing.assert_array_equal(out["pred_boxes"][0, :keep.size].cpu().numpy(), boxes[0, keep])


@pytest.mark.parametrize("n", [63, 64, 65, 500])
def test_nms_inputs_sit_on_no_threshold(n):
    """the seeds above are fixed so that no pair's oracle IoU lies within 1e-4 of a threshold (CPU arithmetic only; for the
    4096-box set: tests/test_center_decode_ref_cpu.py)"""
    full = nms_sample(n)[0]
    assert near_pair_iou_margin(full, False, (0.1, 0.7)) > 1e-4
    assert near_pair_iou_margin(full, True, (0.1, 0.7)) > 1e-4


# ---- heads: class maps, head-major append, the list path --------------------------------------------------------------
def golden(golden_dir):
    d = np.load(os.path.join(golden_dir, "det_bev_head.npz"))
    return d, json.loads(str(d["cfg_json"]))


def make_head(cfg, names_each_head, V, nms_type, K, pre_max, post_max, nms_thresh, score_thresh, limit):
    from mssvt_amd.center_head import CenterHead
    from mssvt_amd.config import Config
    hc = json.loads(json.dumps(cfg["HEAD"]))
    hc["CLASS_NAMES_EACH_HEAD"] = names_each_head
    hc["TARGET_ASSIGNER_CONFIG"]["FEATURE_MAP_STRIDE"] = GEOM["feature_map_stride"]
    hc["POST_PROCESSING"].update(MAX_OBJ_PER_SAMPLE=K, SCORE_THRESH=score_thresh, POST_CENTER_LIMIT_RANGE=limit)
    hc["POST_PROCESSING"]["NMS_CONFIG"].update(NMS_TYPE=nms_type, NMS_THRESH=nms_thresh, NMS_PRE_MAXSIZE=pre_max,
                                               NMS_POST_MAXSIZE=post_max)
    if V:
        hc["SEPARATE_HEAD_CFG"]["HEAD_ORDER"].append("vel")
        hc["SEPARATE_HEAD_CFG"]["HEAD_DICT"]["vel"] = dict(out_channels=V, num_conv=2)
    return CenterHead(Config.wrap(hc), 8, len(cfg["CLASSES"]), cfg["CLASSES"], np.array(cfg["GRID"]),
                      np.array(GEOM["point_cloud_range"] + [30.0, 20.0, 4.0]), GEOM["voxel_size"],
                      predict_boxes_when_training=False).eval().to(DEV)


HEADS2 = [["Pedestrian"], ["Vehicle", "Cyclist"]]
HEADS3 = [["Cyclist"], ["Vehicle"], ["Pedestrian"]]
HEADS_2_1 = [["Vehicle", "Cyclist"], ["Pedestrian"]]


@pytest.mark.parametrize("names,V,nms_type,H,W,K,pre_max,post_max,seed", [  # seeds: no score / centre on a filter bound
    (HEADS2, 2, "nms_gpu", 13, 21, 100, 70, 12, 31),
    (HEADS3, 0, "nms_normal_gpu", 7, 37, 64, 1000, 1000, 31),
    (HEADS2, 0, "nms_gpu", 160, 168, 500, 300, 40, 31),
    (HEADS2, 0, "nms_gpu", 17, 241, 257, 1000, 1000, 33),   # head 0: N = 4097 (two workgroups per pass), K' = 257
    (HEADS_2_1, 2, "nms_gpu", 64, 32, 256, 1000, 1000, 31),  # head 0: N = 4096 (one workgroup per pass), K' = 256
])
def test_heads_append_head_major_and_equal_the_list_path(golden_dir, names, V, nms_type, H, W, K, pre_max, post_max, seed):
    _, cfg = golden(golden_dir)
    limit = [-29.0, -19.5, -0.8, 1e6, 1e6, 0.9]
    head = make_head(cfg, names, V, nms_type, K, pre_max, post_max, 0.2, 0.3, limit)
    B = 3
    heads = ref.random_heads(np.random.default_rng(seed), B, [len(n) for n in names], H, W, V)  # distinct logits
    dev_heads = [{k: torch.from_numpy(v).to(DEV) for k, v in pd.items()} for pd in heads]
    padded = head.generate_predicted_boxes_padded(B, dev_heads)
    P = len(names) * post_max
    assert padded["pred_boxes"].shape == (B, P, 7 + V) and padded["pred_boxes"].dtype == torch.float32
    assert padded["pred_scores"].shape == (B, P) and padded["pred_scores"].dtype == torch.float32
    assert padded["pred_labels"].shape == (B, P) and padded["pred_labels"].dtype == torch.int64
    assert padded["num"].shape == (B,) and padded["num"].dtype == torch.int32
    got = center_head.unpad(padded)
    listed = head.generate_predicted_boxes(B, dev_heads)  # the existing path on the device: row for row
    want = ref.head_major(heads, [m.numpy() for m in head._class_maps], K, GEOM["feature_map_stride"], GEOM["voxel_size"],
                          GEOM["point_cloud_range"], limit, 0.3, 0.2, pre_max, post_max, normal=nms_type == "nms_normal_gpu")
    for b in range(B):
        assert want[b]["margin"] > 1e-4
        n = want[b]["pred_boxes"].shape[0]
        assert 0 < n == int(padded["num"][b]) <= P
        ref.assert_rows_close(got[b]["pred_boxes"].cpu().numpy(), got[b]["pred_scores"].cpu().numpy(), want[b]["pred_boxes"],
                              want[b]["pred_scores"])
        np.testing.assert_array_equal(got[b]["pred_labels"].cpu().numpy(), want[b]["pred_labels"])
        ref.assert_rows_close(got[b]["pred_boxes"].cpu().numpy(), got[b]["pred_scores"].cpu().numpy(),
                              listed[b]["pred_boxes"].cpu().numpy(), listed[b]["pred_scores"].cpu().numpy())
        assert torch.equal(got[b]["pred_labels"], listed[b]["pred_labels"])
        assert not padded["pred_boxes"][b, n:].any() and not padded["pred_scores"][b, n:].any() and \
            not padded["pred_labels"][b, n:].any()


def test_what_the_padded_path_does_not_cover_is_refused(golden_dir):
    _, cfg = golden(golden_dir)
    heads = ref.random_heads(np.random.default_rng(3), 1, [1, 2], 5, 13)
    dev_heads = [{k: torch.from_numpy(v).to(DEV) for k, v in pd.items()} for pd in heads]
    for kw, word in ((dict(nms_thresh=[0.2, 0.3]), "per-class"), (dict(nms_type="circle_nms"), "NMS_TYPE"),
                     (dict(K=K_LIMIT + 1), "MAX_OBJ_PER_SAMPLE")):
        args = dict(nms_type="nms_gpu", K=50, nms_thresh=0.2)
        args.update(kw)
        head = make_head(cfg, HEADS2, 0, args["nms_type"], args["K"], 100, 10, args["nms_thresh"], 0.1, WIDE)
        with pytest.raises(_lib.MssvtHipError, match=word):
            head.generate_predicted_boxes_padded(1, dev_heads)
    head = make_head(cfg, HEADS2, 0, "nms_gpu", 50, 100, 10, [0.2], 0.1, WIDE)  # a one-entry list is one threshold
    head.generate_predicted_boxes_padded(1, dev_heads)
    head.nms_fn = lambda *a, **k: None
    with pytest.raises(_lib.MssvtHipError, match="nms_fn"):
        head.generate_predicted_boxes_padded(1, dev_heads)


# ---- end to end -------------------------------------------------------------------------------------------------------
def test_golden_reference_run_through_the_padded_path(golden_dir):
    from tests.test_detector_cpu import build_from_golden
    d, _, head = build_from_golden(golden_dir)
    head = head.to(DEV)
    head.padded_predictions = True
    with torch.no_grad():
        res = head(dict(spatial_features_2d=torch.from_numpy(d["spatial_features_2d"]).to(DEV), batch_size=int(d["batch_size"])))
    assert "final_box_dicts" not in res
    finals = center_head.unpad(res["final_box_padded"])
    for b in range(int(d["batch_size"])):
        got = finals[b]
        want_boxes, want_scores = d["final%d.pred_boxes" % b], d["final%d.pred_scores" % b]
        assert got["pred_boxes"].shape == want_boxes.shape
        np.testing.assert_allclose(got["pred_scores"].cpu().numpy(), want_scores, rtol=1e-4, atol=5e-5)
        rows = lambda bx, lb: np.concatenate([bx, lb[:, None].astype(np.float32)], 1)  # noqa: E731
        g = rows(got["pred_boxes"].cpu().numpy(), got["pred_labels"].cpu().numpy())
        w = rows(want_boxes, d["final%d.pred_labels" % b])
        g, w = g[np.lexsort((g[:, 1], g[:, 0]))], w[np.lexsort((w[:, 1], w[:, 0]))]
        np.testing.assert_allclose(g, w, rtol=1e-4, atol=1e-4)


@pytest.fixture(scope="module")
def padded_detector():
    """mssvt.yaml's CenterPoint with padded_predictions on, built once for the two tests below"""
    from mssvt_amd import centerpoint
    torch.manual_seed(0)
    det = centerpoint.build_detector().to(DEV).eval()
    with torch.no_grad():
        for h in det.dense_head.heads_list:  # random init: lift the heat map above the score threshold
            h.hm[-1].bias.fill_(0.5)
    det.dense_head.padded_predictions = True
    return det


def test_centerpoint_detector_with_padded_predictions(padded_detector):
    from mssvt_amd import centerpoint
    det = padded_detector
    B = 2
    pts = torch.from_numpy(synthetic.make_batch_points(20000, B, 123)).to(DEV)
    rng = np.random.default_rng(5)
    gt = np.zeros((B, 6, 8), np.float32)
    gt[:, :4, 0:2] = rng.uniform(-40, 40, (B, 4, 2))
    gt[:, :4, 3:6] = rng.uniform([1.5, 0.8, 1.0], [5.0, 2.5, 2.0], (B, 4, 3))
    gt[:, :4, 6] = rng.uniform(-3, 3, (B, 4))
    gt[:, :4, 7] = rng.integers(1, 4, (B, 4))
    batch = dict(points=pts, batch_size=B, gt_boxes=torch.from_numpy(gt).to(DEV))
    with torch.no_grad():
        preds, recall = det(batch)
    post = det.dense_head.model_cfg.POST_PROCESSING
    P = len(det.dense_head.heads_list) * int(post.NMS_CONFIG.NMS_POST_MAXSIZE)
    assert isinstance(preds, list) and len(preds) == B
    want_recall = {}
    for b, p in enumerate(preds):
        n = p["pred_boxes"].shape[0]
        assert 0 < n <= P and p["pred_boxes"].shape == (n, 7) and p["pred_scores"].shape == (n,) and p["pred_labels"].shape == (n,)
        assert p["pred_boxes"].dtype == torch.float32 and p["pred_scores"].dtype == torch.float32 and p["pred_labels"].dtype == torch.int64
        assert int(p["pred_labels"].min()) >= 1 and int(p["pred_labels"].max()) <= 3
        assert bool((p["pred_scores"] > float(post.SCORE_THRESH)).all())
        assert bool((p["pred_scores"][:-1] >= p["pred_scores"][1:]).all())  # one head: non-increasing throughout
        want_recall = centerpoint.CenterPoint.generate_recall_record(
            p["pred_boxes"], want_recall, b, batch, det.model_cfg.POST_PROCESSING.RECALL_THRESH_LIST)
    assert recall == want_recall and recall["gt"] == B * 4


# ---- no host synchronisation, determinism, streams ---------------------------------------------------------------------
def small_head_and_maps(golden_dir, family="ties"):
    _, cfg = golden(golden_dir)
    head = make_head(cfg, HEADS2, 2, "nms_gpu", 300, 200, 50, 0.2, 0.1, [-29.0, -19.5, -0.8, 1e6, 1e6, 0.9])
    B, H, W = 3, 40, 53
    rng = np.random.default_rng(41)
    heads = ref.random_heads(rng, B, [1, 2], H, W, 2, hm=[make_hm(family, rng, B, c, H, W) for c in (1, 2)])
    return head, B, [{k: torch.from_numpy(v).to(DEV) for k, v in pd.items()} for pd in heads]


def test_padded_path_never_synchronises_the_host(golden_dir):
    head, B, dev_heads = small_head_and_maps(golden_dir)
    warm = head.generate_predicted_boxes_padded(B, dev_heads)  # class maps reach the device here, once
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe = torch.ones(1, device=DEV)
        try:
            probe.item()
            live = False
        except RuntimeError:
            live = True
        if live:
            out = head.generate_predicted_boxes_padded(B, dev_heads)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    for k in warm:
        assert torch.equal(warm[k], out[k]), k
    lists = center_head.unpad(out)  # outside the mode: one read-back
    listed = head.generate_predicted_boxes(B, dev_heads)  # the list path is unaffected
    assert len(lists) == len(listed) == B
    for a, b in zip(lists, listed):
        assert a["pred_boxes"].shape == b["pred_boxes"].shape and a["pred_labels"].dtype == b["pred_labels"].dtype


def test_tied_map_is_bit_identical_run_to_run_and_across_streams(golden_dir):
    head, B, dev_heads = small_head_and_maps(golden_dir)
    first = head.generate_predicted_boxes_padded(B, dev_heads)
    second = head.generate_predicted_boxes_padded(B, dev_heads)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for s in streams:  # both in flight together: each call owns its workspace
        with torch.cuda.stream(s):
            outs.append(head.generate_predicted_boxes_padded(B, dev_heads))
    torch.cuda.synchronize()
    assert int(first["num"].sum()) > 0
    for other in [second] + outs:
        for k in first:
            assert torch.equal(first[k], other[k]), k


def test_head_as_the_pipeline_post_stage_hands_the_padded_dict_over(padded_detector):
    """FramePipeline(backbone, pre=vfe, post=BEV + head) with padded_predictions: the head runs on each frame's own stream,
    `get()` hands the nested `final_box_padded` tensors over to the consumer's stream; every frame equals the frame run alone."""
    from mssvt_amd.pipeline import FramePipeline
    det = padded_detector

    def post(bd):
        for m in (det.map_to_bev_module, det.backbone_2d, det.dense_head):
            bd = m(bd)
        return bd
    clouds = [torch.from_numpy(synthetic.make_batch_points(20000, 1, 60 + f)).to(DEV) for f in range(3)]
    with torch.no_grad():
        alone = [{k: v.clone() for k, v in post(det.backbone_3d(det.vfe(dict(points=c, batch_size=1))))["final_box_padded"].items()}
                 for c in clouds]
    torch.cuda.synchronize()
    pipe = FramePipeline(det.backbone_3d, depth=3, pre=det.vfe, post=post)
    frames = [pipe(dict(points=clouds[i % 3], batch_size=1)) for i in range(6)]
    for i in reversed(range(6)):
        got = frames[i].get()["final_box_padded"]
        assert int(alone[i % 3]["num"][0]) > 0
        for k in alone[i % 3]:
            assert torch.equal(got[k], alone[i % 3][k]), (i, k)
        lists = center_head.unpad(got)
        assert len(lists) == 1 and lists[0]["pred_boxes"].shape[0] == int(got["num"][0])
    pipe.close()
