"""Rotated-box IoU operators on the MI355X (csrc/box_iou.hip through iou3d_nms_utils): the four pair measures against
oracle/nms_ref.py and numpy restatements of the reference's height / volume arithmetic and iou_normal, the exactness of
the far-pair rejection, shapes / strides / streams, an anchor-scale call, agreement with the existing NMS, nms_normal_gpu,
the pybind stand-ins, and the detector's recall bookkeeping end to end.

Tolerance against the oracle (IoU, absolute; for overlap areas times the pair's union area): kernel and oracle are two
fp32 evaluations of one procedure that differ in sinf / cosf / atan2f and in the division (the library is built with
-ffp-contract=off, so there is no contraction on either side), so each is as far from the exact value as the other.  Each test measures d = max |oracle in float32 - oracle in float64| on its own candidate pairs
and allows 4 d (2 x for two independent roundings of that size, 2 x for pairs worse than the sample's worst), floor 1e-6.
Measured on the MI355X (the tests print these): spread 20 -- d = 1.9e-06 ... 4.0e-06 per seed, the kernel's worst deviation
over modes 0 - 2 8.1e-07 ... 2.2e-06; spread 75 -- d = 5.9e-06 ... 1.1e-05, worst 1.0e-06 ... 4.4e-06; the anchor-scale
sample -- d = 4.4e-06, worst 1.8e-06.  Mode 2 against the torch composition around the kernel's own overlap: 0 (equal bits)."""
import numpy as np
import pytest
import torch

from mssvt_amd import synthetic
from oracle import nms_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP8 = 8 * 2.0 ** -24  # two fp32 evaluations of one formula: a not-correctly-rounded division on each side + one ulp


def boxes(n, rng, spread):
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = rng.uniform(-spread, spread, (n, 2)); b[:, 2] = rng.uniform(-1, 1, n)
    b[:, 3] = rng.uniform(1.5, 5.0, n); b[:, 4] = rng.uniform(0.8, 2.5, n); b[:, 5] = rng.uniform(1.0, 2.0, n)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    return b


def pair_sets(seed, spread, n=160, m=120):       # b = 90 jittered copies of boxes of a + 30 unrelated boxes
    rng = np.random.default_rng(seed); a = boxes(n, rng, spread); k = m * 3 // 4
    j = a[rng.permutation(n)[:k]].copy()
    j[:, 0:2] += rng.normal(0, 0.4, (k, 2)); j[:, 2] += rng.normal(0, 0.2, k)
    j[:, 3:6] *= rng.uniform(0.85, 1.15, (k, 3)); j[:, 6] += rng.normal(0, 0.3, k)
    return a, np.concatenate([j, boxes(m - k, rng, spread)]).astype(np.float32)


def _random_boxes(n, seed, spread=20.0):  # as tests/test_detector_gpu.py
    rng = np.random.default_rng(seed)
    b = boxes(n, rng, spread)
    q = n // 4
    b[q:2 * q] = b[:q] + rng.normal(0, 0.15, (q, 7)).astype(np.float32)
    return b, rng.uniform(0.1, 1.0, n).astype(np.float32)


def candidate_mask(a, b):
    """Pairs whose centres are no further apart than (half-diagonal + 0.02) of a + (half-diagonal + 0.02) of b; every
    other pair is 'far' and must come out as exactly 0.0 in modes 0 - 2."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    ra, rb = 0.5 * np.hypot(a[:, 3], a[:, 4]) + 0.02, 0.5 * np.hypot(b[:, 3], b[:, 4]) + 0.02
    dist = np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1])
    return dist <= ra[:, None] + rb[None, :]


def height_overlap(a, b):  # ref iou3d_nms_utils.py:59-71, float32
    lo = np.maximum((a[:, 2] - a[:, 5] / 2)[:, None], (b[:, 2] - b[:, 5] / 2)[None, :])
    hi = np.minimum((a[:, 2] + a[:, 5] / 2)[:, None], (b[:, 2] + b[:, 5] / 2)[None, :])
    return np.maximum(hi - lo, np.float32(0))


def iou3d_from_overlap(a, b, ov):  # ref iou3d_nms_utils.py:73-79, float32
    ov3 = (ov * height_overlap(a, b)).astype(np.float32)
    va, vb = a[:, 3] * a[:, 4] * a[:, 5], b[:, 3] * b[:, 4] * b[:, 5]
    return ov3 / np.maximum(va[:, None] + vb[None, :] - ov3, np.float32(1e-6))


def iou_normal_np(a, b):  # ref iou3d_nms_kernel.cu:314-325, float32
    left = np.maximum((a[:, 0] - a[:, 3] / 2)[:, None], (b[:, 0] - b[:, 3] / 2)[None, :])
    right = np.minimum((a[:, 0] + a[:, 3] / 2)[:, None], (b[:, 0] + b[:, 3] / 2)[None, :])
    top = np.maximum((a[:, 1] - a[:, 4] / 2)[:, None], (b[:, 1] - b[:, 4] / 2)[None, :])
    bottom = np.minimum((a[:, 1] + a[:, 4] / 2)[:, None], (b[:, 1] + b[:, 4] / 2)[None, :])
    inter = np.maximum(right - left, np.float32(0)) * np.maximum(bottom - top, np.float32(0))
    sa, sb = a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]
    return inter / np.maximum(sa[:, None] + sb[None, :] - inter, np.float32(1e-8))


def torch_iou3d_composition(boxes_a, boxes_b, overlaps_bev):
    """3-D IoU as a torch composition around a given BEV overlap matrix, on the tensors' device: the arithmetic of the
    reference's boxes_iou3d_gpu (iou3d_nms_utils.py:59-79) restated -- the same operations in the same order, so the same
    fp32 roundings: z -+ dz/2, height = clamp(min of tops - max of bottoms, 0), ov3 = ov * height, volumes (dx dy) dz,
    ov3 / clamp((va + vb) - ov3, 1e-6)."""
    def z_range_and_volume(t):
        half = t[:, 5] / 2
        return t[:, 2] - half, t[:, 2] + half, t[:, 3] * t[:, 4] * t[:, 5]

    (lo_a, hi_a, va), (lo_b, hi_b, vb) = z_range_and_volume(boxes_a), z_range_and_volume(boxes_b)
    height = (torch.minimum(hi_a[:, None], hi_b[None, :]) - torch.maximum(lo_a[:, None], lo_b[None, :])).clamp(min=0)
    ov3 = overlaps_bev * height
    return ov3 / (va[:, None] + vb[None, :] - ov3).clamp(min=1e-6)


def oracle_on(a, b, pairs, monkeypatch):
    """(overlap, IoU) of the fp32 oracle on the listed pairs, and d = max |IoU in float32 - IoU in float64|."""
    ov32 = np.array([nms_ref.box_overlap(a[i], b[j]) for i, j in pairs], np.float32)
    iou32 = np.array([nms_ref.iou_bev(a[i], b[j]) for i, j in pairs], np.float32)
    with monkeypatch.context() as mp:
        mp.setattr(nms_ref, "F", np.float64)
        mp.setattr(nms_ref, "EPS", np.float64(1e-8))
        mp.setattr(nms_ref, "MARGIN", np.float64(1e-2))
        iou64 = np.array([nms_ref.iou_bev(a[i], b[j]) for i, j in pairs], np.float64)
    assert nms_ref.F is np.float32
    return ov32, iou32, float(np.abs(iou32.astype(np.float64) - iou64).max())


def all_modes(a, b):
    from mssvt_amd import iou3d_nms_utils as u
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    ov, iou, iou3 = u.boxes_overlap_bev(ta, tb), u.boxes_iou_bev(ta, tb), u.boxes_iou3d_gpu(ta, tb)
    return ta, tb, ov, iou, iou3


def is_zero_bits(x):
    return x.view(np.int32) == 0


def test_known_answers():
    from mssvt_amd import iou3d_nms_utils as u
    t = lambda *rows: torch.tensor(rows, dtype=torch.float32, device=DEV)  # noqa: E731
    a = [0, 0, 0, 4, 2, 1, 0.0]
    assert abs(float(u.boxes_iou_bev(t(a), t(a))[0, 0]) - 1.0) < 1e-6
    assert abs(float(u.boxes_overlap_bev(t(a), t([1, 0, 0, 4, 2, 1, 0.0]))[0, 0]) - 6.0) < 1e-5  # 3 x 2 overlap
    sq, tilted = [0, 0, 0, 2, 2, 1, 0.0], [0, 0, 0, 2, 2, 1, np.pi / 4]
    assert abs(float(u.boxes_overlap_bev(t(tilted), t(sq))[0, 0]) - 8 * (np.sqrt(2) - 1)) < 1e-4  # a regular octagon
    far = [10, 10, 0, 1, 1, 1, 0.3]
    for fn in (u.boxes_overlap_bev, u.boxes_iou_bev, u.boxes_iou3d_gpu):
        assert bool(is_zero_bits(fn(t(a), t(far)).cpu().numpy()).all())
    assert abs(float(u.boxes_iou3d_gpu(t(a), t(a))[0, 0]) - 1.0) < 1e-6
    # half the height shared: 8 * 0.5 of a union of 8 + 8 - 4
    assert abs(float(u.boxes_iou3d_gpu(t(a), t([0, 0, 0.5, 4, 2, 1, 0.0]))[0, 0]) - 1 / 3) < 1e-6
    assert float(u.boxes_iou3d_gpu(t(a), t([0, 0, 30, 4, 2, 1, 0.0]))[0, 0]) == 0.0


@pytest.mark.parametrize("spread,seed", [(s, k) for s in (20.0, 75.0) for k in range(8)])
def test_modes_0_1_2_against_the_oracle(spread, seed, monkeypatch):
    a, b = pair_sets(seed, spread)
    assert a.shape == (160, 7) and b.shape == (120, 7)
    ta, tb, ov_t, iou_t, iou3_t = all_modes(a, b)
    ov, iou, iou3 = ov_t.cpu().numpy(), iou_t.cpu().numpy(), iou3_t.cpu().numpy()
    cand = candidate_mask(a, b)
    for name, m in (("overlap", ov), ("iou_bev", iou), ("iou3d", iou3)):
        assert m.shape == (160, 120) and m.dtype == np.float32
        assert bool(is_zero_bits(m[~cand]).all()), "%s: a far pair is not exactly 0.0" % name
    pairs = np.argwhere(cand)
    want_ov, want_iou, d = oracle_on(a, b, pairs, monkeypatch)
    tol = max(4 * d, 1e-6)
    got_ov, got_iou, got_iou3 = ov[cand], iou[cand], iou3[cand]  # argwhere and boolean indexing share the row-major order
    sa, sb = a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]
    union = (sa[:, None] + sb[None, :])[cand] - want_ov
    err_ov, err_iou = np.abs(got_ov - want_ov) / union, np.abs(got_iou - want_iou)
    want_full = np.zeros_like(ov)
    want_full[cand] = want_ov
    want_iou3 = iou3d_from_overlap(a, b, want_full)[cand]
    err_iou3 = np.abs(got_iou3 - want_iou3)
    # mode 2 against the reference's torch composition around OUR overlap matrix: the same arithmetic, rounding for rounding
    comp = torch_iou3d_composition(ta, tb, ov_t)
    err_comp = float((iou3_t - comp).abs().max())
    print("spread %g seed %d: %d candidates, %d non-zero; d %.3g tol %.3g; worst overlap/union %.3g iou_bev %.3g iou3d %.3g; "
          "iou3d vs torch composition %.3g" % (spread, seed, len(pairs), int((want_iou > 0).sum()), d, tol, err_ov.max(),
                                               err_iou.max(), err_iou3.max(), err_comp))
    assert len(pairs) > 60 and int((want_iou > 0).sum()) > 50
    assert np.array_equal(want_ov == 0, got_ov == 0) and np.array_equal(want_iou == 0, got_iou == 0)
    assert err_ov.max() <= tol, pairs[err_ov.argmax()]
    assert err_iou.max() <= tol, pairs[err_iou.argmax()]
    assert err_iou3.max() <= tol, pairs[err_iou3.argmax()]
    assert err_comp <= ULP8


def greedy_nms(iou, scores, thresh):
    order = np.argsort(-scores.astype(np.float64), kind="stable")
    removed, keep = np.zeros(len(order), bool), []
    for p, i in enumerate(order):
        if removed[p]:
            continue
        keep.append(int(i))
        removed[p + 1:] |= iou[i, order[p + 1:]] > np.float32(thresh)
    return keep


def test_iou_normal_matrix():
    from mssvt_amd import iou3d_nms_utils as u
    a, b = pair_sets(3, 20.0)
    got = u.boxes_pairwise(u.BOX_IOU_NORMAL, torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).cpu().numpy()
    want = iou_normal_np(a, b)
    print("iou_normal: worst deviation %.3g, %d non-zero" % (np.abs(got - want).max(), int((want > 0).sum())))
    assert got.shape == (160, 120) and int((want > 0).sum()) > 90
    assert np.abs(got - want).max() <= ULP8 and np.array_equal(got == 0, want == 0)


@pytest.mark.parametrize("n,thresh,seed", [(1, 0.5, 0), (130, 0.5, 2), (193, 0.25, 4)])
def test_nms_normal_keeps_what_greedy_nms_over_iou_normal_keeps(n, thresh, seed):
    from mssvt_amd import iou3d_nms_utils as u
    bx, scores = _random_boxes(n, seed)
    want = greedy_nms(iou_normal_np(bx, bx), scores, thresh)
    got, none = u.nms_normal_gpu(torch.from_numpy(bx).to(DEV), torch.from_numpy(scores).to(DEV), thresh)
    assert none is None and got.dtype == torch.int64 and got.cpu().numpy().tolist() == want
    if n > 1:
        assert 1 < len(want) < n
    e, _ = u.nms_normal_gpu(torch.zeros((0, 7), device=DEV), torch.zeros(0, device=DEV), thresh)
    assert e.numel() == 0


def test_class_agnostic_nms_resolves_nms_normal_gpu_by_name():
    """A yaml with NMS_TYPE: nms_normal_gpu: center_head.class_agnostic_nms finds the function by name and keeps what the
    greedy numpy NMS over iou_normal keeps among the boxes above the score threshold."""
    from mssvt_amd import center_head
    bx, scores = _random_boxes(193, 4)
    cfg = dict(NMS_TYPE="nms_normal_gpu", NMS_THRESH=0.25, NMS_PRE_MAXSIZE=4096, NMS_POST_MAXSIZE=500)
    sel, sel_scores = center_head.class_agnostic_nms(torch.from_numpy(scores).to(DEV), torch.from_numpy(bx).to(DEV), cfg,
                                                     score_thresh=0.3)
    above = np.flatnonzero(scores >= np.float32(0.3))
    want = above[greedy_nms(iou_normal_np(bx[above], bx[above]), scores[above], 0.25)]
    assert sel.cpu().numpy().tolist() == want.tolist() and 1 < want.size < above.size
    assert np.array_equal(sel_scores.cpu().numpy(), scores[want])


def test_boxes_pairwise_refuses_rows_that_cannot_hold_a_box():
    from mssvt_amd import iou3d_nms_utils as u
    ok = torch.zeros((1, 7), device=DEV)
    for bad in (torch.zeros((1, 5), device=DEV), torch.zeros((3, 6), device=DEV), torch.zeros(7, device=DEV)):
        with pytest.raises(AssertionError):
            u.boxes_pairwise(u.BOX_IOU_BEV, bad, ok)
        with pytest.raises(AssertionError):
            u.boxes_pairwise(u.BOX_IOU_BEV, ok, bad)


@pytest.mark.parametrize("n,m", [(0, 5), (5, 0), (1, 1), (64, 64), (65, 129)])
def test_shapes(n, m):
    from mssvt_amd import iou3d_nms_utils as u
    rng = np.random.default_rng(n * 1000 + m)
    a, b = boxes(n, rng, 6.0), boxes(m, rng, 6.0)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    for fn in (u.boxes_overlap_bev, u.boxes_iou_bev, u.boxes_iou3d_gpu):
        out = fn(ta, tb)
        assert out.shape == (n, m) and out.dtype == torch.float32 and out.device.type == "cuda"
    if n and m:
        iou = u.boxes_iou_bev(ta, tb).cpu().numpy()
        picks = [(0, 0), (n - 1, m - 1), (n // 2, m - 1), (n - 1, m // 2)]
        for i, j in picks:  # the corners of the matrix: the last partial tile included
            # 4 d of the spread-20 sets (d <= 4.0e-6 there, the coordinates here are smaller)
            assert abs(float(iou[i, j]) - float(nms_ref.iou_bev(a[i], b[j]))) <= 1.6e-5
        assert np.abs(u.boxes_pairwise(u.BOX_IOU_NORMAL, ta, tb).cpu().numpy() - iou_normal_np(a, b)).max() <= ULP8
        assert bool(torch.isfinite(u.boxes_iou3d_gpu(ta, tb)).all())
        if n * m >= 4096:
            assert (iou > 0).sum() > 0


def test_strided_rows_repeat_calls_and_side_stream():
    from mssvt_amd import iou3d_nms_utils as u
    a, b = pair_sets(1, 20.0)
    rng = np.random.default_rng(11)
    wide_a = torch.from_numpy(np.concatenate([a, rng.normal(size=(160, 2)).astype(np.float32)], 1)).to(DEV)  # (N, 9)
    wide_b = torch.from_numpy(np.concatenate([b, np.ones((120, 1), np.float32)], 1)).to(DEV)                  # (M, 8)
    ta, tb = wide_a[:, 0:7].contiguous(), wide_b[:, 0:7].contiguous()
    assert not wide_a[:, 0:7].is_contiguous()
    for fn in (u.boxes_overlap_bev, u.boxes_iou_bev, u.boxes_iou3d_gpu):
        ref = fn(ta, tb)
        assert torch.equal(fn(wide_a[:, 0:7], wide_b[:, 0:7]), ref)  # read in place through the row stride
        assert torch.equal(fn(ta, tb), ref)                          # two calls, the same bits
        assert torch.equal(fn(ta.double(), tb.double()), ref)        # other dtypes are made fp32
    ref = u.boxes_iou3d_gpu(ta, tb)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        big = torch.randn(4096, 4096, device=DEV)
        ta2 = (big @ big)[:160, :7] * 0 + ta       # the inputs are produced on the side stream, after a long kernel
        out = u.boxes_iou3d_gpu(ta2, tb)
        best = out.max(dim=0)[0]                    # and the result is used on it
    side.synchronize()
    assert torch.equal(out, ref) and torch.equal(best, ref.max(dim=0)[0])


def anchor_boxes():
    c = ((np.arange(188) + 0.5) * 0.8 - 75.2).astype(np.float32)
    sizes = [[4.7, 2.1, 1.7], [0.91, 0.86, 1.73], [1.78, 0.84, 1.78]]
    out = np.zeros((3, 2, 188, 188, 7), np.float32)  # size-major, then heading, then x, then y
    out[..., 0] = c[None, None, :, None]
    out[..., 1] = c[None, None, None, :]
    for s, size in enumerate(sizes):
        out[s, ..., 3:6] = np.array(size, np.float32)
    out[:, 1, ..., 6] = np.float32(np.pi / 2)
    return out.reshape(-1, 7)


def test_anchor_scale(monkeypatch):
    from mssvt_amd import iou3d_nms_utils as u
    a, b = anchor_boxes(), boxes(128, np.random.default_rng(5), 75.0)
    assert a.shape == (212064, 7)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    ov_t, iou_t = u.boxes_overlap_bev(ta, tb), u.boxes_iou_bev(ta, tb)
    assert int((ov_t > 0).sum()) == int((iou_t > 0).sum()) > 0
    ov, iou = ov_t.cpu().numpy(), iou_t.cpu().numpy()
    cand = candidate_mask(a, b)
    assert int(cand.sum()) == 41950
    assert bool(is_zero_bits(ov[~cand]).all()) and bool(is_zero_bits(iou[~cand]).all())
    pairs = np.argwhere(cand)[np.random.default_rng(6).permutation(int(cand.sum()))[:2000]]
    want_ov, want_iou, d = oracle_on(a, b, pairs, monkeypatch)
    tol = max(4 * d, 1e-6)
    got_ov, got_iou = ov[pairs[:, 0], pairs[:, 1]], iou[pairs[:, 0], pairs[:, 1]]
    union = a[pairs[:, 0], 3] * a[pairs[:, 0], 4] + b[pairs[:, 1], 3] * b[pairs[:, 1], 4] - want_ov
    err_ov, err_iou = np.abs(got_ov - want_ov) / union, np.abs(got_iou - want_iou)
    print("anchors: %d candidates, %d of 2000 non-zero; d %.3g tol %.3g; worst overlap/union %.3g iou %.3g" % (
        int(cand.sum()), int((want_iou > 0).sum()), d, tol, err_ov.max(), err_iou.max()))
    assert np.array_equal(want_ov == 0, got_ov == 0) and np.array_equal(want_iou == 0, got_iou == 0)
    assert err_ov.max() <= tol, pairs[err_ov.argmax()]
    assert err_iou.max() <= tol, pairs[err_iou.argmax()]


def test_iou_matrix_agrees_with_the_nms():
    from mssvt_amd import iou3d_nms_utils as u
    bx, scores = _random_boxes(1024, 9)
    tb = torch.from_numpy(bx).to(DEV)
    kept, _ = u.nms_gpu(tb, torch.from_numpy(scores).to(DEV), 0.7)
    kept = kept.cpu().numpy()
    m = u.boxes_iou_bev(tb, tb).cpu().numpy()
    assert 100 < kept.size < 1024
    kk = m[np.ix_(kept, kept)]
    assert float(np.triu(kk, 1).max()) <= 0.7 + 1e-5           # no two kept boxes suppress each other (earlier vs later)
    dropped = np.setdiff1d(np.arange(1024), kept)
    for j in dropped:                                          # every dropped box has a kept suppressor of higher score
        better = kept[scores[kept] >= scores[j]]
        assert better.size and float(m[better, j].max()) > 0.7 - 1e-5, j
    same = greedy_nms(m, scores, 0.7) == kept.tolist()
    print("greedy NMS over the boxes_iou_bev matrix keeps exactly what nms_gpu keeps: %s" % same)


def test_detector_recall_bookkeeping_end_to_end():
    from mssvt_amd import centerpoint
    torch.manual_seed(0)
    det = centerpoint.build_detector().to(DEV).eval()
    with torch.no_grad():
        for h in det.dense_head.heads_list:  # random init: lift the heat map above the score threshold
            h.hm[-1].bias.fill_(0.5)
    B = 2
    pts = torch.from_numpy(synthetic.make_batch_points(40000, B, 123)).to(DEV)
    with torch.no_grad():
        preds, recall = det(dict(points=pts, batch_size=B))
    assert recall == {}
    gt = torch.zeros((B, 12, 8), device=DEV)
    copied = []
    for s, p in enumerate(preds):
        c = min(4, p["pred_boxes"].shape[0])
        assert c > 0
        gt[s, :c, 0:7] = p["pred_boxes"][:c]
        gt[s, c:c + 4, 0:7] = torch.tensor([0, 0, 30, 1, 1, 1, 0], dtype=torch.float32, device=DEV)  # above everything
        gt[s, :c + 4, 7] = 1
        copied.append(c)
    with torch.no_grad():
        preds2, recall = det(dict(points=pts, batch_size=B, gt_boxes=gt))
    want = {"gt": sum(copied) + 8}
    for t in ("0.3", "0.5", "0.7"):
        want["rcnn_" + t], want["roi_" + t] = sum(copied), 0
    assert recall == want and all(type(v) is int for v in recall.values())
    for p, q in zip(preds, preds2):  # ground truth in the batch does not change the predictions
        for k in ("pred_boxes", "pred_scores", "pred_labels"):
            assert torch.equal(p[k], q[k])
    # the static method, sample by sample, with rois = the predictions
    r = {}
    for s, p in enumerate(preds):
        r = centerpoint.CenterPoint.generate_recall_record(
            p["pred_boxes"], r, s, dict(gt_boxes=gt, rois=[q["pred_boxes"] for q in preds]), [0.3, 0.5, 0.7])
    assert r["gt"] == want["gt"] and all(r["roi_" + t] == r["rcnn_" + t] == sum(copied) for t in ("0.3", "0.5", "0.7"))


def test_pybind_stand_ins_reproduce_the_direct_route():
    from mssvt_amd import iou3d_nms_compat as c
    from mssvt_amd import iou3d_nms_utils as u
    a, b = pair_sets(2, 20.0)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    ans = torch.full((160, 120), -1.0, device=DEV)
    assert c.boxes_iou_bev_gpu(ta.contiguous(), tb.contiguous(), ans) == 1
    assert torch.equal(ans, u.boxes_iou_bev(ta, tb))
    ans = torch.full((160, 120), -1.0, device=DEV)
    assert c.boxes_overlap_bev_gpu(ta.contiguous(), tb.contiguous(), ans) == 1
    assert torch.equal(ans, u.boxes_overlap_bev(ta, tb))
    assert torch.equal(torch_iou3d_composition(ta, tb, ans), torch_iou3d_composition(ta, tb, u.boxes_overlap_bev(ta, tb)))
    bx, scores = _random_boxes(193, 4)
    tbx, ts = torch.from_numpy(bx).to(DEV), torch.from_numpy(scores).to(DEV)
    order = ts.sort(0, descending=True)[1]
    for fast, slow in ((u.nms_gpu, c.nms_gpu), (u.nms_normal_gpu, c.nms_normal_gpu)):
        keep = torch.LongTensor(193)  # the reference's calling sequence (iou3d_nms_utils.py:96-99)
        num_out = slow(tbx[order].contiguous(), keep, 0.25)
        assert isinstance(num_out, int) and torch.equal(order[keep[:num_out].to(DEV)], fast(tbx, ts, 0.25)[0])
