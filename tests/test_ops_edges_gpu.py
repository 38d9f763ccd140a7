"""The granular operators and the detector's NMS at the sizes where their code takes another path -- every comparison is
against a CPU oracle (oracle/nms_ref.py, oracle/cref.py) or a float64 restatement written here:

* NMS (csrc/nms_bev.hip): more than 4096 boxes, where k_nms_scan's removed bits spill into registers 1..3 of each lane,
  the 16384-box limit of one launch, the score-ordered chunks of iou3d_nms_utils._nms_ordered beyond it, both refusals;
* FPS (csrc/fps_nn.hip): every step of the reference block size 32 ... 1024, the dynamic LDS request crossing 64 KB
  (n = 769), the switch from points in LDS to points in global memory (n = 1025);
* three_nn: several 64-point chunks per batch item, a partial last chunk, a half-empty last workgroup;
* the gradients of gather_operation / grouping_operation (float atomics) and the grid-stride loops of K8 / K10.

NMS results are compared as lists (kept indices, best first).  Scores are pairwise distinct: the device sort is not stable
and the oracle's is, so a tie would compare two different orders.  What a case is there to exercise (boxes kept AND
removed in every 4096-rank block, the fate of rank 4096, survivors per 8192-rank prefix) is asserted on the oracle's
result before the kernel's is looked at, so a generator that stops exercising it fails the test."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import cref, nms_ref
from tests.test_box_iou_gpu import boxes
from tests.test_ops_gpu import _padded_offsets

pytestmark = pytest.mark.gpu
DEV = "cuda"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- NMS
def clustered(n, seed, spread, copies):
    """ceil(n / copies) random boxes, each `copies` times with N(0, 0.15) jitter on all seven fields, rows shuffled;
    scores from a permutation, so pairwise distinct."""
    rng = np.random.default_rng(seed)
    base = boxes(-(-n // copies), rng, spread)
    b = np.repeat(base, copies, axis=0)[:n] + rng.normal(0, 0.15, (n, 7)).astype(np.float32)
    b = np.ascontiguousarray(b[rng.permutation(n)], np.float32)
    scores = (0.1 + 0.9 * (rng.permutation(n) + 0.5) / n).astype(np.float32)
    assert np.unique(scores).size == n
    return b, scores


def ranks(scores):
    """rank[i] = position of box i in descending score order."""
    r = np.empty(scores.size, np.int64)
    r[np.argsort(-scores.astype(np.float64), kind="stable")] = np.arange(scores.size)
    return r


def kept_per_block(want, scores, block=4096):
    """Boxes the oracle keeps in each block of `block` consecutive score ranks that is full."""
    n = scores.size
    return np.bincount(ranks(scores)[want] // block, minlength=-(-n // block))[:n // block]


def assert_every_register_works(want, scores):
    """In every full block of 4096 ranks -- one register of k_nms_scan's removed bits -- boxes are kept and removed."""
    kept = kept_per_block(want, scores)
    print("kept per 4096-rank block %s, removed %s" % (kept.tolist(), (4096 - kept).tolist()))
    assert kept.size >= 3 and (kept >= 50).all() and (4096 - kept >= 50).all()


def assert_chunks_fit(want, scores, n):
    """The wrapper carries the survivors of every 8192-rank prefix into the next launch: they must fit beside a chunk."""
    r = np.sort(ranks(scores)[want])
    survivors = [int(np.searchsorted(r, lo)) for lo in range(8192, n, 8192)]
    print("survivors per 8192-rank prefix %s of %d kept" % (survivors, r.size))
    assert survivors and max(survivors) <= 8192


@functools.lru_cache(maxsize=None)
def oracle_case(kind, n, seed, spread, copies, thresh):
    b, scores = clustered(n, seed, spread, copies)
    want = nms_ref.nms_normal(b, scores, thresh) if kind == "normal" else nms_ref.nms_sparse(b, scores, thresh)
    for a in (b, scores, want):
        a.setflags(write=False)
    return b, scores, want


def run_nms(kind, b, scores, thresh, **kw):
    from mssvt_amd import iou3d_nms_utils as u
    fn = u.nms_normal_gpu if kind == "normal" else u.nms_gpu
    got, none = fn(torch.tensor(b, device=DEV), torch.tensor(scores, device=DEV), thresh, **kw)
    assert none is None and got.dtype == torch.int64
    return got.cpu().numpy().tolist()


@pytest.mark.parametrize("kind,n", [("normal", 4096), ("normal", 12289), ("normal", 16384), ("rotated", 16384)])
def test_nms_one_launch_beyond_register_0(kind, n):
    """col_blocks = 64, 193 and 256: register 0 full, one word in register 3, the limit of one launch."""
    b, scores, want = oracle_case(kind, n, n, 300.0, 3, 0.3)
    if n >= 12289:
        assert_every_register_works(want, scores)
    else:
        assert 50 <= want.size <= n - 50
    assert run_nms(kind, b, scores, 0.3) == want.tolist()


@pytest.mark.parametrize("kind", ["normal", "rotated"])
def test_nms_4097_boxes_the_single_bit_of_register_1(kind):
    """Rank 4096 is bit 0 of word 64: lane 0, register 1.  Once the box is a copy of the best box (the bit is set while
    box 0 is processed and read 4096 boxes later), once it is alone 10 km away (the bit must still be clear)."""
    n = 4097
    b, scores = clustered(n, n, 300.0, 3)
    best, last = int(scores.argmax()), int(scores.argmin())
    oracle = nms_ref.nms_normal if kind == "normal" else nms_ref.nms_sparse
    twin = b.copy()
    twin[last] = twin[best]
    want = oracle(twin, scores, 0.3)
    assert want[0] == best and last not in want.tolist() and 50 <= want.size <= n - 50
    assert run_nms(kind, twin, scores, 0.3) == want.tolist()
    apart = b.copy()
    apart[last, 0:2] = 10000.0
    want = oracle(apart, scores, 0.3)
    assert want[-1] == last and 50 <= want.size <= n - 50
    assert run_nms(kind, apart, scores, 0.3) == want.tolist()


@pytest.mark.parametrize("kind,n", [("normal", 16385), ("normal", 20000), ("rotated", 20000)])
def test_nms_in_score_ordered_chunks(kind, n):
    """More boxes than one launch takes: chunks of 8192 (16385 = 8192 + 8192 + 1), the survivors in front of each."""
    b, scores, want = oracle_case(kind, n, n, 300.0, 4, 0.1)
    assert_chunks_fit(want, scores, n)
    assert 50 <= want.size <= n - 50
    assert run_nms(kind, b, scores, 0.1) == want.tolist()


def test_nms_in_score_ordered_chunks_with_pre_maxsize():
    """pre_maxsize = 17000 of 20000: greedy NMS decides a box from the boxes ranked before it alone, so what it keeps of
    the best 17000 is what it keeps of all 20000, cut at rank 17000 (tests/test_box_iou_cpu.py pins nms_sparse's own
    pre_maxsize to nms's)."""
    n, pre = 20000, 17000
    b, scores, want_all = oracle_case("rotated", n, n, 300.0, 4, 0.1)
    want = want_all[ranks(scores)[want_all] < pre]
    assert_chunks_fit(want, scores, pre)
    assert 50 <= want.size < want_all.size
    assert run_nms("rotated", b, scores, 0.1, pre_maxsize=pre) == want.tolist()


def test_nms_refuses_more_survivors_than_a_launch_takes():
    """16385 pairwise disjoint boxes: 16384 survive two chunks, the last box no longer fits beside them."""
    from mssvt_amd import _lib
    n = 16385
    gx, gy = np.meshgrid(np.arange(129, dtype=np.float32) * 10, np.arange(128, dtype=np.float32) * 10, indexing="ij")
    b = np.zeros((129 * 128, 7), np.float32)
    b[:, 0], b[:, 1], b[:, 3], b[:, 4], b[:, 5] = gx.ravel(), gy.ravel(), 2.0, 1.0, 1.0
    b = b[:n]
    scores = (0.1 + 0.9 * (np.random.default_rng(0).permutation(n) + 0.5) / n).astype(np.float32)
    assert np.unique(scores).size == n
    with pytest.raises(_lib.MssvtHipError, match="8192"):
        run_nms("rotated", b, scores, 0.5)
    # one box fewer is one launch, and every box is kept
    assert run_nms("rotated", b[:-1], scores[:-1], 0.5) == np.argsort(-scores[:-1].astype(np.float64)).tolist()


def test_nms_entry_point_refuses_16385_boxes():
    """mssvt_nms_bev returns MSSVT_E_TOOLARGE before any launch."""
    from mssvt_amd import _lib
    n = 16385
    lib = _lib.lib()
    b = torch.zeros((n, 7), dtype=torch.float32, device=DEV)
    ws = torch.empty(int(lib.mssvt_nms_workspace_bytes(ctypes.c_int(n))) // 8 + 1, dtype=torch.int64, device=DEV)
    keep = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    for entry in ("mssvt_nms_bev", "mssvt_nms_normal"):
        with pytest.raises(_lib.MssvtHipError, match="size exceeds"):
            _lib.call(entry, ctypes.c_int(n), _lib.ptr(b), ctypes.c_float(0.5), _lib.ptr(ws), _lib.ptr(keep),
                      _lib.ptr(cnt), _lib.stream())
    assert int(cnt.item()) == -7 and bool((keep == -7).all())  # nothing ran


# ---------------------------------------------------------------- K7
FPS_B, FPS_M = 9, 32  # nine batch items: the third workgroup holds one live wave of four


@pytest.mark.parametrize("n", [63, 64, 65, 127, 128, 129, 511, 512, 513, 768, 769, 1000, 1023, 1024, 1025, 2048])
def test_farthest_point_sample_at_the_tree_and_lds_boundaries(n):
    """The reference block size steps 32 -> 64 -> 128 -> 256 -> 512 -> 1024 across the list (two and three LDS levels
    above the shuffle levels at 512 and 1024), the LDS request passes 64 KB at 769, the points leave LDS at 1025."""
    from mssvt_amd import pointnet2_utils as pn2
    assert cref.opt_n_threads(n) == min(1024, 1 << (n.bit_length() - 1))
    xyz = _padded_offsets(np.random.default_rng(n), FPS_B, n, -3, 3, n)
    want = cref.farthest_point_sample(xyz, FPS_M)
    got = pn2.farthest_point_sample(t(xyz), FPS_M)
    np.testing.assert_array_equal(got.cpu().numpy(), want)


def test_farthest_point_sample_floats_identical_points_and_more_samples_than_points():
    from mssvt_amd import pointnet2_utils as pn2
    rng = np.random.default_rng(7)
    for xyz, m in ((rng.standard_normal((FPS_B, 1000, 3)).astype(np.float32), FPS_M),
                   (np.full((FPS_B, 1024, 3), 1.5, np.float32), FPS_M),  # every round is a full tie, at 96 KB of LDS
                   (rng.integers(-3, 4, (FPS_B, 3, 3)).astype(np.float32), 8)):
        want = cref.farthest_point_sample(xyz, m)
        got = pn2.farthest_point_sample(t(xyz), m)
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=str(xyz.shape))


# ---------------------------------------------------------------- K9
def _grid_points(rng, b, n):
    return (rng.integers(-3, 4, (b, n, 3)) * np.array([0.32, 0.32, 0.1875])).astype(np.float32) + 10.0


@pytest.mark.parametrize("B,N,M", [(3, 64, 20), (5, 65, 20), (7, 200, 45), (1, 129, 3)])
def test_three_nn_across_chunks(B, N, M):
    """One, two, four and three 64-point chunks per batch item; (5, 65, 20) is ten wave items, so the last workgroup has
    two live waves, and every shape but the first ends in a partial chunk."""
    from mssvt_amd import pointnet2_utils as pn2
    rng = np.random.default_rng(B * 1000 + N)
    unknown, known = _grid_points(rng, B, N), _grid_points(rng, B, M)
    wd, wi = cref.three_nn(unknown, known)
    ties = float((wd[..., 0] == wd[..., 1]).mean())
    print("first and second distance equal at %.1f %% of the points" % (100 * ties))
    if M >= 45:  # the densest shape: a quarter of the 343 grid positions are known points
        assert ties >= 0.05
    gd, gi = pn2.three_nn(t(unknown), t(known))
    np.testing.assert_array_equal(gi.cpu().numpy(), wi)
    np.testing.assert_allclose(gd.cpu().numpy(), wd, rtol=1e-6)


@pytest.mark.parametrize("B,N,M", [(6, 70, 2), (2, 70, 1)])
def test_three_nn_with_fewer_than_three_known_points(B, N, M):
    from mssvt_amd import pointnet2_utils as pn2
    rng = np.random.default_rng(B * 1000 + M)
    unknown, known = _grid_points(rng, B, N), _grid_points(rng, B, M)
    wd, wi = cref.three_nn(unknown, known)
    assert np.isinf(wd[..., M:]).all() and np.isfinite(wd[..., :M]).all()
    gd, gi = pn2.three_nn(t(unknown), t(known))
    gd = gd.cpu().numpy()
    np.testing.assert_array_equal(gi.cpu().numpy(), wi)
    np.testing.assert_array_equal(np.isinf(gd), np.isinf(wd))
    np.testing.assert_allclose(gd[..., :M], wd[..., :M], rtol=1e-6)


# ---------------------------------------------------------------- K8 / K10 and their gradients
def scatter_add_reference(grad_out, idx, N):
    """grad[b, c, idx[b, j]] += grad_out[b, c, j] in float64; also the sum of |terms| and the number of terms per
    destination, for the bound on a float32 sum in any order."""
    B, C, J = grad_out.shape
    where = (np.arange(B)[:, None, None], np.arange(C)[None, :, None], idx[:, None, :].astype(np.int64))
    want, mag = np.zeros((B, C, N)), np.zeros((B, C, N))
    np.add.at(want, where, grad_out.astype(np.float64))
    np.add.at(mag, where, np.abs(grad_out.astype(np.float64)))
    terms = np.zeros((B, N), np.int64)
    np.add.at(terms, (np.arange(B)[:, None], idx.astype(np.int64)), 1)
    return want, mag, terms


def assert_atomic_sum(got, want, mag, terms):
    """A float32 sum of k terms t_i in any order is within (k - 1) u sum |t_i| (1 + O(k u)) of the exact sum, u = 2^-24
    (one rounding per addition, each at most u times a partial sum of magnitude <= sum |t_i|); k u sum |t_i| covers it.
    A destination nothing was added to keeps the 0.0 it was allocated with."""
    assert got.dtype == np.float32 and got.shape == want.shape
    k = np.broadcast_to(terms[:, None, :], want.shape)
    err, bound = np.abs(got.astype(np.float64) - want), k * 2.0 ** -24 * mag
    print("terms per destination up to %d, %d of %d destinations empty, worst error / bound %.3g" % (
        int(terms.max()), int((terms == 0).sum()), terms.size, float((err[k > 0] / bound[k > 0]).max())))
    assert (err <= bound).all()
    assert (got[k == 0] == 0.0).all()


GATHER_SHAPES = [(6, 16, 343, 32, "random"), (6, 16, 343, 32, "equal"), (17, 64, 300, 2048, "random")]


@pytest.mark.parametrize("B,C,N,npoint,how", GATHER_SHAPES)
def test_gather_operation_gradient(B, C, N, npoint, how):
    """(17, 64, 300, 2048) is 2 228 224 elements: more than the 8192 x 256 threads of the grid, so the loop iterates."""
    from mssvt_amd import pointnet2_utils as pn2
    rng = np.random.default_rng(N + npoint)
    feats = rng.standard_normal((B, C, N)).astype(np.float32)
    idx = rng.integers(0, N, (B, npoint)).astype(np.int32)
    if how == "equal":  # one address takes all the atomics of its row
        idx[:] = rng.integers(0, N, (B, 1))
    f = t(feats).requires_grad_(True)
    out = pn2.gather_operation(f, t(idx))
    if B * C * npoint > 8192 * 256:
        np.testing.assert_array_equal(out.detach().cpu().numpy(), cref.gather_operation(feats, idx))
    go = rng.standard_normal((B, C, npoint)).astype(np.float32)
    out.backward(t(go))
    want, mag, terms = scatter_add_reference(go, idx, N)
    if how == "equal":
        assert int(terms.max()) == npoint
    else:
        assert 0 < int((terms == 0).sum()) < terms.size and int(terms.max()) > 1
    assert_atomic_sum(f.grad.cpu().numpy(), want, mag, terms)


@pytest.mark.parametrize("B,C,N,npts,nsample", [(6, 16, 20, 45, 3), (9, 32, 64, 256, 32)])
def test_grouping_operation_gradient(B, C, N, npts, nsample):
    """(9, 32, 64, 256, 32) is 2 359 296 elements: the grid-stride loop iterates."""
    from mssvt_amd import pointnet2_utils as pn2
    rng = np.random.default_rng(N + npts)
    feats = rng.standard_normal((B, C, N)).astype(np.float32)
    idx = rng.integers(0, N, (B, npts, nsample)).astype(np.int32)
    idx[idx == 5] = 6  # a destination nothing is added to
    f = t(feats).requires_grad_(True)
    out = pn2.grouping_operation(f, t(idx))
    if B * C * npts * nsample > 8192 * 256:
        np.testing.assert_array_equal(out.detach().cpu().numpy(), cref.group_points(feats, idx))
    go = rng.standard_normal((B, C, npts, nsample)).astype(np.float32)
    out.backward(t(go))
    want, mag, terms = scatter_add_reference(go.reshape(B, C, npts * nsample), idx.reshape(B, npts * nsample), N)
    assert (terms[:, 5] == 0).all() and int(terms.max()) > 1
    assert_atomic_sum(f.grad.cpu().numpy(), want, mag, terms)
