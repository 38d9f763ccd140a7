"""CenterHead's shared layer and trunk in training mode: the C entry points of csrc/head_conv.hip (mssvt_head_conv_shared_train /
_dgrad / _wgrad, mssvt_head_conv_trunk_train / _dgrad / _wgrad, mssvt_head_conv_bgrad) and the Functions of
``mssvt_amd.head_conv_train`` against the float64 statement and the bounds of tests/head_conv_train_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

from mssvt_amd import _lib, bev_conv, head_conv_train as hct
from mssvt_amd._lib import MssvtHipError
from tests import bev_conv_train_ref as tref, head_conv_train_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHARED = ref.SHARED_SHAPES
NARROW = (64, 32)
TRUNK = [(s, nb) for s in ref.TRUNK_S for nb in (1, 2, 5)]
KINDS = ("plain", "tail", "spike")
SL = ref.SLICE_PIXELS
# (B, H, W): one pixel | 31 / 32 / 33 pixels (the wave tile) | a wave tile spanning two samples, odd widths | 255 / 256 / 257 (the
# workgroup tile) | a workgroup tile spanning samples
EDGE_SIZES = [(1, 1, 1), (1, 1, 31), (1, 4, 8), (1, 3, 11), (2, 3, 5), (1, 15, 17), (1, 16, 16), (1, 257, 1), (3, 7, 13)]
# pixel counts either side of one, two and three slices: all six for the narrow shape, spread over the wide ones
SLICE_CASES = [(NARROW, n) for n in (SL - 1, SL + 1, 2 * SL - 1, 2 * SL + 1, 3 * SL - 1, 3 * SL + 1)] + \
              [((256, 64), SL - 1), ((256, 64), 2 * SL + 1), ((384, 32), SL + 1), ((384, 32), 3 * SL - 1),
               ((512, 64), 2 * SL - 1), ((512, 64), 3 * SL + 1)]
TRUNK_SLICE_CASES = [((32, 2), SL - 1), ((32, 5), SL + 1), ((32, 1), 2 * SL - 1), ((64, 2), 2 * SL + 1), ((64, 1), 3 * SL - 1),
                     ((64, 5), 3 * SL + 1)]


def grid_of(n):
    """(H, W) with H W = n and W the odd divisor of n nearest to sqrt(n)."""
    w = min((d for d in range(1, n + 1, 2) if n % d == 0), key=lambda d: abs(d - n ** 0.5))
    return n // w, w


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).permute(0, 3, 1, 2)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rows(t):
    return t.permute(0, 2, 3, 1).cpu().numpy()


def fwd(x, w, bias=None):
    return rows(hct.shared_forward(nchw(x), dev(w), dev(bias)))


def dgrad(dy, w):
    return rows(hct.shared_dgrad(nchw(dy), dev(w)))


def wgrad(x, dy):
    return hct.shared_wgrad(nchw(x), nchw(dy)).cpu().numpy()


def bgrad(dys):
    return hct.bias_grad([nchw(d) for d in dys]).cpu().numpy()


def t_fwd(y, ws, bs):
    return [rows(t) for t in hct.trunk_forward(nchw(y), [dev(w) for w in ws], [dev(b) for b in bs])]


def t_dgrad(dts, ws):
    return rows(hct.trunk_dgrad([nchw(d) for d in dts], [dev(w) for w in ws]))


def t_wgrad(y, dts):
    return hct.trunk_wgrad(nchw(y), [nchw(d) for d in dts]).cpu().numpy()


def inside(got, want_bound, what):
    want, bound = want_bound
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst error / bound %.3f" % (what, ratio))
    assert got.shape == want.shape and (err <= bound).all(), (what, ratio)
    return ratio


def bias_of(s, seed, on=True):
    return np.random.default_rng(seed).standard_normal(s).astype(np.float32) if on else None


def trunk_inputs(kind, B, H, W, s, nb, seed):
    y = tref.inputs(kind, B, H, W, s, s, seed)[0]
    dts = [tref.inputs(kind, B, H, W, s, s, seed + 1 + b)[1] for b in range(nb)]
    ws = [ref.weights(s, s, seed + 100 + b) for b in range(nb)]
    return y, dts, ws


def test_the_rules_and_the_workspaces_are_as_published():
    lib = _lib.lib()
    r256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for cin in (64, 256, 384, 512):
        for s in (32, 64):
            assert lib.mssvt_head_conv_train_supported(cin, s, 1) == 1 and lib.mssvt_head_conv_train_supported(cin, s, 64) == 1
            assert hct.slice_pixels(cin, s) == ref.SLICE_PIXELS and hct.slice_pixels(s, s) == ref.SLICE_PIXELS
            assert hct.bias_piece_rows(s) == ref.BIAS_PIECE_ROWS
            for B, H, W in ((1, 3, 2 * SL), (2, 5, 7), (1, 1, 1), (1, 1, 3 * SL + 1)):
                M = B * H * W
                assert lib.mssvt_head_conv_shared_dgrad_workspace_bytes(B, H, W, cin, s) == r256(4 * M) + 64 + 8 * cin + 36 * cin * s
                assert lib.mssvt_head_conv_shared_wgrad_workspace_bytes(B, H, W, cin, s) == \
                    2 * r256(4 * M) + -(-M // SL) * 9 * cin * s * 4
                for nb in (1, 5):
                    assert lib.mssvt_head_conv_trunk_dgrad_workspace_bytes(B, H, W, s, nb) == \
                        r256(4 * nb * M) + 64 + 8 * s + 36 * s * s * nb
                    assert lib.mssvt_head_conv_trunk_wgrad_workspace_bytes(B, H, W, s, nb) == \
                        r256(4 * M) + r256(4 * nb * M) + -(-M // SL) * 9 * nb * s * s * 4
                    assert lib.mssvt_head_conv_bgrad_workspace_bytes(B, H, W, s, nb) == -(-M // ref.BIAS_PIECE_ROWS) * nb * s * 4
    for bad in [(128, 64, 1), (512, 48, 1), (512, 64, 0), (512, 64, 65), (0, 32, 1), (64, 128, 2)]:
        assert lib.mssvt_head_conv_train_supported(*bad) == 0, bad
    assert hct.slice_pixels(512, 48) == 0 and hct.slice_pixels(128, 64) == 0 and hct.bias_piece_rows(48) == 0
    assert hct.slice_pixels(32, 64) == 0  # (the trunk is (s, s): no entry point covers 32 -> 64)


# ---- random operands: every element inside its bound -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHARED)
@pytest.mark.parametrize("i", range(len(EDGE_SIZES)))
def test_shared_forward_and_input_gradient_at_the_tile_edges(i, shape):
    cin, s = shape
    B, H, W = EDGE_SIZES[i]
    kind = KINDS[i % 3]
    x, dy = tref.inputs(kind, B, H, W, cin, s, seed=10 * i + s)
    w, bias = ref.weights(s, cin, i), bias_of(s, i, i % 2 == 0)
    tag = "%s %s %s bias=%s" % (shape, (B, H, W), kind, bias is not None)
    inside(fwd(x, w, bias), ref.forward(x, w, bias), "y " + tag)
    inside(dgrad(dy, w), ref.dx(dy, w), "dX " + tag)


@pytest.mark.parametrize("i", range(len(SLICE_CASES)))
def test_shared_weight_and_bias_gradient_either_side_of_the_slices(i):
    (cin, s), n = SLICE_CASES[i]
    H, W = grid_of(n)
    kind = KINDS[i % 3]
    x, dy = tref.inputs(kind, 1, H, W, cin, s, seed=7 * i + s)
    tag = "%s %d pixels %s" % ((cin, s), n, kind)
    inside(wgrad(x, dy), ref.dw(x, dy, hct.slice_pixels(cin, s)), "dW " + tag)
    inside(bgrad([dy])[0], ref.db(dy, hct.bias_piece_rows(s)), "db " + tag)


@pytest.mark.parametrize("shape", [NARROW, (512, 64)])
def test_a_slice_may_span_two_samples(shape):
    cin, s = shape
    H, W = 9, SL // 12  # samples of ~0.75 slices: slice 0 ends inside sample 1
    B = 3
    assert tref.num_slices(B * H * W, SL) == B and H * W < SL
    x, dy = tref.inputs("plain", B, H, W, cin, s, seed=5)
    inside(wgrad(x, dy), ref.dw(x, dy, SL), "dW spanning %s" % (shape,))
    inside(bgrad([dy])[0], ref.db(dy), "db spanning %s" % (shape,))


@pytest.mark.parametrize("s,nb", TRUNK)
@pytest.mark.parametrize("i", range(len(EDGE_SIZES)))
def test_trunk_forward_and_input_gradient_at_the_tile_edges(i, s, nb):
    B, H, W = EDGE_SIZES[i]
    kind = KINDS[(i + nb) % 3]
    y, dts, ws = trunk_inputs(kind, B, H, W, s, nb, seed=10 * i + s + nb)
    bs = [bias_of(s, b, (i + b) % 2 == 0) for b in range(nb)]
    tag = "S=%d nb=%d %s %s" % (s, nb, (B, H, W), kind)
    for b, (got, want) in enumerate(zip(t_fwd(y, ws, bs), ref.trunk_forward(y, ws, bs))):
        inside(got, want, "t_%d %s" % (b, tag))
    inside(t_dgrad(dts, ws), ref.trunk_dy(dts, ws), "dy " + tag)


@pytest.mark.parametrize("i", range(len(TRUNK_SLICE_CASES)))
def test_trunk_weight_and_bias_gradient_either_side_of_the_slices(i):
    (s, nb), n = TRUNK_SLICE_CASES[i]
    H, W = grid_of(n)
    kind = KINDS[i % 3]
    y, dts, _ = trunk_inputs(kind, 1, H, W, s, nb, seed=3 * i + s)
    got_w, got_b = t_wgrad(y, dts), bgrad(dts)
    assert got_w.shape == (nb, s, s, 3, 3) and got_b.shape == (nb, s)
    for b, (want_w, want_b) in enumerate(zip(ref.trunk_dw(y, dts, hct.slice_pixels(s, s)), ref.trunk_db(dts, hct.bias_piece_rows(s)))):
        inside(got_w[b], want_w, "dW_%d S=%d nb=%d %d pixels %s" % (b, s, nb, n, kind))
        inside(got_b[b], want_b, "db_%d S=%d nb=%d %d pixels %s" % (b, s, nb, n, kind))


def test_trunk_slice_spanning_two_samples():
    s, nb = 64, 2
    H, W, B = 9, SL // 12, 3
    y, dts, _ = trunk_inputs("plain", B, H, W, s, nb, seed=9)
    got = t_wgrad(y, dts)
    for b, want in enumerate(ref.trunk_dw(y, dts, SL)):
        inside(got[b], want, "trunk dW_%d spanning" % b)


# ---- integer operands: bit for bit -----------------------------------------------------------------------------------------------
def ints(rng, shape, top):
    return rng.integers(-top, top + 1, shape).astype(np.float32)


@pytest.mark.parametrize("shape", SHARED)
def test_shared_integer_operands_are_exact(shape):
    cin, s = shape
    rng = np.random.default_rng(cin + s)
    B, H, W = 2, 9, 13
    x, dy, w, bias = ints(rng, (B, H, W, cin), 8), ints(rng, (B, H, W, s), 8), ints(rng, (s, cin, 3, 3), 4), ints(rng, (s,), 100)
    np.testing.assert_array_equal(fwd(x, w, bias), ref.forward(x, w, bias)[0])
    np.testing.assert_array_equal(fwd(x, w), ref.forward(x, w)[0])
    np.testing.assert_array_equal(dgrad(dy, w), ref.dx(dy, w)[0])
    np.testing.assert_array_equal(wgrad(x, dy), ref.dw(x, dy)[0])
    np.testing.assert_array_equal(bgrad([dy])[0], ref.db(dy)[0])


@pytest.mark.parametrize("s,nb", TRUNK)
def test_trunk_integer_operands_are_exact(s, nb):
    rng = np.random.default_rng(s + nb)
    B, H, W = 2, 9, 13
    y = ints(rng, (B, H, W, s), 8)
    dts = [ints(rng, (B, H, W, s), 8) for _ in range(nb)]
    ws = [ints(rng, (s, s, 3, 3), 4) for _ in range(nb)]
    bs = [ints(rng, (s,), 100) if b % 2 == 0 else None for b in range(nb)]
    for got, (want, _) in zip(t_fwd(y, ws, bs), ref.trunk_forward(y, ws, bs)):
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(t_dgrad(dts, ws), ref.trunk_dy(dts, ws)[0])
    got_w, got_b = t_wgrad(y, dts), bgrad(dts)
    for b in range(nb):
        np.testing.assert_array_equal(got_w[b], ref.dw(y, dts[b])[0])
        np.testing.assert_array_equal(got_b[b], ref.db(dts[b])[0])


# ---- impulses ------------------------------------------------------------------------------------------------------------------
PLACES = [(0, 0, 0), (1, 4, 6), (0, 0, 3), (1, 2, 0), (1, 2, 3)]  # corners, edges, interior of a 5 x 7 map


def planted_weights(cout, cin):
    """w[o, c, ky, kx] = +-(1 + q / 64)(1 + 2^-13), q and the sign functions of (o, c, ky, kx): a value read from another channel
    or tap is another number; hi = +-(1 + q / 64) and a non-zero lo that the split carries exactly."""
    o_, c_, ky_, kx_ = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(3), np.arange(3), indexing="ij")
    q = (7 * c_ + 3 * o_ + 13 * (3 * ky_ + kx_)) % 64
    exact = np.where((c_ + o_ + ky_ + kx_) % 2, -1.0, 1.0) * (1.0 + q / 64.0) * (1.0 + 2.0 ** -13)
    w = exact.astype(np.float32)
    assert np.array_equal(w.astype(np.float64), exact)
    return w


@pytest.mark.parametrize("shape", [NARROW, (512, 64)])
def test_weight_gradient_of_an_impulse_against_an_impulse_is_the_product_at_the_one_tap(shape):
    """x holds one value at one pixel and channel, dy one at one pixel and channel: dW is EXACTLY their product at the one tap that
    joins them (3 x 5 = 15; (1 + 2^-12)(1 + 2^-13): hi hi = 1 and exact cross terms give the float32 rounding of the product) and
    zero everywhere else; the trunk's dW_b the same in its own branch and zero in the others."""
    cin, s = shape
    B, H, W, c, n = 2, 5, 7, 5, s - 3
    pairs = [(3.0, 5.0), (1.0 + 2.0 ** -12, 1.0 + 2.0 ** -13)]
    hits = 0
    for k, (b, py, px) in enumerate(PLACES if shape == NARROW else PLACES[1:3]):
        for ky, kx in tref.TAPS:
            iy, ix = py + ky - 1, px + kx - 1
            if not (0 <= iy < H and 0 <= ix < W):
                continue
            vx, vd = pairs[(k + ky + kx) % 2]
            x, dy = np.zeros((B, H, W, cin), np.float32), np.zeros((B, H, W, s), np.float32)
            x[b, iy, ix, c], dy[b, py, px, n] = vx, vd
            want = np.zeros((s, cin, 3, 3), np.float32)
            want[n, c, ky, kx] = np.float32(vx * vd)
            np.testing.assert_array_equal(want, ref.dw(x, dy)[0].astype(np.float32))
            np.testing.assert_array_equal(wgrad(x, dy), want, err_msg=str((b, py, px, ky, kx)))
            hits += 1
    assert hits >= 9
    # the trunk: the impulse in branch 1 of 3
    y, dt = np.zeros((B, H, W, s), np.float32), np.zeros((B, H, W, s), np.float32)
    y[1, 1, 2, c], dt[1, 2, 3, n] = 3.0, 5.0
    got = t_wgrad(y, [np.zeros_like(dt), dt, np.zeros_like(dt)])
    want = np.zeros((3, s, s, 3, 3), np.float32)
    want[1, n, c, 0, 0] = 15.0
    np.testing.assert_array_equal(got, want)
    # another sample: no tap joins them
    x, dy = np.zeros((B, H, W, cin), np.float32), np.zeros((B, H, W, s), np.float32)
    x[0, 1, 1, c], dy[1, 1, 1, n] = 3.0, 5.0
    assert (wgrad(x, dy) == 0.0).all()


@pytest.mark.parametrize("shape", [NARROW, (512, 64), (384, 32)])
def test_input_gradient_of_an_impulse_reads_the_single_right_weights(shape):
    """A unit impulse of dy at (b, py, px, n) gives dx[b, py + ky - 1, px + kx - 1, :] = w[n, :, ky, kx] within 1 ulp at the up to
    nine pixels inside the image and exact zeros everywhere else; the trunk's dy the same with its branch's own weights."""
    cin, s = shape
    B, H, W, n = 2, 5, 7, s - 5
    w = planted_weights(s, cin)
    wb = [planted_weights(s, s) * np.float32(2.0 ** b) for b in range(3)]
    seen = set()
    for b, py, px in PLACES:
        dy = np.zeros((B, H, W, s), np.float32)
        dy[b, py, px, n] = 1.0
        got = dgrad(dy, w)
        got_t = t_dgrad([np.zeros_like(dy), np.zeros_like(dy), dy], wb)
        touched = 0
        for ky, kx in tref.TAPS:
            iy, ix = py + ky - 1, px + kx - 1
            if not (0 <= iy < H and 0 <= ix < W):
                continue
            for g, col in ((got, w[n, :, ky, kx]), (got_t, wb[2][n, :, ky, kx])):
                assert (np.abs(g[b, iy, ix] - col) <= np.spacing(np.abs(col))).all(), (b, py, px, ky, kx)
                g[b, iy, ix] = 0.0
            touched += 1
        seen.add(touched)
        assert (got == 0.0).all() and (got_t == 0.0).all(), (b, py, px)
    assert seen == {4, 6, 9}


# ---- branches of very different magnitude ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("s,nb", [(32, 2), (64, 5)])
def test_trunk_branches_planted_far_apart_keep_their_own_bounds(s, nb):
    """dT_1 is 2^20 above the other branches: every dW_b and db_b stays inside the bound computed from ITS OWN dT_b (the weight
    gradient normalises a slice's rows per branch), dy inside the shared bound (one chain, max|dT| over all branches)."""
    H, W = grid_of(SL + 77)
    y, dts, ws = trunk_inputs("plain", 1, H, W, s, nb, seed=21)
    dts = [d * np.float32(2.0 ** 20) if b == min(1, nb - 1) else d for b, d in enumerate(dts)]
    got_w, got_b = t_wgrad(y, dts), bgrad(dts)
    for b, (want_w, want_b) in enumerate(zip(ref.trunk_dw(y, dts), ref.trunk_db(dts))):
        inside(got_w[b], want_w, "dW_%d planted" % b)
        inside(got_b[b], want_b, "db_%d planted" % b)
    inside(t_dgrad(dts, ws), ref.trunk_dy(dts, ws), "dy planted")


# ---- powers of two -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [NARROW, (256, 64)])
def test_power_of_two_scaling_is_exact(shape):
    cin, s = shape
    H, W = grid_of(SL + SL // 2 + 1)  # two slices
    x, dy = tref.inputs("plain", 1, H, W, cin, s, seed=3)
    w = ref.weights(s, cin, 4)
    y0, dx0, dw0, db0 = fwd(x, w), dgrad(dy, w), wgrad(x, dy), bgrad([dy])
    yt, dts, ws = trunk_inputs("plain", 1, H, W, s, 2, seed=5)
    t0, ty0, tw0 = t_fwd(yt, ws, [None, None]), t_dgrad(dts, ws), t_wgrad(yt, dts)
    for p in (18, -20):
        f = np.float32(2.0 ** p)
        assert np.array_equal(fwd(x * f, w), y0 * f) and np.array_equal(fwd(x, w * f), y0 * f), p
        assert np.array_equal(dgrad(dy * f, w), dx0 * f) and np.array_equal(dgrad(dy, w * f), dx0 * f), p
        assert np.array_equal(wgrad(x * f, dy), dw0 * f) and np.array_equal(wgrad(x, dy * f), dw0 * f), p
        assert np.array_equal(bgrad([dy * f]), db0 * f), p
        assert all(np.array_equal(a, b * f) for a, b in zip(t_fwd(yt * f, ws, [None, None]), t0)), p
        assert np.array_equal(t_dgrad([d * f for d in dts], ws), ty0 * f), p
        assert np.array_equal(t_dgrad(dts, [v * f for v in ws]), ty0 * f), p
        assert np.array_equal(t_wgrad(yt * f, dts), tw0 * f) and np.array_equal(t_wgrad(yt, [d * f for d in dts]), tw0 * f), p
        # one branch alone: its own dW scales, the other's bits stay
        one = t_wgrad(yt, [dts[0] * f, dts[1]])
        assert np.array_equal(one[0], tw0[0] * f) and np.array_equal(one[1], tw0[1]), p


# ---- NaN / inf -------------------------------------------------------------------------------------------------------------------
def same_finite(got, want, count):
    bad = ~np.isfinite(want)
    assert bad.sum() == count, (bad.sum(), count)
    assert not np.isfinite(got[bad]).any() and np.isfinite(got[~bad]).all()


@pytest.mark.parametrize("shape", [NARROW, (512, 64)])
def test_non_finite_values_reach_exactly_what_they_should(shape):
    """A NaN at a corner pixel and an inf at an interior one (one channel each): the forward / input gradient is non-finite at
    exactly the 4 + 9 pixels whose taps read them (all channels), the weight gradient at exactly that channel's row for the taps
    inside the image, the bias gradient at exactly those channels; finite everywhere else."""
    cin, s = shape
    B, H, W = 2, 24, 30
    x, dy = tref.inputs("plain", B, H, W, cin, s, seed=8)
    w = ref.weights(s, cin, 9)
    xb, dyb = x.copy(), dy.copy()
    xb[0, 0, 0, 9], xb[1, 11, 7, 3] = np.nan, -np.inf
    dyb[0, 0, 0, 9], dyb[1, 11, 7, 3] = np.nan, -np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        same_finite(fwd(xb, w), ref.forward(xb, w)[0], 13 * s)
        same_finite(dgrad(dyb, w), ref.dx(dyb, w)[0], 13 * cin)
        same_finite(wgrad(x, dyb), ref.dw(x, dyb)[0], 13 * cin)
        same_finite(wgrad(xb, dy), ref.dw(xb, dy)[0], 13 * s)
        same_finite(bgrad([dyb])[0], ref.db(dyb)[0], 2)
        # the trunk: branch 1 of 3 holds them
        yt, dts, ws = trunk_inputs("plain", B, H, W, s, 3, seed=11)
        dts[1][0, 0, 0, 9], dts[1][1, 11, 7, 3] = np.nan, -np.inf
        same_finite(t_dgrad(dts, ws), ref.trunk_dy(dts, ws)[0], 13 * s)
        got = t_wgrad(yt, dts)
        same_finite(got[1], ref.dw(yt, dts[1])[0], 13 * s)
        assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
        gb = bgrad(dts)
        assert np.isfinite(gb[0]).all() and np.isfinite(gb[2]).all() and (~np.isfinite(gb[1])).sum() == 2


# ---- reads, writes, determinism --------------------------------------------------------------------------------------------------
def guarded(values, guard=4096):
    n = values.size
    big = torch.full((n + 2 * guard,), float("nan"), device=DEV)
    big[guard:guard + n] = torch.from_numpy(np.ascontiguousarray(values)).to(DEV).reshape(-1)
    return big, big[guard:guard + n]


def guards_intact(big, n, guard=4096):
    return bool(torch.isnan(big[:guard]).all()) and bool(torch.isnan(big[guard + n:]).all())


def ff_filled(n, guard=4096):
    """n floats of 0xFF bytes inside a NaN-filled allocation."""
    big = torch.full((n + 2 * guard,), float("nan"), device=DEV)
    big[guard:guard + n].view(torch.uint8).fill_(0xFF)
    return big, big[guard:guard + n]


def pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


@pytest.mark.parametrize("shape,nb,hw", [((512, 64), 5, (17, 19)), (NARROW, 2, (6, 51)), ((384, 32), 1, (1, 1)), ((64, 64), 3, (34, 33))])
def test_reads_stay_inside_the_inputs_and_every_output_element_is_written(shape, nb, hw):
    """Inputs are slices of NaN-filled allocations (a read outside them poisons the result); outputs and workspaces are filled
    with 0xFF bytes inside NaN-filled allocations: outputs fully written, the guards untouched, the bits those of the wrappers'
    runs on fresh memory."""
    cin, s = shape
    B, (H, W) = 2, hw
    M = B * H * W
    lib, st = _lib.lib(), _lib.stream()
    xs, dys = tref.inputs("plain", B, H, W, cin, s, seed=6)
    w, bias = ref.weights(s, cin, 7), bias_of(s, 8)
    yt, dts, tws = trunk_inputs("plain", B, H, W, s, nb, seed=12)
    ins = [guarded(a) for a in [xs, dys, w, bias, yt] + dts + tws]
    (x, dy, wt, bt, y), dtv, twv = [v for _, v in ins[:5]], [v for _, v in ins[5:5 + nb]], [v for _, v in ins[5 + nb:]]
    sizes = [a.size for a in [xs, dys, w, bias, yt] + dts + tws]
    outs = []

    def out(n):
        outs.append((ff_filled(n), n))
        return outs[-1][0][1]

    def ws(name, *a):
        n = int(getattr(lib, name)(*a))
        assert n > 0 and n % 4 == 0
        return out(n // 4)

    # the shared layer
    blob = torch.zeros(int(lib.mssvt_head_conv_shared_pack_bytes(cin, s)), dtype=torch.uint8, device=DEV)
    _lib.call("mssvt_head_conv_shared_pack", wt.data_ptr(), bt.data_ptr(), None, None, None, None, 0.0, cin, s, blob.data_ptr(), st)
    o_y, o_e = out(M * s), out(M)
    _lib.call("mssvt_head_conv_shared_train", x.data_ptr(), B, H, W, cin, s, blob.data_ptr(), o_e.data_ptr(), o_y.data_ptr(), st)
    o_dx = out(M * cin)
    _lib.call("mssvt_head_conv_shared_dgrad", dy.data_ptr(), wt.data_ptr(), B, H, W, cin, s, o_dx.data_ptr(),
              ws("mssvt_head_conv_shared_dgrad_workspace_bytes", B, H, W, cin, s).data_ptr(), st)
    o_dw = out(w.size)
    _lib.call("mssvt_head_conv_shared_wgrad", x.data_ptr(), dy.data_ptr(), B, H, W, cin, s, o_dw.data_ptr(),
              ws("mssvt_head_conv_shared_wgrad_workspace_bytes", B, H, W, cin, s).data_ptr(), st)
    o_db = out(s)
    _lib.call("mssvt_head_conv_bgrad", pointers([dy]), B, H, W, s, 1, o_db.data_ptr(),
              ws("mssvt_head_conv_bgrad_workspace_bytes", B, H, W, s, 1).data_ptr(), st)
    # the trunk
    tblob = torch.zeros(int(lib.mssvt_head_conv_trunk_pack_bytes(s, nb)), dtype=torch.uint8, device=DEV)
    for b in range(nb):
        _lib.call("mssvt_head_conv_trunk_pack", twv[b].data_ptr(), None, None, None, None, None, 0.0, s, nb, b, tblob.data_ptr(), st)
    o_t, o_te = out(nb * M * s), out(M)
    _lib.call("mssvt_head_conv_trunk_train", y.data_ptr(), B, H, W, s, nb, tblob.data_ptr(), o_te.data_ptr(), o_t.data_ptr(), st)
    o_ty = out(M * s)
    _lib.call("mssvt_head_conv_trunk_dgrad", pointers(dtv), pointers(twv), B, H, W, s, nb, o_ty.data_ptr(),
              ws("mssvt_head_conv_trunk_dgrad_workspace_bytes", B, H, W, s, nb).data_ptr(), st)
    o_tw = out(nb * s * s * 9)
    _lib.call("mssvt_head_conv_trunk_wgrad", y.data_ptr(), pointers(dtv), B, H, W, s, nb, o_tw.data_ptr(),
              ws("mssvt_head_conv_trunk_wgrad_workspace_bytes", B, H, W, s, nb).data_ptr(), st)
    o_tb = out(nb * s)
    _lib.call("mssvt_head_conv_bgrad", pointers(dtv), B, H, W, s, nb, o_tb.data_ptr(),
              ws("mssvt_head_conv_bgrad_workspace_bytes", B, H, W, s, nb).data_ptr(), st)
    torch.cuda.synchronize()
    for (big, _), n in [(i, n) for i, n in zip(ins, sizes)] + [(o[0], o[1]) for o in outs]:
        assert guards_intact(big, n)
    results = [o_y, o_dx, o_dw, o_db, o_t, o_ty, o_tw, o_tb]
    assert all(bool(torch.isfinite(r).all()) for r in results)
    np.testing.assert_array_equal(o_y.view(B, H, W, s).cpu().numpy(), fwd(xs, w, bias))
    np.testing.assert_array_equal(o_dx.view(B, H, W, cin).cpu().numpy(), dgrad(dys, w))
    np.testing.assert_array_equal(o_dw.view(s, cin, 3, 3).cpu().numpy(), wgrad(xs, dys))
    np.testing.assert_array_equal(o_db.cpu().numpy(), bgrad([dys])[0])
    np.testing.assert_array_equal(o_t.view(nb, B, H, W, s).cpu().numpy(), np.stack(t_fwd(yt, tws, [None] * nb)))
    np.testing.assert_array_equal(o_ty.view(B, H, W, s).cpu().numpy(), t_dgrad(dts, tws))
    np.testing.assert_array_equal(o_tw.view(nb, s, s, 3, 3).cpu().numpy(), t_wgrad(yt, dts))
    np.testing.assert_array_equal(o_tb.view(nb, s).cpu().numpy(), bgrad(dts))


def everything(x, dy, w, bias, y, dts, ws):
    return [hct.shared_forward(x, w, bias), hct.shared_dgrad(dy, w), hct.shared_wgrad(x, dy), hct.bias_grad([dy]),
            torch.stack(hct.trunk_forward(y, ws, [None] * len(ws))), hct.trunk_dgrad(dts, ws), hct.trunk_wgrad(y, dts), hct.bias_grad(dts)]


def device_operands(shape, nb, B, H, W, seed):
    cin, s = shape
    xs, dys = tref.inputs("plain", B, H, W, cin, s, seed=seed)
    yt, dts, tws = trunk_inputs("plain", B, H, W, s, nb, seed=seed + 1)
    return (nchw(xs), nchw(dys), dev(ref.weights(s, cin, seed)), dev(bias_of(s, seed)), nchw(yt), [nchw(d) for d in dts],
            [dev(v) for v in tws])


@pytest.mark.parametrize("shape,nb", [(NARROW, 2), ((512, 64), 5)])
def test_bit_identical_across_calls_and_streams(shape, nb):
    H, W = 50, (2 * SL + 100) // 100  # three slices over two samples
    ops = device_operands(shape, nb, 2, H, W, seed=12)
    assert tref.num_slices(2 * H * W, SL) == 3
    first, again = everything(*ops), everything(*ops)
    torch.cuda.synchronize()
    runs = [again]
    for _ in range(2):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            runs.append(everything(*ops))
        st.synchronize()
    for run in runs:
        assert all(torch.equal(a, b) for a, b in zip(first, run))


def test_nothing_synchronises_the_host():
    ops = device_operands(NARROW, 3, 2, 18, 41, seed=15)
    x, dy, w, bias, y, dts, ws = ops
    warm = everything(*ops)
    xg, wg, bg = x.clone().requires_grad_(), w.clone().requires_grad_(), bias.clone().requires_grad_()
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
            out = everything(*ops)
            hct.SharedFunction.apply(xg, wg, bg).backward(dy)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    assert all(torch.equal(a, b) for a, b in zip(warm, out))
    assert torch.equal(wg.grad, warm[2])


def test_every_status_code_is_reached_and_nothing_is_launched():
    lib, st = _lib.lib(), _lib.stream()
    BAD, BIG = -1, -2
    B, H, W, cin, s, nb = 1, 4, 4, 64, 32, 2
    for f in (lib.mssvt_head_conv_shared_dgrad_workspace_bytes, lib.mssvt_head_conv_shared_wgrad_workspace_bytes):
        assert f(1, 4, 4, 128, 32) == 0 and f(0, 4, 4, 64, 32) == 0 and f(1, 4, -4, 64, 32) == 0 and f(1, 4, 4, 64, 48) == 0
        assert f(1 << 15, 1 << 8, 1 << 8, 64, 32) == 0 and f(1 << 13, 1 << 8, 1 << 8, 64, 32) > 0
    for f in (lib.mssvt_head_conv_trunk_dgrad_workspace_bytes, lib.mssvt_head_conv_trunk_wgrad_workspace_bytes,
              lib.mssvt_head_conv_bgrad_workspace_bytes):
        assert f(1, 4, 4, 48, 2) == 0 and f(0, 4, 4, 32, 2) == 0 and f(1, 4, 4, 32, 0) == 0 and f(1, 4, 4, 32, 65) == 0
        assert f(1 << 15, 1 << 8, 1 << 8, 32, 2) == 0 and f(1, 4, 4, 32, 64) > 0
    x = torch.ones(B, H, W, cin, device=DEV)
    dy = torch.ones(B, H, W, s, device=DEV)
    w = torch.ones(s, cin, 3, 3, device=DEV)
    tw = [torch.ones(s, s, 3, 3, device=DEV) for _ in range(nb)]
    dts = [torch.ones(B, H, W, s, device=DEV) for _ in range(nb)]
    outs = {k: torch.full((n,), 7.0, device=DEV) for k, n in
            dict(y=B * H * W * s, e=B * H * W, dx=B * H * W * cin, dw=s * cin * 9, db=nb * s, t=nb * B * H * W * s, ty=B * H * W * s,
                 tw=nb * s * s * 9, ws=1 << 20).items()}
    blob = torch.zeros(int(lib.mssvt_head_conv_shared_pack_bytes(cin, s)), dtype=torch.uint8, device=DEV)
    tblob = torch.zeros(int(lib.mssvt_head_conv_trunk_pack_bytes(s, nb)), dtype=torch.uint8, device=DEV)
    p = {k: v.data_ptr() for k, v in outs.items()}
    X, DY, Wp, Y = x.data_ptr(), dy.data_ptr(), w.data_ptr(), dy.data_ptr()
    DT, TW = pointers(dts), pointers(tw)
    null2 = (ctypes.c_void_p * 2)(dts[0].data_ptr(), None)
    odd2 = (ctypes.c_void_p * 2)(dts[0].data_ptr(), dts[1].data_ptr() + 4)

    def variants(call, ptr_slots, size_slots, good, big_sizes):
        """`call(args)`; each pointer slot null and unaligned in turn, each size slot zero / negative: BADARG; big_sizes: TOOLARGE."""
        for k in ptr_slots:
            a = list(good)
            a[k] = None
            assert call(a) == BAD, ("null", k)
            if isinstance(good[k], int):
                a[k] = good[k] + 4
                assert call(a) == BAD, ("unaligned", k)
        for k in size_slots:
            for v in (0, -3):
                a = list(good)
                a[k] = v
                assert call(a) == BAD, ("size", k, v)
        for k, v in big_sizes:
            a = list(good)
            a[k] = v
            assert call(a) == BIG, ("big", k, v)

    # shared_train(x, B, H, W, cin, s, packed, exp_workspace, y, stream)
    good = [X, B, H, W, cin, s, blob.data_ptr(), p["e"], p["y"], st]
    variants(lambda a: lib.mssvt_head_conv_shared_train(*a), [0, 6, 8], [1, 2, 3, 4, 5], good, [(4, 128), (5, 48)])
    assert lib.mssvt_head_conv_shared_train(X, 1 << 15, 1 << 8, 1 << 8, cin, s, blob.data_ptr(), p["e"], p["y"], st) == BIG
    a = list(good)
    a[7] = None
    assert lib.mssvt_head_conv_shared_train(*a) == BAD
    # shared_dgrad(dy, weight, B, H, W, cin, s, dx, workspace, stream) / shared_wgrad(x, dy, ..., dw, workspace, stream)
    for f, g in ((lib.mssvt_head_conv_shared_dgrad, [DY, Wp, B, H, W, cin, s, p["dx"], p["ws"], st]),
                 (lib.mssvt_head_conv_shared_wgrad, [X, DY, B, H, W, cin, s, p["dw"], p["ws"], st])):
        variants(lambda a, f=f: f(*a), [0, 1, 7, 8], [2, 3, 4, 5, 6], g, [(5, 128), (6, 48)])
        a = list(g)
        a[2], a[3], a[4] = 1 << 15, 1 << 8, 1 << 8
        assert f(*a) == BIG
    # trunk_train(y, B, H, W, s, nb, packed, exp_workspace, t, stream)
    good = [Y, B, H, W, s, nb, tblob.data_ptr(), p["e"], p["t"], st]
    variants(lambda a: lib.mssvt_head_conv_trunk_train(*a), [0, 6, 8], [1, 2, 3, 4, 5], good, [(4, 48), (5, 65)])
    a = list(good)
    a[7] = None
    assert lib.mssvt_head_conv_trunk_train(*a) == BAD
    assert lib.mssvt_head_conv_trunk_train(Y, 1 << 15, 1 << 8, 1 << 8, s, nb, tblob.data_ptr(), p["e"], p["t"], st) == BIG
    # bgrad(host_dys, B, H, W, s, nb, db, workspace, stream)
    good = [DT, B, H, W, s, nb, p["db"], p["ws"], st]
    variants(lambda a: lib.mssvt_head_conv_bgrad(*a), [0, 6, 7], [1, 2, 3, 4, 5], good, [(4, 48), (5, 65)])
    # trunk_dgrad(host_dts, host_weights, B, H, W, s, nb, dy, workspace, stream)
    good = [DT, TW, B, H, W, s, nb, p["ty"], p["ws"], st]
    variants(lambda a: lib.mssvt_head_conv_trunk_dgrad(*a), [0, 1, 7, 8], [2, 3, 4, 5, 6], good, [(5, 48), (6, 65)])
    # trunk_wgrad(y, host_dts, B, H, W, s, nb, dw, workspace, stream)
    good = [Y, DT, B, H, W, s, nb, p["tw"], p["ws"], st]
    variants(lambda a: lib.mssvt_head_conv_trunk_wgrad(*a), [0, 1, 7, 8], [2, 3, 4, 5, 6], good, [(5, 48), (6, 65)])
    # a null or unaligned ENTRY of a pointer array
    for arr in (null2, odd2):
        assert lib.mssvt_head_conv_bgrad(arr, B, H, W, s, nb, p["db"], p["ws"], st) == BAD
        assert lib.mssvt_head_conv_trunk_dgrad(arr, TW, B, H, W, s, nb, p["ty"], p["ws"], st) == BAD
        assert lib.mssvt_head_conv_trunk_dgrad(DT, arr, B, H, W, s, nb, p["ty"], p["ws"], st) == BAD
        assert lib.mssvt_head_conv_trunk_wgrad(Y, arr, B, H, W, s, nb, p["tw"], p["ws"], st) == BAD
    torch.cuda.synchronize()
    assert all(bool((v == 7.0).all()) for v in outs.values())
    # and the good calls are MSSVT_OK (0)
    assert lib.mssvt_head_conv_shared_pack(Wp, None, None, None, None, None, 0.0, cin, s, blob.data_ptr(), st) == 0
    assert lib.mssvt_head_conv_shared_train(X, B, H, W, cin, s, blob.data_ptr(), p["e"], p["y"], st) == 0
    assert lib.mssvt_head_conv_shared_dgrad(DY, Wp, B, H, W, cin, s, p["dx"], p["ws"], st) == 0
    assert lib.mssvt_head_conv_shared_wgrad(X, DY, B, H, W, cin, s, p["dw"], p["ws"], st) == 0
    assert lib.mssvt_head_conv_bgrad(DT, B, H, W, s, nb, p["db"], p["ws"], st) == 0
    assert lib.mssvt_head_conv_trunk_dgrad(DT, TW, B, H, W, s, nb, p["ty"], p["ws"], st) == 0
    assert lib.mssvt_head_conv_trunk_wgrad(Y, DT, B, H, W, s, nb, p["tw"], p["ws"], st) == 0
    torch.cuda.synchronize()
    assert bool((outs["db"] == 16.0).all()) and bool((outs["y"][:s] == 4.0 * cin).all()) and not bool((outs["tw"] == 7.0).any())
    # the Python layer: no CPU path, channels-last fp32 only, covered shapes only
    good_x = torch.zeros(1, 64, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last)
    for wrong in (torch.zeros(1, 64, 4, 4, device=DEV), good_x.cpu(), good_x.double(), good_x[0]):
        with pytest.raises(MssvtHipError):
            hct.shared_forward(wrong, w)
    with pytest.raises(MssvtHipError):
        hct.shared_forward(good_x, torch.zeros(48, 64, 3, 3, device=DEV))
    with pytest.raises(MssvtHipError):
        hct.shared_forward(good_x, w.cpu())
    with pytest.raises(MssvtHipError):
        hct.shared_wgrad(good_x, torch.zeros(1, 32, 4, 5, device=DEV).contiguous(memory_format=torch.channels_last))
    with pytest.raises(MssvtHipError):
        hct.TrunkFunction.apply(torch.zeros(1, 32, 4, 4, device=DEV), 2, tw[0], tw[1], None)


# ---- the Functions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [NARROW, (512, 64)])
@pytest.mark.parametrize("input_grad,bias,nchw_grad", [(True, True, False), (False, True, False), (True, False, True)])
def test_shared_function_matches_the_statement_and_the_entry_points(shape, input_grad, bias, nchw_grad, monkeypatch):
    cin, s = shape
    B, H, W = 2, 9, 11
    xs, dys = tref.inputs("plain", B, H, W, cin, s, seed=cin + H)
    ws, bsv = ref.weights(s, cin, 2), bias_of(s, 3, bias)
    calls = []
    for name in ("shared_dgrad", "shared_wgrad", "bias_grad"):
        real = getattr(hct, name)
        monkeypatch.setattr(hct, name, lambda *a, _r=real, _n=name, **k: (calls.append(_n), _r(*a, **k))[1])
    # with nchw_grad the input is NCHW in memory as well: the Function makes it channels-last
    x = (nchw(xs).contiguous() if nchw_grad else nchw(xs)).requires_grad_(input_grad)
    w = dev(ws).requires_grad_(True)
    b = dev(bsv).requires_grad_(True) if bias else None
    y = hct.SharedFunction.apply(x, w, b)
    assert bev_conv.is_channels_last(y) and tuple(y.shape) == (B, s, H, W)
    inside(rows(y.detach()), ref.forward(xs, ws, bsv), "Function y")
    g = nchw(dys).contiguous() if nchw_grad else nchw(dys)
    y.backward(g)
    assert calls == (["shared_dgrad"] if input_grad else []) + ["shared_wgrad"] + (["bias_grad"] if bias else [])
    np.testing.assert_array_equal(w.grad.cpu().numpy(), wgrad(xs, dys))
    inside(w.grad.cpu().numpy(), ref.dw(xs, dys), "Function dW")
    if bias:
        np.testing.assert_array_equal(b.grad.cpu().numpy(), bgrad([dys])[0])
    if input_grad:
        assert bev_conv.is_channels_last(x.grad) == (not nchw_grad) and tuple(x.grad.shape) == (B, cin, H, W)
        np.testing.assert_array_equal(rows(x.grad), dgrad(dys, ws))
    else:
        assert x.grad is None


@pytest.mark.parametrize("s,nb", [(32, 2), (64, 5), (32, 1)])
@pytest.mark.parametrize("absent", [False, True])
def test_trunk_function_matches_the_statement_with_a_branch_absent_or_not(s, nb, absent):
    """The outputs are dense views of ONE buffer; with `absent` the last branch takes no part in the loss: its upstream gradient
    counts as zero (dW_b = 0, db_b = 0, no term in dy)."""
    B, H, W = 2, 7, 9
    ys, dts, wsv = trunk_inputs("plain", B, H, W, s, nb, seed=s + nb)
    bsv = [bias_of(s, b, b % 2 == 0) for b in range(nb)]
    y = nchw(ys).requires_grad_(True)
    ws = [dev(v).requires_grad_(True) for v in wsv]
    bs = [None if v is None else dev(v).requires_grad_(True) for v in bsv]
    outs = hct.TrunkFunction.apply(y, nb, *(ws + bs))
    assert len(outs) == nb and all(tuple(t.shape) == (B, s, H, W) and bev_conv.is_channels_last(t) for t in outs)
    step = B * H * W * s * 4
    assert [t.data_ptr() - outs[0].data_ptr() for t in outs] == [b * step for b in range(nb)]
    for b, (t, want) in enumerate(zip(outs, ref.trunk_forward(ys, wsv, bsv))):
        inside(rows(t.detach()), want, "Function t_%d" % b)
    used = nb - 1 if absent and nb > 1 else nb
    if used < nb:
        dts[-1] = np.zeros_like(dts[-1])
    torch.autograd.backward(list(outs[:used]), [nchw(d) for d in dts[:used]])
    inside(rows(y.grad), ref.trunk_dy(dts, wsv), "Function dy")
    np.testing.assert_array_equal(rows(y.grad), t_dgrad(dts, wsv))
    want_w, want_b = t_wgrad(ys, dts), bgrad(dts)
    for b in range(nb):
        np.testing.assert_array_equal(ws[b].grad.cpu().numpy(), want_w[b])
        inside(ws[b].grad.cpu().numpy(), ref.dw(ys, dts[b]), "Function dW_%d" % b)
        if bs[b] is not None:
            np.testing.assert_array_equal(bs[b].grad.cpu().numpy(), want_b[b])
    if used < nb:
        assert not bool(ws[-1].grad.any())
