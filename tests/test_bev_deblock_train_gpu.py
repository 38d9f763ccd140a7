"""mssvt_bev_deblock_wgrad / mssvt_bev_deblock_dgrad (csrc/bev_conv.hip, kernels in csrc/split_wgrad.hip.h and
csrc/split_conv.hip.h) and ``bev_deblock_train.DeblockFunction`` against the float64 statement and the bounds of
tests/bev_deblock_train_ref.py (its docstring states them; tests/bev_conv_train_ref.py derives the weight gradient's)."""
import numpy as np
import pytest
import torch
from torch import nn

from mssvt_amd import _lib, bev_conv, bev_deblock_train as bdt
from mssvt_amd._lib import MssvtHipError
from tests import bev_deblock_train_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = ref.SHAPES
NARROW = [(1, 32, 64), (2, 64, 32)]
PRODUCT = [(1, 128, 256), (2, 256, 256)]
FIXED_SIZES = [(1, 1, 1), (1, 2, 3), (3, 5, 7), (1, 1, 31), (1, 1, 32), (1, 1, 33), (2, 15, 17)]
KINDS = ("plain", "tail", "spike")


def grid_of(n):
    """(1, H, W) with H W = n and W the odd divisor of n nearest to sqrt(n)."""
    w = min((d for d in range(1, n + 1, 2) if n % d == 0), key=lambda d: abs(d - n ** 0.5))
    return (1, n // w, w)


def slice_counts(shape):
    sl = ref.SLICE_PIXELS[shape]
    if shape in NARROW:
        return [sl - 1, sl, sl + 1, 2 * sl - 1, 2 * sl + 1, 3 * sl + 1]
    return [sl - 1, sl + 1, 2 * sl - 1, 2 * sl + 1]


SLICE_CASES = [(shape, n) for shape in SHAPES for n in slice_counts(shape)]


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).permute(0, 3, 1, 2)


def wgrad(x, dy, s, workspace=None):
    """x (B, H, W, cin), dy (B, s H, s W, cout) host arrays -> dw (cin, cout, s, s) numpy through the C entry point."""
    return bdt.deblock_wgrad(nchw(x), nchw(dy), s, workspace).cpu().numpy()


def dgrad(dy, w, s, workspace=None):
    """dy (B, s H, s W, cout), w (cin, cout, s, s) host arrays -> dx (B, H, W, cin) numpy through the C entry point."""
    return bdt.deblock_dgrad(nchw(dy), torch.from_numpy(w).to(DEV), s, workspace).permute(0, 2, 3, 1).cpu().numpy()


def check_dw(x, dy, shape, tag):
    s = shape[0]
    got = wgrad(x, dy, s)
    want = ref.dw_ref(x, dy, s)
    bound = ref.dw_bound(x, dy, s, bdt.slice_pixels(*shape))
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("dW %s %s: worst error / bound %.3f" % (shape, tag, ratio))
    assert got.shape == want.shape and (err <= bound).all(), (tag, ratio)
    return ratio


def check_dx(dy, w, shape, tag):
    s = shape[0]
    got = dgrad(dy, w, s)
    want, _, bound = ref.dx_ref(dy, w, s)
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("dX %s %s: worst error / bound %.3f" % (shape, tag, ratio))
    assert got.shape == want.shape and (err <= bound).all(), (tag, ratio)
    return ratio


def test_the_slice_rule_and_the_workspaces_are_as_published():
    lib = _lib.lib()
    r256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for shape in SHAPES:
        s, cin, cout = shape
        assert lib.mssvt_bev_deblock_train_supported(*shape) == 1
        sl = bdt.slice_pixels(*shape)
        assert sl == ref.SLICE_PIXELS[shape]
        for B, H, W in ((1, 3, sl), (1, 1, 3 * sl + 1), (2, 5, 7)):
            M = B * H * W
            slices = -(-M // sl)
            assert bdt.wgrad_workspace_bytes(B, H, W, *shape) == r256(4 * M) + r256(4 * s * s * M) + slices * s * s * cin * cout * 4
            assert bdt.dgrad_workspace_bytes(B, H, W, *shape) == r256(4 * s * s * M) + 64 + 8 * cin + 4 * s * s * cin * cout
    assert [bdt.slice_pixels(*shape) for shape in SHAPES] == [1024, 2048, 256, 256]


# ---- the weight gradient -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("i", range(len(FIXED_SIZES)))
def test_dw_error_bound_at_the_small_sizes(i, shape):
    B, H, W = FIXED_SIZES[i]
    kind = KINDS[i % 3]
    x, dy = ref.inputs(kind, B, H, W, *shape, seed=100 * i + shape[1])
    check_dw(x, dy, shape, "%s %s" % ((B, H, W), kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(SLICE_CASES)))
def test_dw_error_bound_either_side_of_the_slices(i, kind):
    shape, n = SLICE_CASES[i]
    B, H, W = grid_of(n)
    assert W % 2 == 1 and H * W == n
    x, dy = ref.inputs(kind, B, H, W, *shape, seed=7 * i + shape[2])
    check_dw(x, dy, shape, "%s %s" % ((B, H, W), kind))


@pytest.mark.parametrize("shape", NARROW + [(1, 128, 256)])
def test_dw_a_slice_may_span_two_samples(shape):
    sl = bdt.slice_pixels(*shape)
    H, W = 9, sl // 12  # 3 samples of ~0.75 slices: slice 0 ends inside sample 1, slice 1 inside sample 2
    assert ref.num_slices(3 * H * W, sl) == 3 and H * W < sl
    x, dy = ref.inputs("plain", 3, H, W, *shape, seed=5)
    check_dw(x, dy, shape, "spanning")


@pytest.mark.parametrize("shape", SHAPES)
def test_dw_impulse_against_impulse_lands_on_the_single_right_element(shape):
    """x holds one value at one pixel and channel, dy one at one pixel of its 2 x 2 (or 1 x 1) patch: dw is EXACTLY their product
    at that (c, n, dy, dx) and exactly zero everywhere else.  3 x 5: both fp16-exact, the product is 15.  (1 + 2^-12) x (1 + 2^-13):
    hi = 1 and lo = 2^-12 / 2^-13 exactly, so hi hi = 1 and the cross terms 2^-12 + 2^-13 are exact and the kernel's result is
    1 + 2^-12 + 2^-13 -- the float32 rounding of the product, whose dropped lo lo term 2^-25 is a quarter of an ulp.  A dropped
    cross term is 2048 / 1024 ulp off, a misplaced rounding or un-normalisation one."""
    s, cin, cout = shape
    B, H, W, c, n = 2, 5, 7, 5, cout - 3
    pairs = [(3.0, 5.0), (1.0 + 2.0 ** -12, 1.0 + 2.0 ** -13)]
    assert np.float32(pairs[1][0] * pairs[1][1]) == np.float32(1.0 + 2.0 ** -12 + 2.0 ** -13)
    places = [(0, 0, 0), (1, H - 1, W - 1), (0, 0, 3), (1, 2, 0), (1, 2, 3)]  # corners, edges, interior
    for k, (b, iy, ix) in enumerate(places if shape in NARROW else [places[1], places[3], places[4]]):
        for py, px in ref.phases(s):
            vx, vd = pairs[(k + py + px) % 2]
            x, dy = np.zeros((B, H, W, cin), np.float32), np.zeros((B, s * H, s * W, cout), np.float32)
            x[b, iy, ix, c] = vx
            dy[b, s * iy + py, s * ix + px, n] = vd
            got = wgrad(x, dy, s)
            want = np.zeros((cin, cout, s, s), np.float32)
            want[c, n, py, px] = np.float32(vx * vd)
            np.testing.assert_array_equal(want, ref.dw_ref(x, dy, s).astype(np.float32))
            np.testing.assert_array_equal(got, want, err_msg=str((b, iy, ix, py, px, vx, vd)))
            # the impulse of dy one pixel off its patch meets nothing
            if s == 2 and ix + 1 < W:
                dy2 = np.zeros_like(dy)
                dy2[b, s * iy + py, s * (ix + 1) + px, n] = 1.0
                assert (wgrad(x, dy2, s) == 0.0).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_dw_power_of_two_scaling_of_either_operand_is_exact(shape):
    s = shape[0]
    sl = bdt.slice_pixels(*shape)
    B, H, W = grid_of(sl + sl // 2 + 1)  # two slices
    x, dy = ref.inputs("plain", B, H, W, *shape, seed=3)
    base = wgrad(x, dy, s)
    for p in (18, -20):
        f = np.float32(2.0 ** p)
        assert np.array_equal(wgrad(x * f, dy, s), base * f), p
        assert np.array_equal(wgrad(x, dy * f, s), base * f), p
    assert np.array_equal(wgrad(x * np.float32(2.0 ** 40), dy * np.float32(2.0 ** -37), s), base * np.float32(8.0))


@pytest.mark.parametrize("shape", SHAPES)
def test_dw_non_finite_inputs_never_come_out_finite(shape):
    s, cin, cout = shape
    x, dy = ref.inputs("plain", 2, 12, 30, *shape, seed=8)  # 720 input pixels: three slices of the narrow shapes
    x[0, 2, 3, 5] = np.nan
    x[1, 4, 8, 31] = np.inf
    dy[1, s * 12 - 1, s * 30 - 1, 7] = -np.inf
    dy[0, 0, 0, 9] = np.nan
    got = wgrad(x, dy, s)
    with np.errstate(invalid="ignore", over="ignore"):
        want = ref.dw_ref(x, dy, s)
    bad = ~np.isfinite(want)
    assert bad.sum() > 0 and not np.isfinite(got[bad]).any()
    clean = np.isfinite(want)
    assert clean.sum() > 0 and np.isfinite(got[clean]).all()  # (elements no bad value reaches stay finite at this range)


# ---- the input gradient ---------------------------------------------------------------------------------------------------
DX_SIZES = [(1, 1, 31), (1, 32, 1), (1, 3, 11), (1, 17, 15), (1, 256, 1), (1, 1, 257), (2, 3, 5)]  # (2, 3, 5): 15 pixels a sample


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("i", range(len(DX_SIZES)))
def test_dx_error_bound(i, shape):
    B, H, W = DX_SIZES[i]
    assert W % 2 == 1
    kind = KINDS[i % 3]
    _, dy = ref.inputs(kind, B, H, W, *shape, seed=11 * i + shape[1])
    check_dx(dy, ref.weights(*shape, seed=i), shape, "%s %s" % ((B, H, W), kind))


@pytest.mark.parametrize("shape", SHAPES)
def test_dx_impulse_reads_the_single_right_weights(shape):
    """A unit impulse of dy at (b, s iy + dy, s ix + dx, n) gives dx[b, iy, ix, :] = w[:, n, dy, dx] within 1 ulp and exact zeros
    everywhere else.  The weights are planted as in tests/test_bev_up2_gpu.py: w[c, n, dy, dx] = +-(1 + q / 64)(1 + 2^-13) with q
    and the sign functions of (c, n, dy, dx), so a value read from another channel or phase is another number, and every weight
    has hi = +-(1 + q / 64) and a non-zero lo that the split carries exactly (an arbitrary float32 weight is carried to 22 bits
    only: that is the error bound's business, not this test's)."""
    s, cin, cout = shape
    B, H, W, n = 2, 3, 5, cout - 5
    c_, n_, py_, px_ = np.meshgrid(np.arange(cin), np.arange(cout), np.arange(s), np.arange(s), indexing="ij")
    q = (7 * c_ + 3 * n_ + 13 * (2 * py_ + px_)) % 64
    w = (np.where((c_ + n_ + py_ + px_) % 2, -1.0, 1.0) * (1.0 + q / 64.0) * (1.0 + 2.0 ** -13)).astype(np.float32)
    assert np.array_equal(w.astype(np.float64), np.where((c_ + n_ + py_ + px_) % 2, -1.0, 1.0) * (1.0 + q / 64.0) * (1.0 + 2.0 ** -13))
    assert len({float(w[3, n, py, px]) for py, px in ref.phases(s)}) == s * s
    for b, iy, ix in [(0, 0, 0), (1, H - 1, W - 1), (0, 1, 0), (1, 1, 2)]:
        for py, px in ref.phases(s):
            dy = np.zeros((B, s * H, s * W, cout), np.float32)
            dy[b, s * iy + py, s * ix + px, n] = 1.0
            got = dgrad(dy, w, s)
            col = w[:, n, py, px]
            assert (np.abs(got[b, iy, ix] - col) <= np.spacing(np.abs(col))).all(), (b, iy, ix, py, px)
            got[b, iy, ix] = 0.0
            assert (got == 0.0).all(), (b, iy, ix, py, px)


@pytest.mark.parametrize("shape", SHAPES)
def test_dx_power_of_two_scaling_is_exact(shape):
    s = shape[0]
    _, dy = ref.inputs("plain", 2, 7, 9, *shape, seed=4)
    w = ref.weights(*shape, seed=5)
    base = dgrad(dy, w, s)
    for p in (18, -20):
        f = np.float32(2.0 ** p)
        assert np.array_equal(dgrad(dy * f, w, s), base * f), p
        assert np.array_equal(dgrad(dy, w * f, s), base * f), p


# ---- both entry points -----------------------------------------------------------------------------------------------------
def guarded(values, guard=4096):
    n = values.size
    big = torch.full((n + 2 * guard,), float("nan"), device=DEV)
    big[guard:guard + n] = torch.from_numpy(values).to(DEV).reshape(-1)
    return big, big[guard:guard + n]


def guards_intact(big, n, guard=4096):
    return bool(torch.isnan(big[:guard]).all()) and bool(torch.isnan(big[guard + n:]).all())


@pytest.mark.parametrize("shape,hw", [((1, 128, 256), (17, 19)), ((2, 64, 32), (6, 51)), ((2, 256, 256), (3, 5)), ((1, 32, 64), (9, 31))])
def test_reads_stay_inside_the_inputs_and_every_output_element_is_written(shape, hw):
    """Inputs are slices of NaN-filled allocations (a read outside them poisons the result); outputs and the NaN-prefilled
    workspaces sit in NaN-filled allocations: outputs fully written, the guards untouched, the bits those of a tight run and
    of a run on a zeroed workspace."""
    s, cin, cout = shape
    B, (H, W) = 2, hw
    xs, dys = ref.inputs("plain", B, H, W, *shape, seed=6)
    w = ref.weights(*shape, seed=7)
    guard = 4096
    xbig, x = guarded(xs)
    dbig, dyv = guarded(dys)
    wtbig, wt = guarded(w)
    # dW
    ndw = w.size
    wbig = torch.full((ndw + 2 * guard,), float("nan"), device=DEV)
    nws = bdt.wgrad_workspace_bytes(B, H, W, *shape)
    assert nws % 4 == 0
    wsbig = torch.full((nws // 4 + 2 * guard,), float("nan"), device=DEV)
    _lib.call("mssvt_bev_deblock_wgrad", x.data_ptr(), dyv.data_ptr(), B, H, W, cin, cout, s, wbig[guard:guard + ndw].data_ptr(),
              wsbig[guard:guard + nws // 4].data_ptr(), _lib.stream())
    got = wbig[guard:guard + ndw].view(cin, cout, s, s).cpu().numpy()
    assert np.isfinite(got).all()
    for big, n in ((wbig, ndw), (wsbig, nws // 4), (xbig, xs.size), (dbig, dys.size)):
        assert guards_intact(big, n)
    np.testing.assert_array_equal(got, wgrad(xs, dys, s))
    np.testing.assert_array_equal(got, wgrad(xs, dys, s, torch.zeros(nws, dtype=torch.uint8, device=DEV)))
    # dX
    ndx = xs.size
    xgbig = torch.full((ndx + 2 * guard,), float("nan"), device=DEV)
    nds = bdt.dgrad_workspace_bytes(B, H, W, *shape)
    assert nds % 4 == 0
    dsbig = torch.full((nds // 4 + 2 * guard,), float("nan"), device=DEV)
    _lib.call("mssvt_bev_deblock_dgrad", dyv.data_ptr(), wt.data_ptr(), B, H, W, cin, cout, s, xgbig[guard:guard + ndx].data_ptr(),
              dsbig[guard:guard + nds // 4].data_ptr(), _lib.stream())
    gotx = xgbig[guard:guard + ndx].view(B, H, W, cin).cpu().numpy()
    assert np.isfinite(gotx).all()
    for big, n in ((xgbig, ndx), (dsbig, nds // 4), (dbig, dys.size), (wtbig, w.size)):
        assert guards_intact(big, n)
    np.testing.assert_array_equal(gotx, dgrad(dys, w, s))
    np.testing.assert_array_equal(gotx, dgrad(dys, w, s, torch.zeros(nds, dtype=torch.uint8, device=DEV)))


@pytest.mark.parametrize("shape", SHAPES)
def test_bit_identical_across_calls_and_streams(shape):
    s = shape[0]
    sl = bdt.slice_pixels(*shape)
    xs, dys = ref.inputs("plain", 2, 25, (sl + 100) // 25, *shape, seed=12)  # three slices
    x, dy, w = nchw(xs), nchw(dys), torch.from_numpy(ref.weights(*shape, seed=1)).to(DEV)
    first = (bdt.deblock_wgrad(x, dy, s), bdt.deblock_dgrad(dy, w, s))
    again = (bdt.deblock_wgrad(x, dy, s), bdt.deblock_dgrad(dy, w, s))
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            outs.append((bdt.deblock_wgrad(x, dy, s), bdt.deblock_dgrad(dy, w, s)))
        st.synchronize()
    for o in [again] + outs:
        assert torch.equal(first[0], o[0]) and torch.equal(first[1], o[1])


def test_the_backward_never_synchronises_the_host():
    shape = (2, 64, 32)
    xs, dys = ref.inputs("plain", 2, 9, 41, *shape, seed=15)
    x, dy, w = nchw(xs), nchw(dys), torch.from_numpy(ref.weights(*shape, seed=2)).to(DEV)
    warm = (bdt.deblock_wgrad(x, dy, 2), bdt.deblock_dgrad(dy, w, 2))
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
            out = (bdt.deblock_wgrad(x, dy, 2), bdt.deblock_dgrad(dy, w, 2))
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    assert torch.equal(warm[0], out[0]) and torch.equal(warm[1], out[1])


def test_every_status_code_is_reached_and_nothing_is_launched():
    lib = _lib.lib()
    for bad in [(1, 256, 256), (2, 128, 256), (1, 64, 32), (2, 32, 64), (3, 32, 64), (0, 32, 64), (1, 48, 48), (2, 512, 512)]:
        assert lib.mssvt_bev_deblock_train_supported(*bad) == 0, bad
        assert lib.mssvt_bev_deblock_wgrad_slice_pixels(*bad) == 0, bad
    for f in (lib.mssvt_bev_deblock_wgrad_workspace_bytes, lib.mssvt_bev_deblock_dgrad_workspace_bytes):
        assert f(1, 4, 4, 1, 48, 48) == 0 and f(0, 4, 4, 1, 32, 64) == 0 and f(1, 4, -4, 2, 64, 32) == 0
        assert f(1 << 15, 1 << 8, 1 << 8, 1, 32, 64) == 0  # 2^31 pixels
        assert f(1 << 13, 1 << 8, 1 << 8, 2, 64, 32) == 0  # 2^29 input pixels: 2^31 pixels of dy
        assert f(1 << 13, 1 << 8, 1 << 8, 1, 32, 64) > 0
    x = torch.ones(1, 4, 4, 32, device=DEV)
    dy = torch.ones(1, 4, 4, 64, device=DEV)
    w = torch.ones(32, 64, 1, 1, device=DEV)
    dw = torch.full((32, 64, 1, 1), 7.0, device=DEV)
    dx = torch.full((1, 4, 4, 32), 7.0, device=DEV)
    ws = torch.full((max(bdt.wgrad_workspace_bytes(1, 4, 4, 1, 32, 64), bdt.dgrad_workspace_bytes(1, 4, 4, 1, 32, 64)) // 4,), 7.0, device=DEV)
    st = _lib.stream()
    BAD, BIG = -1, -2
    for f, a, b, out in ((lib.mssvt_bev_deblock_wgrad, x.data_ptr(), dy.data_ptr(), dw.data_ptr()),
                         (lib.mssvt_bev_deblock_dgrad, dy.data_ptr(), w.data_ptr(), dx.data_ptr())):
        sp = ws.data_ptr()
        assert f(None, b, 1, 4, 4, 32, 64, 1, out, sp, st) == BAD
        assert f(a, None, 1, 4, 4, 32, 64, 1, out, sp, st) == BAD
        assert f(a, b, 1, 4, 4, 32, 64, 1, None, sp, st) == BAD
        assert f(a, b, 1, 4, 4, 32, 64, 1, out, None, st) == BAD
        assert f(a, b, 0, 4, 4, 32, 64, 1, out, sp, st) == BAD
        assert f(a, b, 1, 4, -4, 32, 64, 1, out, sp, st) == BAD
        assert f(a, b, 1, 4, 4, 32, 64, 0, out, sp, st) == BAD
        assert f(a, b, 1, 4, 4, 0, 64, 1, out, sp, st) == BAD
        for k in range(4):  # each pointer unaligned in turn
            ptrs = [a, b, out, sp]
            ptrs[k] += 4
            assert f(ptrs[0], ptrs[1], 1, 4, 4, 32, 64, 1, ptrs[2], ptrs[3], st) == BAD, k
        assert f(a, b, 1, 4, 4, 48, 48, 1, out, sp, st) == BIG
        assert f(a, b, 1, 4, 4, 64, 32, 1, out, sp, st) == BIG
        assert f(a, b, 1, 4, 4, 32, 64, 2, out, sp, st) == BIG
        assert f(a, b, 1, 4, 4, 32, 64, 3, out, sp, st) == BIG
        assert f(a, b, 1 << 15, 1 << 8, 1 << 8, 32, 64, 1, out, sp, st) == BIG  # 2^31 pixels
        assert f(a, b, 1 << 13, 1 << 8, 1 << 8, 64, 32, 2, out, sp, st) == BIG  # 2^31 pixels of dy
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((dx == 7.0).all()) and bool((ws == 7.0).all())
    # the Python layer: no CPU path, channels-last fp32 only
    xc = torch.zeros(1, 32, 4, 4, device=DEV)
    good = xc.contiguous(memory_format=torch.channels_last)
    gy = torch.zeros(1, 64, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last)
    for wrong in (xc, good.cpu(), good.double(), xc[0]):
        with pytest.raises(MssvtHipError):
            bdt.deblock_wgrad(wrong, gy, 1)
    with pytest.raises(MssvtHipError):
        bdt.deblock_wgrad(good, gy, 2)  # dy is not (2 H, 2 W)
    with pytest.raises(MssvtHipError):
        bdt.deblock_wgrad(good, gy, 1, torch.zeros(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(MssvtHipError):
        bdt.deblock_dgrad(gy, w.cpu(), 1)
    with pytest.raises(MssvtHipError):
        bdt.deblock_dgrad(gy, torch.zeros(32, 64, 2, 2, device=DEV), 1)
    with pytest.raises(MssvtHipError):
        bdt.deblock_dgrad(gy, w, 1, torch.zeros(16, dtype=torch.uint8, device=DEV))


# ---- the Function and the predicates -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("input_grad,nchw_grad", [(True, False), (False, False), (True, True)])
def test_function_matches_the_statement(shape, input_grad, nchw_grad):
    s, cin, cout = shape
    B, H, W = 2, 9, 11
    xs, dys = ref.inputs("plain", B, H, W, *shape, seed=cin + s)
    ws = ref.weights(*shape, seed=cout)
    x = nchw(xs).requires_grad_(input_grad)
    w = torch.from_numpy(ws).to(DEV).requires_grad_(True)
    y = bdt.DeblockFunction.apply(x, w, s)
    assert bev_conv.is_channels_last(y) and tuple(y.shape) == (B, cout, s * H, s * W)
    want_y, _, bound_y = ref.y_ref(xs, ws, s)
    err = np.abs(y.detach().permute(0, 2, 3, 1).cpu().numpy() - want_y)
    print("y %s: worst error / bound %.3f" % (shape, float((err / np.maximum(bound_y, 1e-300)).max())))
    assert (err <= bound_y).all()
    g = nchw(dys)
    if nchw_grad:
        g = g.contiguous()
        assert not bev_conv.is_channels_last(g)
    y.backward(g)
    dw = w.grad.cpu().numpy()
    assert (np.abs(dw - ref.dw_ref(xs, dys, s)) <= ref.dw_bound(xs, dys, s, bdt.slice_pixels(*shape))).all()
    np.testing.assert_array_equal(dw, wgrad(xs, dys, s))
    if not input_grad:
        assert x.grad is None
        return
    want_dx, _, bound_dx = ref.dx_ref(dys, ws, s)
    assert bev_conv.is_channels_last(x.grad)
    assert (np.abs(x.grad.permute(0, 2, 3, 1).cpu().numpy() - want_dx) <= bound_dx).all()


def test_function_makes_an_nchw_input_channels_last_and_refuses_an_uncovered_shape():
    shape = (1, 32, 64)
    xs, dys = ref.inputs("plain", 1, 4, 5, *shape, seed=1)
    w = torch.from_numpy(ref.weights(*shape, seed=2)).to(DEV).requires_grad_(True)
    x = nchw(xs).contiguous().requires_grad_(True)
    assert not bev_conv.is_channels_last(x)
    y = bdt.DeblockFunction.apply(x, w, 1)
    y.backward(nchw(dys))
    want_dx, _, bound_dx = ref.dx_ref(dys, w.detach().cpu().numpy(), 1)
    assert (np.abs(x.grad.permute(0, 2, 3, 1).cpu().numpy() - want_dx) <= bound_dx).all()
    with pytest.raises(MssvtHipError):
        bdt.DeblockFunction.apply(x, torch.zeros(32, 48, 1, 1, device=DEV), 1)
    with pytest.raises(MssvtHipError):
        bdt.DeblockFunction.apply(x, w, 2)


def test_routing_predicates(monkeypatch):
    for s, cin, cout in SHAPES:
        ok = nn.ConvTranspose2d(cin, cout, s, stride=s, bias=False).to(DEV)
        assert bdt.deblock_shape(ok) == (s, cin, cout) and bdt.deblock_train_supported(ok)
        assert bdt.deblock_train_routed(ok) == ((s, cin, cout) in bdt.ROUTED_DEBLOCK_TRAIN or (s, cin, cout) in NARROW)
    for no in (nn.ConvTranspose2d(32, 64, 1, stride=1, bias=True), nn.ConvTranspose2d(64, 32, 2, stride=2, padding=1, bias=False),
               nn.ConvTranspose2d(64, 32, 2, stride=1, bias=False), nn.ConvTranspose2d(64, 32, 3, stride=2, bias=False),
               nn.ConvTranspose2d(64, 32, 2, stride=2, output_padding=1, bias=False), nn.ConvTranspose2d(64, 32, 4, stride=4, bias=False),
               nn.ConvTranspose2d(32, 64, 1, stride=1, groups=2, bias=False), nn.ConvTranspose2d(48, 48, 1, bias=False),
               nn.ConvTranspose2d(64, 32, 1, bias=False), nn.ConvTranspose2d(512, 512, 1, bias=False),
               nn.Conv2d(32, 64, 1, bias=False)):
        assert not bdt.deblock_train_supported(no.to(DEV)) and not bdt.deblock_train_routed(no.to(DEV)), no
    assert not bdt.deblock_train_supported(nn.ConvTranspose2d(32, 64, 1, bias=False))  # parameters on the CPU
    assert not bdt.deblock_train_supported(nn.ConvTranspose2d(32, 64, 1, bias=False).to(DEV).double())
    wide = nn.ConvTranspose2d(128, 256, 1, bias=False).to(DEV)
    monkeypatch.setattr(bdt, "ROUTED_DEBLOCK_TRAIN", frozenset())
    assert bdt.deblock_train_supported(wide) and not bdt.deblock_train_routed(wide)
    monkeypatch.setattr(bdt, "ROUTED_DEBLOCK_TRAIN", frozenset({(1, 128, 256)}))
    assert bdt.deblock_train_routed(wide)
