"""mssvt_bev_down_wgrad / mssvt_bev_down_dgrad (csrc/bev_conv.hip, kernels in csrc/split_wgrad.hip.h and
csrc/split_conv.hip.h) and ``bev_down_train.DownFunction`` against the float64 statement and the bounds of
tests/bev_down_train_ref.py (its docstring states them; tests/bev_conv_train_ref.py derives the weight gradient's)."""
import numpy as np
import pytest
import torch
from torch import nn

from mssvt_amd import _lib, bev_conv, bev_down_train as bdn
from mssvt_amd._lib import MssvtHipError
from tests import bev_down_train_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = ref.SHAPES
NARROW = (32, 64)
PRODUCT = (128, 256)
KINDS = ("plain", "tail", "spike")
# (B, H, W) of the INPUT.  The wave tile of the input-gradient kernel is 32 pixels of a phase and the workgroup tile 256:
# empty phases | small grids, two samples | 31 / 32 / 33 pixels per phase | 240 .. 272 pixels per phase | a tile spanning samples
EDGE_SIZES = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (1, 2, 2), (1, 3, 5), (2, 5, 4), (1, 2, 63), (1, 2, 64), (1, 2, 66),
              (1, 32, 32), (1, 31, 33), (1, 32, 34), (3, 7, 9)]
SMALL_SIZES = EDGE_SIZES[:6] + [(3, 7, 9)]


def grid_of(n):
    """(Ho, Wo) with Ho Wo = n and Wo the odd divisor of n nearest to sqrt(n)."""
    w = min((d for d in range(1, n + 1, 2) if n % d == 0), key=lambda d: abs(d - n ** 0.5))
    return (n // w, w)


def slice_counts(shape):
    sl = ref.SLICE_PIXELS[shape]
    if shape == NARROW:
        return [sl - 1, sl, sl + 1, 2 * sl - 1, 2 * sl + 1, 3 * sl + 1]
    return [sl - 1, sl + 1, 2 * sl - 1, 2 * sl + 1]


SLICE_CASES = [(shape, n) for shape in SHAPES for n in slice_counts(shape)]


def nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).permute(0, 3, 1, 2)


def wgrad(x, dy, workspace=None):
    """x (B, H, W, cin), dy (B, Ho, Wo, cout) host arrays -> dw (cout, cin, 3, 3) numpy through the C entry point."""
    return bdn.down_wgrad(nchw(x), nchw(dy), workspace).cpu().numpy()


def dgrad(dy, w, H, W, workspace=None):
    """dy (B, Ho, Wo, cout), w (cout, cin, 3, 3) host arrays -> dx (B, H, W, cin) numpy through the C entry point."""
    return bdn.down_dgrad(nchw(dy), torch.from_numpy(w).to(DEV), H, W, workspace).permute(0, 2, 3, 1).cpu().numpy()


def check_dw(x, dy, shape, tag):
    got = wgrad(x, dy)
    want = ref.dw_ref(x, dy)
    bound = ref.dw_bound(x, dy, bdn.slice_pixels(*shape))
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("dW %s %s: worst error / bound %.3f" % (shape, tag, ratio))
    assert got.shape == want.shape and (err <= bound).all(), (tag, ratio)
    return ratio


def check_dx(dy, w, H, W, shape, tag):
    got = dgrad(dy, w, H, W)
    want, _, bound = ref.dx_phases(dy, w, H, W)
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("dX %s %s: worst error / bound %.3f" % (shape, tag, ratio))
    assert got.shape == want.shape and (err <= bound).all(), (tag, ratio)
    return ratio


def test_the_slice_rule_and_the_workspaces_are_as_published():
    lib = _lib.lib()
    r256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for shape in SHAPES:
        cin, cout = shape
        assert lib.mssvt_bev_down_train_supported(*shape) == 1 and lib.mssvt_bev_conv_supported(3, cin, cout, 2, 1) == 1
        sl = bdn.slice_pixels(*shape)
        assert sl == ref.SLICE_PIXELS[shape]
        for B, H, W in ((1, 3, 2 * sl), (1, 1, 6 * sl + 1), (2, 5, 7), (1, 1, 1), (3, 6, 6)):
            Ho, Wo = ref.out_size(H, W)
            M = B * Ho * Wo
            slices = -(-M // sl)
            assert bdn.wgrad_workspace_bytes(B, H, W, *shape) == r256(4 * B * H * W) + r256(4 * M) + slices * 9 * cin * cout * 4
            assert bdn.dgrad_workspace_bytes(B, H, W, *shape) == r256(4 * M) + 64 + 8 * cin + 36 * cin * cout
    assert [bdn.slice_pixels(*shape) for shape in SHAPES] == [2048, 256]


# ---- the weight gradient -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("i", range(len(SMALL_SIZES)))
def test_dw_error_bound_at_the_small_sizes(i, shape):
    B, H, W = SMALL_SIZES[i]
    kind = KINDS[i % 3]
    x, dy = ref.inputs(kind, B, H, W, *shape, seed=100 * i + shape[1])
    check_dw(x, dy, shape, "%s %s" % ((B, H, W), kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(SLICE_CASES)))
def test_dw_error_bound_either_side_of_the_slices(i, kind):
    shape, n = SLICE_CASES[i]
    Ho, Wo = grid_of(n)
    assert Wo % 2 == 1 and Ho * Wo == n
    H, W = 2 * Ho - 1, 2 * Wo  # an odd and an even input size with that output grid
    assert ref.out_size(H, W) == (Ho, Wo)
    x, dy = ref.inputs(kind, 1, H, W, *shape, seed=7 * i + shape[1])
    check_dw(x, dy, shape, "%s -> %s %s" % ((1, H, W), (Ho, Wo), kind))


@pytest.mark.parametrize("shape", SHAPES)
def test_dw_a_slice_may_span_two_samples(shape):
    sl = bdn.slice_pixels(*shape)
    Ho, Wo = 9, sl // 12  # samples of ~0.75 slices: slice 0 ends inside sample 1
    B = 2 if shape == PRODUCT else 3
    assert ref.num_slices(B * Ho * Wo, sl) == B and Ho * Wo < sl
    x, dy = ref.inputs("plain", B, 2 * Ho, 2 * Wo - 1, *shape, seed=5)
    assert dy.shape[1:3] == (Ho, Wo)
    check_dw(x, dy, shape, "spanning")


IMPULSE_SIZES = [(5, 7), (4, 6), (5, 6)]  # odd x odd, even x even, odd x even


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("hw", IMPULSE_SIZES)
def test_dw_impulse_against_impulse_lands_on_the_single_right_element(shape, hw):
    """x holds one value at one pixel and channel, dy one at one output pixel and channel: dw is EXACTLY their product at the one
    tap (ky, kx) = (iy - 2 oy + 1, ix - 2 ox + 1) that joins them and exactly zero everywhere else; zero everywhere if no tap
    joins them.  3 x 5: both fp16-exact, the product is 15.  (1 + 2^-12) x (1 + 2^-13): hi = 1 and lo = 2^-12 / 2^-13 exactly, so
    hi hi = 1 and the cross terms 2^-12 + 2^-13 are exact and the kernel's result is 1 + 2^-12 + 2^-13 -- the float32 rounding
    of the product.  At the last row / column of an even-sized input the ky = 0 / kx = 0 tap of output row Ho has no pixel."""
    cin, cout = shape
    H, W = hw
    Ho, Wo = ref.out_size(H, W)
    B, c, n = 2, 5, cout - 3
    pairs = [(3.0, 5.0), (1.0 + 2.0 ** -12, 1.0 + 2.0 ** -13)]
    assert np.float32(pairs[1][0] * pairs[1][1]) == np.float32(1.0 + 2.0 ** -12 + 2.0 ** -13)
    places = [(0, 0, 0), (1, Ho - 1, Wo - 1), (0, 0, 1), (1, 1, 1)]  # corners, an edge, interior (output pixels)
    hits = 0
    for k, (b, oy, ox) in enumerate(places if shape == NARROW else places[1:3]):
        for ky, kx in ref.TAPS:
            iy, ix = 2 * oy + ky - 1, 2 * ox + kx - 1
            inside = 0 <= iy < H and 0 <= ix < W
            vx, vd = pairs[(k + ky + kx) % 2]
            x, dy = np.zeros((B, H, W, cin), np.float32), np.zeros((B, Ho, Wo, cout), np.float32)
            # a tap that leaves the image: the nearest pixel inside instead, which another tap (or none) joins to the output pixel
            x[b, min(max(iy, 0), H - 1), min(max(ix, 0), W - 1), c] = vx
            dy[b, oy, ox, n] = vd
            want = np.zeros((cout, cin, 3, 3), np.float32)
            jy, jx = min(max(iy, 0), H - 1) - 2 * oy + 1, min(max(ix, 0), W - 1) - 2 * ox + 1
            if 0 <= jy < 3 and 0 <= jx < 3:
                want[n, c, jy, jx] = np.float32(vx * vd)
            hits += inside
            np.testing.assert_array_equal(want, ref.dw_ref(x, dy).astype(np.float32))
            np.testing.assert_array_equal(wgrad(x, dy), want, err_msg=str((b, oy, ox, ky, kx, vx, vd)))
    assert hits > 0
    # no tap joins them: another sample, or an input row that output row 1 does not read (2 oy + ky - 1 >= 1)
    x, dy = np.zeros((B, H, W, cin), np.float32), np.zeros((B, Ho, Wo, cout), np.float32)
    x[0, 1, 1, c], dy[1, 1, 1, n] = 3.0, 5.0
    assert (wgrad(x, dy) == 0.0).all()
    x[:] = 0.0
    x[1, 0, 1, c] = 3.0
    assert (wgrad(x, dy) == 0.0).all() and (ref.dw_ref(x, dy) == 0.0).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_dw_power_of_two_scaling_of_either_operand_is_exact(shape):
    sl = bdn.slice_pixels(*shape)
    Ho, Wo = grid_of(sl + sl // 2 + 1)  # two slices
    x, dy = ref.inputs("plain", 1, 2 * Ho, 2 * Wo - 1, *shape, seed=3)
    base = wgrad(x, dy)
    for p in (18, -20):
        f = np.float32(2.0 ** p)
        assert np.array_equal(wgrad(x * f, dy), base * f), p
        assert np.array_equal(wgrad(x, dy * f), base * f), p
    assert np.array_equal(wgrad(x * np.float32(2.0 ** 40), dy * np.float32(2.0 ** -37)), base * np.float32(8.0))


@pytest.mark.parametrize("shape", SHAPES)
def test_non_finite_dy_reaches_exactly_what_it_should(shape):
    """A NaN in one dY pixel and an inf in another: dW is non-finite at exactly the (o, :, ky, kx) whose tap lies inside the image
    for that pixel, dX at exactly the input pixels those output pixels' taps touch (all channels) -- and finite everywhere else
    (the powers of two of a slice / a pixel pass a non-finite maximum through unscaled; the values here keep fp16's range)."""
    cin, cout = shape
    B, H, W = 2, 24, 30  # 360 output pixels: two slices of the narrow shape
    Ho, Wo = ref.out_size(H, W)
    x, dy = ref.inputs("plain", B, H, W, *shape, seed=8)
    w = ref.weights(*shape, seed=9)
    dy[0, 0, 0, 9] = np.nan  # a corner: the ky = 0 and kx = 0 taps leave the image
    dy[1, Ho - 1, 7, 3] = -np.inf  # the last row of an even-sized input: every tap inside
    got_dw, got_dx = wgrad(x, dy), dgrad(dy, w, H, W)
    with np.errstate(invalid="ignore", over="ignore"):
        want_dw, want_dx = ref.dw_ref(x, dy), ref.dx_phases(dy, w, H, W)[0]
    bad = ~np.isfinite(want_dw)
    assert bad.sum() == (4 + 9) * cin and bad[9, :, 1:, 1:].all() and bad[3].all()
    assert not np.isfinite(got_dw[bad]).any() and np.isfinite(got_dw[~bad]).all()
    badx = ~np.isfinite(want_dx)
    assert badx.sum() == (4 + 9) * cin and badx[0, :2, :2].all() and badx[1, H - 3:H, 13:16].all()
    assert not np.isfinite(got_dx[badx]).any() and np.isfinite(got_dx[~badx]).all()


# ---- the input gradient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("i", range(len(EDGE_SIZES)))
def test_dx_error_bound_at_the_tile_edges(i, shape):
    B, H, W = EDGE_SIZES[i]
    kind = KINDS[i % 3]
    _, dy = ref.inputs(kind, B, H, W, *shape, seed=11 * i + shape[1])
    check_dx(dy, ref.weights(*shape, seed=i), H, W, shape, "%s %s" % ((B, H, W), kind))


def planted_weights(cin, cout):
    """w[o, c, ky, kx] = +-(1 + q / 64)(1 + 2^-13) with q and the sign functions of (o, c, ky, kx), as tests/test_bev_up2_gpu.py
    plants them: a value read from another channel or tap is another number, every weight has hi = +-(1 + q / 64) and a non-zero
    lo that the split carries exactly."""
    o_, c_, ky_, kx_ = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(3), np.arange(3), indexing="ij")
    q = (7 * c_ + 3 * o_ + 13 * (3 * ky_ + kx_)) % 64
    exact = np.where((c_ + o_ + ky_ + kx_) % 2, -1.0, 1.0) * (1.0 + q / 64.0) * (1.0 + 2.0 ** -13)
    w = exact.astype(np.float32)
    assert np.array_equal(w.astype(np.float64), exact)
    return w


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("hw", IMPULSE_SIZES)
def test_dx_impulse_reads_the_single_right_weights(shape, hw):
    """A unit impulse of dy at (b, oy, ox, n) gives dx[b, 2 oy + ky - 1, 2 ox + kx - 1, :] = w[n, :, ky, kx] within 1 ulp at the
    up to nine input pixels inside the image and exact zeros everywhere else."""
    cin, cout = shape
    H, W = hw
    Ho, Wo = ref.out_size(H, W)
    B, n = 2, cout - 5
    w = planted_weights(cin, cout)
    assert len({float(w[n, 3, ky, kx]) for ky, kx in ref.TAPS}) == 9
    seen = set()
    # corners, edges, interior; (1, 0, 1): the first row of sample 1 must not reach the last row of sample 0, whose ky = 0 tap
    # is absent when H is even
    for b, oy, ox in [(0, 0, 0), (1, Ho - 1, Wo - 1), (0, 1, 0), (1, Ho - 1, 1), (1, 1, 1), (1, 0, 1)]:
        dy = np.zeros((B, Ho, Wo, cout), np.float32)
        dy[b, oy, ox, n] = 1.0
        got = dgrad(dy, w, H, W)
        touched = 0
        for ky, kx in ref.TAPS:
            iy, ix = 2 * oy + ky - 1, 2 * ox + kx - 1
            if not (0 <= iy < H and 0 <= ix < W):
                continue
            col = w[n, :, ky, kx]
            assert (np.abs(got[b, iy, ix] - col) <= np.spacing(np.abs(col))).all(), (b, oy, ox, ky, kx)
            got[b, iy, ix] = 0.0
            touched += 1
        seen.add(touched)
        assert (got == 0.0).all(), (b, oy, ox)
    assert 9 in seen and 4 in seen
    if H % 2 == 0 and W % 2 == 0:
        assert seen == {4, 6, 9}  # (the last output row / column of an even size keeps all three taps: 2 Ho - 1 = H - 1)


@pytest.mark.parametrize("shape", SHAPES)
def test_dx_power_of_two_scaling_is_exact(shape):
    B, H, W = 2, 7, 10
    _, dy = ref.inputs("plain", B, H, W, *shape, seed=4)
    w = ref.weights(*shape, seed=5)
    base = dgrad(dy, w, H, W)
    for p in (18, -20):
        f = np.float32(2.0 ** p)
        assert np.array_equal(dgrad(dy * f, w, H, W), base * f), p
        assert np.array_equal(dgrad(dy, w * f, H, W), base * f), p


# ---- both entry points -----------------------------------------------------------------------------------------------------
def guarded(values, guard=4096):
    n = values.size
    big = torch.full((n + 2 * guard,), float("nan"), device=DEV)
    big[guard:guard + n] = torch.from_numpy(values).to(DEV).reshape(-1)
    return big, big[guard:guard + n]


def guards_intact(big, n, guard=4096):
    return bool(torch.isnan(big[:guard]).all()) and bool(torch.isnan(big[guard + n:]).all())


def ff_filled(n, guard=4096):
    """n floats of 0xFF bytes inside a NaN-filled allocation."""
    big = torch.full((n + 2 * guard,), float("nan"), device=DEV)
    big[guard:guard + n].view(torch.uint8).fill_(0xFF)
    return big, big[guard:guard + n]


@pytest.mark.parametrize("shape,hw", [(PRODUCT, (17, 19)), (NARROW, (6, 51)), (PRODUCT, (3, 4)), (NARROW, (34, 33)), (NARROW, (1, 1))])
def test_reads_stay_inside_the_inputs_and_every_output_element_is_written(shape, hw):
    """Inputs are slices of NaN-filled allocations (a read outside them poisons the result); outputs and workspaces are filled
    with 0xFF bytes and sit in NaN-filled allocations: outputs fully written, the guards untouched, the bits those of a tight run
    and of a run on a zeroed workspace."""
    cin, cout = shape
    B, (H, W) = 2, hw
    xs, dys = ref.inputs("plain", B, H, W, *shape, seed=6)
    w = ref.weights(*shape, seed=7)
    xbig, x = guarded(xs)
    dbig, dyv = guarded(dys)
    wtbig, wt = guarded(w)
    # dW
    nws = bdn.wgrad_workspace_bytes(B, H, W, *shape)
    assert nws % 4 == 0
    wbig, dw = ff_filled(w.size)
    wsbig, ws = ff_filled(nws // 4)
    _lib.call("mssvt_bev_down_wgrad", x.data_ptr(), dyv.data_ptr(), B, H, W, cin, cout, dw.data_ptr(), ws.data_ptr(), _lib.stream())
    got = dw.view(cout, cin, 3, 3).cpu().numpy()
    assert np.isfinite(got).all()
    for big, n in ((wbig, w.size), (wsbig, nws // 4), (xbig, xs.size), (dbig, dys.size)):
        assert guards_intact(big, n)
    np.testing.assert_array_equal(got, wgrad(xs, dys))
    np.testing.assert_array_equal(got, wgrad(xs, dys, torch.zeros(nws, dtype=torch.uint8, device=DEV)))
    # dX
    nds = bdn.dgrad_workspace_bytes(B, H, W, *shape)
    assert nds % 4 == 0
    xgbig, dx = ff_filled(xs.size)
    dsbig, ds = ff_filled(nds // 4)
    _lib.call("mssvt_bev_down_dgrad", dyv.data_ptr(), wt.data_ptr(), B, H, W, cin, cout, dx.data_ptr(), ds.data_ptr(), _lib.stream())
    gotx = dx.view(B, H, W, cin).cpu().numpy()
    assert np.isfinite(gotx).all()
    for big, n in ((xgbig, xs.size), (dsbig, nds // 4), (dbig, dys.size), (wtbig, w.size)):
        assert guards_intact(big, n)
    np.testing.assert_array_equal(gotx, dgrad(dys, w, H, W))
    np.testing.assert_array_equal(gotx, dgrad(dys, w, H, W, torch.zeros(nds, dtype=torch.uint8, device=DEV)))


@pytest.mark.parametrize("shape", SHAPES)
def test_bit_identical_across_calls_and_streams(shape):
    sl = bdn.slice_pixels(*shape)
    H, W = 50, 2 * ((sl + 100) // 25) - 1  # 2 x 25 x (sl + 100) / 25 output pixels: three slices
    xs, dys = ref.inputs("plain", 2, H, W, *shape, seed=12)
    assert ref.num_slices(dys.shape[0] * dys.shape[1] * dys.shape[2], sl) == 3
    x, dy, w = nchw(xs), nchw(dys), torch.from_numpy(ref.weights(*shape, seed=1)).to(DEV)
    first = (bdn.down_wgrad(x, dy), bdn.down_dgrad(dy, w, H, W))
    again = (bdn.down_wgrad(x, dy), bdn.down_dgrad(dy, w, H, W))
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            outs.append((bdn.down_wgrad(x, dy), bdn.down_dgrad(dy, w, H, W)))
        st.synchronize()
    for o in [again] + outs:
        assert torch.equal(first[0], o[0]) and torch.equal(first[1], o[1])


def test_the_backward_never_synchronises_the_host():
    shape = NARROW
    H, W = 18, 41
    xs, dys = ref.inputs("plain", 2, H, W, *shape, seed=15)
    x, dy, w = nchw(xs), nchw(dys), torch.from_numpy(ref.weights(*shape, seed=2)).to(DEV)
    warm = (bdn.down_wgrad(x, dy), bdn.down_dgrad(dy, w, H, W))
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
            out = (bdn.down_wgrad(x, dy), bdn.down_dgrad(dy, w, H, W))
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    assert torch.equal(warm[0], out[0]) and torch.equal(warm[1], out[1])


def test_every_status_code_is_reached_and_nothing_is_launched():
    lib = _lib.lib()
    for bad in [(256, 128), (64, 32), (128, 128), (256, 256), (32, 32), (48, 48), (0, 64), (32, 0), (512, 512), (128, 64)]:
        assert lib.mssvt_bev_down_train_supported(*bad) == 0, bad
        assert lib.mssvt_bev_down_wgrad_slice_pixels(*bad) == 0, bad
    for f in (lib.mssvt_bev_down_wgrad_workspace_bytes, lib.mssvt_bev_down_dgrad_workspace_bytes):
        assert f(1, 4, 4, 48, 48) == 0 and f(0, 4, 4, 32, 64) == 0 and f(1, 4, -4, 32, 64) == 0 and f(1, 0, 4, 32, 64) == 0
        assert f(1 << 15, 1 << 8, 1 << 8, 32, 64) == 0  # 2^31 input pixels
        assert f(1 << 13, 1 << 8, 1 << 8, 32, 64) > 0
    x = torch.ones(1, 4, 4, 32, device=DEV)
    dy = torch.ones(1, 2, 2, 64, device=DEV)
    w = torch.ones(64, 32, 3, 3, device=DEV)
    dw = torch.full((64, 32, 3, 3), 7.0, device=DEV)
    dx = torch.full((1, 4, 4, 32), 7.0, device=DEV)
    ws = torch.full((max(bdn.wgrad_workspace_bytes(1, 4, 4, 32, 64), bdn.dgrad_workspace_bytes(1, 4, 4, 32, 64)) // 4,), 7.0, device=DEV)
    st = _lib.stream()
    BAD, BIG = -1, -2
    for f, a, b, out in ((lib.mssvt_bev_down_wgrad, x.data_ptr(), dy.data_ptr(), dw.data_ptr()),
                         (lib.mssvt_bev_down_dgrad, dy.data_ptr(), w.data_ptr(), dx.data_ptr())):
        sp = ws.data_ptr()
        assert f(None, b, 1, 4, 4, 32, 64, out, sp, st) == BAD
        assert f(a, None, 1, 4, 4, 32, 64, out, sp, st) == BAD
        assert f(a, b, 1, 4, 4, 32, 64, None, sp, st) == BAD
        assert f(a, b, 1, 4, 4, 32, 64, out, None, st) == BAD
        assert f(a, b, 0, 4, 4, 32, 64, out, sp, st) == BAD
        assert f(a, b, 1, 0, 4, 32, 64, out, sp, st) == BAD
        assert f(a, b, 1, 4, -4, 32, 64, out, sp, st) == BAD
        assert f(a, b, 1, 4, 4, 0, 64, out, sp, st) == BAD
        assert f(a, b, 1, 4, 4, 32, -64, out, sp, st) == BAD
        for k in range(4):  # each pointer unaligned in turn
            ptrs = [a, b, out, sp]
            ptrs[k] += 4
            assert f(ptrs[0], ptrs[1], 1, 4, 4, 32, 64, ptrs[2], ptrs[3], st) == BAD, k
        assert f(a, b, 1, 4, 4, 48, 48, out, sp, st) == BIG
        assert f(a, b, 1, 4, 4, 64, 32, out, sp, st) == BIG
        assert f(a, b, 1, 4, 4, 32, 32, out, sp, st) == BIG
        assert f(a, b, 1 << 15, 1 << 8, 1 << 8, 32, 64, out, sp, st) == BIG  # 2^31 input pixels
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((dx == 7.0).all()) and bool((ws == 7.0).all())
    # and the good call is MSSVT_OK (0) for both
    assert lib.mssvt_bev_down_wgrad(x.data_ptr(), dy.data_ptr(), 1, 4, 4, 32, 64, dw.data_ptr(), ws.data_ptr(), st) == 0
    assert lib.mssvt_bev_down_dgrad(dy.data_ptr(), w.data_ptr(), 1, 4, 4, 32, 64, dx.data_ptr(), ws.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool((dw == 4.0).sum() > 0) and not bool((dx == 7.0).any())
    # the Python layer: no CPU path, channels-last fp32 only, workspaces checked
    xc = torch.zeros(1, 32, 4, 4, device=DEV)
    good = xc.contiguous(memory_format=torch.channels_last)
    gy = torch.zeros(1, 64, 2, 2, device=DEV).contiguous(memory_format=torch.channels_last)
    for wrong in (xc, good.cpu(), good.double(), xc[0]):
        with pytest.raises(MssvtHipError):
            bdn.down_wgrad(wrong, gy)
    with pytest.raises(MssvtHipError):
        bdn.down_wgrad(good, torch.zeros(1, 64, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last))  # dy is not (Ho, Wo)
    with pytest.raises(MssvtHipError):
        bdn.down_wgrad(good, gy, torch.zeros(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(MssvtHipError):
        bdn.down_dgrad(gy, w.cpu(), 4, 4)
    with pytest.raises(MssvtHipError):
        bdn.down_dgrad(gy, torch.zeros(64, 32, 1, 1, device=DEV), 4, 4)
    with pytest.raises(MssvtHipError):
        bdn.down_dgrad(gy, w, 5, 4)  # (5, 4) has a (3, 2) output
    with pytest.raises(MssvtHipError):
        bdn.down_dgrad(gy, w, 4, 4, torch.zeros(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(MssvtHipError):
        bdn.wgrad_workspace_bytes(1, 4, 4, 48, 48)
    with pytest.raises(MssvtHipError):
        bdn.dgrad_workspace_bytes(1, 4, 4, 64, 32)


# ---- the Function and the predicates -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("hw", [(9, 11), (10, 12)])
@pytest.mark.parametrize("input_grad,weight_grad,nchw_grad", [(True, True, False), (False, True, False), (True, False, False),
                                                              (True, True, True)])
def test_function_matches_the_statement(shape, hw, input_grad, weight_grad, nchw_grad):
    cin, cout = shape
    B, (H, W) = 2, hw
    Ho, Wo = ref.out_size(H, W)
    xs, dys = ref.inputs("plain", B, H, W, *shape, seed=cin + H)
    ws = ref.weights(*shape, seed=cout)
    x = nchw(xs).requires_grad_(input_grad)
    w = torch.from_numpy(ws).to(DEV).requires_grad_(weight_grad)
    y = bdn.DownFunction.apply(x, w)
    assert bev_conv.is_channels_last(y) and tuple(y.shape) == (B, cout, Ho, Wo)
    # the forward IS the inference kernel with the stride-2 pack
    with torch.no_grad():
        same = bev_conv.conv_bn_act(nchw(xs), bev_conv.pack_weight(w.detach(), 3, cin, cout, 2, 1), relu=False)
    assert torch.equal(y.detach(), same)
    want_y, _, bound_y = ref.y_ref(xs, ws)
    err = np.abs(y.detach().permute(0, 2, 3, 1).cpu().numpy() - want_y)
    print("y %s %s: worst error / bound %.3f" % (shape, hw, float((err / np.maximum(bound_y, 1e-300)).max())))
    assert (err <= bound_y).all()
    g = nchw(dys)
    if nchw_grad:
        g = g.contiguous()
        assert not bev_conv.is_channels_last(g)
    y.backward(g)
    if weight_grad:
        dw = w.grad.cpu().numpy()
        assert (np.abs(dw - ref.dw_ref(xs, dys)) <= ref.dw_bound(xs, dys, bdn.slice_pixels(*shape))).all()
        np.testing.assert_array_equal(dw, wgrad(xs, dys))
    else:
        assert w.grad is None
    if input_grad:
        want_dx, _, bound_dx = ref.dx_phases(dys, ws, H, W)
        assert bev_conv.is_channels_last(x.grad) and tuple(x.grad.shape) == (B, cin, H, W)
        got_dx = x.grad.permute(0, 2, 3, 1).cpu().numpy()
        assert (np.abs(got_dx - want_dx) <= bound_dx).all()
        np.testing.assert_array_equal(got_dx, dgrad(dys, ws, H, W))
    else:
        assert x.grad is None


def test_function_skips_the_gradient_kernels_nobody_needs(monkeypatch):
    shape = NARROW
    xs, dys = ref.inputs("plain", 1, 6, 7, *shape, seed=1)
    calls = []
    real_d, real_w = bdn.down_dgrad, bdn.down_wgrad
    monkeypatch.setattr(bdn, "down_dgrad", lambda *a, **k: (calls.append("dx"), real_d(*a, **k))[1])
    monkeypatch.setattr(bdn, "down_wgrad", lambda *a, **k: (calls.append("dw"), real_w(*a, **k))[1])
    for gx, gw, want in ((True, True, ["dx", "dw"]), (False, True, ["dw"]), (True, False, ["dx"])):
        del calls[:]
        x = nchw(xs).requires_grad_(gx)
        w = torch.from_numpy(ref.weights(*shape, seed=2)).to(DEV).requires_grad_(gw)
        bdn.DownFunction.apply(x, w).backward(nchw(dys))
        assert calls == want, (gx, gw)


def test_function_makes_an_nchw_input_channels_last_and_refuses_an_uncovered_shape():
    shape = NARROW
    H, W = 4, 5
    xs, dys = ref.inputs("plain", 1, H, W, *shape, seed=1)
    w = torch.from_numpy(ref.weights(*shape, seed=2)).to(DEV).requires_grad_(True)
    x = nchw(xs).contiguous().requires_grad_(True)
    assert not bev_conv.is_channels_last(x)
    y = bdn.DownFunction.apply(x, w)
    y.backward(nchw(dys))
    want_dx, _, bound_dx = ref.dx_phases(dys, w.detach().cpu().numpy(), H, W)
    assert (np.abs(x.grad.permute(0, 2, 3, 1).cpu().numpy() - want_dx) <= bound_dx).all()
    with pytest.raises(MssvtHipError):
        bdn.DownFunction.apply(x, torch.zeros(48, 32, 3, 3, device=DEV))
    with pytest.raises(MssvtHipError):
        bdn.DownFunction.apply(x, torch.zeros(64, 32, 1, 1, device=DEV))
    with pytest.raises(MssvtHipError):
        bdn.DownFunction.apply(nchw(np.zeros((1, 4, 5, 64), np.float32)), torch.zeros(32, 64, 3, 3, device=DEV))  # (64, 32)


def test_routing_predicates(monkeypatch):
    for cin, cout in SHAPES:
        for ok, pad in ((nn.Conv2d(cin, cout, 3, stride=2, padding=1, bias=False).to(DEV), None),
                        (nn.Conv2d(cin, cout, 3, stride=2, padding=0, bias=False).to(DEV), 1)):
            assert bdn.down_shape(ok, pad) == (cin, cout) and bdn.down_train_supported(ok, pad)
            assert bdn.down_train_routed(ok, pad) == ((cin, cout) in bdn.ROUTED_DOWN_TRAIN or (cin, cout) == NARROW)
    for no in (nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=True), nn.Conv2d(32, 64, 3, stride=1, padding=1, bias=False),
               nn.Conv2d(32, 64, 3, stride=2, padding=0, bias=False), nn.Conv2d(32, 64, 3, stride=2, padding=2, dilation=2, bias=False),
               nn.Conv2d(64, 32, 3, stride=2, padding=1, bias=False), nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False),
               nn.Conv2d(256, 256, 3, stride=2, padding=1, bias=False), nn.Conv2d(32, 64, 3, stride=2, padding=1, groups=2, bias=False),
               nn.ConvTranspose2d(32, 64, 3, stride=2, padding=1, bias=False)):
        assert not bdn.down_train_supported(no.to(DEV)) and not bdn.down_train_routed(no.to(DEV)), no
    assert not bdn.down_train_supported(nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False))  # parameters on the CPU
    assert not bdn.down_train_supported(nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False).to(DEV).double())
    wide = nn.Conv2d(128, 256, 3, stride=2, padding=1, bias=False).to(DEV)
    monkeypatch.setattr(bdn, "ROUTED_DOWN_TRAIN", frozenset())
    assert bdn.down_train_supported(wide) and not bdn.down_train_routed(wide)
    monkeypatch.setattr(bdn, "ROUTED_DOWN_TRAIN", frozenset({PRODUCT}))
    assert bdn.down_train_routed(wide)
