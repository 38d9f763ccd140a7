"""mssvt_bev_conv_wgrad (csrc/bev_conv.hip, kernels in csrc/split_wgrad.hip.h) and ``bev_conv_train.Conv3x3Function`` against
the float64 statement and the bound of tests/bev_conv_train_ref.py (its docstring derives the bound)."""
import numpy as np
import pytest
import torch

from mssvt_amd import _lib, bev_conv, bev_conv_train as bct
from mssvt_amd._lib import MssvtHipError
from tests import bev_conv_ref, bev_conv_train_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = bct.CHANNEL_SHAPES
FIXED_SIZES = [(1, 1, 1), (1, 2, 3), (3, 5, 7), (1, 1, 31), (1, 1, 32), (1, 1, 33), (2, 15, 17)]


def grid_of(n):
    """(1, H, W) with H W = n and H as large as it gets up to sqrt(n) (a prime n: one row)."""
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return (1, h, n // h)


def slice_sizes(c):
    """Grids with pixel counts one below, at and one above one, two and three slices."""
    sl = bct.slice_pixels(c, c)
    return [grid_of(k * sl + e) for k in (1, 2, 3) for e in (-1, 0, 1)]


def wgrad(x, dy, d, workspace=None):
    """x (B, H, W, cin), dy (B, H, W, cout) host arrays -> dw (cout, cin, 3, 3) numpy through the C entry point."""
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(DEV).permute(0, 3, 1, 2)
    dyt = torch.from_numpy(np.ascontiguousarray(dy)).to(DEV).permute(0, 3, 1, 2)
    return bct.conv_wgrad(xt, dyt, d, workspace).cpu().numpy()


def check(x, dy, d, c, tag):
    got = wgrad(x, dy, d)
    want = ref.dw_ref(x, dy, d)
    bound = ref.dw_bound(x, dy, d, bct.slice_pixels(c, c))
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst error / bound %.3f" % (tag, ratio))
    assert got.shape == want.shape and (err <= bound).all(), (tag, ratio)
    return ratio


def test_the_slice_rule_is_published():
    assert [bct.slice_pixels(c, c) for c, _ in SHAPES] == [4096, 2048, 256, 256]
    assert bct.slice_pixels(128, 256) == 0
    sl = bct.slice_pixels(128, 128)
    base = 2 * ((4 * 3 * sl + 255) // 256 * 256)
    assert bct.workspace_bytes(1, 3, sl, 128, 128) == base + 3 * 9 * 128 * 128 * 4
    assert bct.workspace_bytes(1, 1, 3 * sl + 1, 128, 128) == 2 * ((4 * (3 * sl + 1) + 255) // 256 * 256) + 4 * 9 * 128 * 128 * 4


@pytest.mark.parametrize("c", [c for c, _ in SHAPES])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("i", range(len(FIXED_SIZES)))
def test_error_bound_at_the_small_sizes(i, d, c):
    B, H, W = FIXED_SIZES[i]
    kind = ("plain", "tail", "spike")[i % 3]
    x, dy = ref.inputs(kind, B, H, W, c, c, seed=100 * i + c + d)
    check(x, dy, d, c, "%d ch d%d %s %s" % (c, d, (B, H, W), kind))


@pytest.mark.parametrize("c", [c for c, _ in SHAPES])
@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("i", range(9))
def test_error_bound_either_side_of_one_two_and_three_slices(i, d, c):
    B, H, W = slice_sizes(c)[i]
    kind = ("tail", "spike", "plain")[i % 3]
    x, dy = ref.inputs(kind, B, H, W, c, c, seed=7 * i + c + d)
    check(x, dy, d, c, "%d ch d%d %s %s" % (c, d, (B, H, W), kind))


@pytest.mark.parametrize("c", [32, 128])
def test_a_slice_may_span_two_samples(c):
    sl = bct.slice_pixels(c, c)
    H, W = 9, sl // 12  # 3 samples of ~0.75 slices: slice 0 ends inside sample 1, slice 1 inside sample 2
    x, dy = ref.inputs("plain", 3, H, W, c, c, seed=5)
    assert ref.num_slices(3 * H * W, sl) == 3 and H * W < sl
    check(x, dy, 2, c, "%d ch spanning" % c)


@pytest.mark.parametrize("c", [32, 128])
@pytest.mark.parametrize("d", [1, 2])
def test_impulse_against_impulse_lands_on_the_single_right_element(c, d):
    """x holds 1 + 2^-12 (hi = 1, lo = 2^-12) at one pixel and channel, dy 1 + 2^-13 at the pixel one tap away: dw is the
    float32 product within 1 ulp at that (o, c, ky, kx) and exactly zero everywhere else -- the taps that fall outside the image
    at a corner or an edge included.  A dropped cross term is 2^-12 or 2^-13 off: 2048 / 1024 ulp."""
    H, W, ci, co = 5, 7, 5 % c, (c - 3)
    hits = 0
    for (py, px) in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 3), (2, 0), (H - 1, 4), (2, 3)]:
        for ky, kx in ref.TAPS:
            qy, qx = py - (ky - 1) * d, px - (kx - 1) * d  # the output pixel whose tap (ky, kx) reads (py, px)
            x, dy = np.zeros((1, H, W, c), np.float32), np.zeros((1, H, W, c), np.float32)
            x[0, py, px, ci] = 1.0 + 2.0 ** -12
            inside = 0 <= qy < H and 0 <= qx < W
            # outside: the gradient impulse sits on the input pixel itself, whose only matching tap is the centre
            dy[0, qy if inside else py, qx if inside else px, co] = 1.0 + 2.0 ** -13
            got = wgrad(x, dy, d)
            want = np.zeros((c, c, 3, 3))
            want[co, ci, ky if inside else 1, kx if inside else 1] = (1.0 + 2.0 ** -12) * (1.0 + 2.0 ** -13)
            np.testing.assert_array_equal(want, ref.dw_ref(x, dy, d))
            assert (got[want == 0.0] == 0.0).all(), (py, px, ky, kx)
            assert (np.abs(got - want)[want != 0.0] <= 2.0 ** -23).all(), (py, px, ky, kx)
            hits += inside
    assert hits > 40


@pytest.mark.parametrize("c,d", [(128, 2), (64, 1), (256, 1)])
def test_power_of_two_scaling_of_either_operand_is_exact(c, d):
    sl = bct.slice_pixels(c, c)
    B, H, W = grid_of(sl + sl // 2)  # two slices
    x, dy = ref.inputs("plain", B, H, W, c, c, seed=3)
    base = wgrad(x, dy, d)
    for p in (18, -20):
        s = np.float32(2.0 ** p)
        assert np.array_equal(wgrad(x * s, dy, d), base * s), p
        assert np.array_equal(wgrad(x, dy * s, d), base * s), p
    assert np.array_equal(wgrad(x * np.float32(2.0 ** 40), dy * np.float32(2.0 ** -37), d), base * np.float32(8.0))


def test_non_finite_inputs_never_come_out_finite():
    c, d = 32, 1
    x, dy = ref.inputs("plain", 2, 12, 30, c, c, seed=8)  # 720 pixels: three slices
    x[0, 2, 3, 5] = np.nan
    x[1, 4, 8, 31] = np.inf
    dy[1, 11, 29, 7] = -np.inf
    dy[0, 0, 0, 9] = np.nan
    got = wgrad(x, dy, d)
    with np.errstate(invalid="ignore", over="ignore"):
        want = ref.dw_ref(x, dy, d)
    bad = ~np.isfinite(want)
    assert bad.sum() > 0 and not np.isfinite(got[bad]).any()
    clean = np.isfinite(want)
    assert clean.sum() > 0 and np.isfinite(got[clean]).all()  # (channels no bad value reaches stay finite at this range)


@pytest.mark.parametrize("c,d,hw", [(128, 2, (17, 19)), (32, 1, (6, 50)), (256, 1, (3, 5))])
def test_reads_stay_inside_the_inputs_and_every_element_of_dw_is_written(c, d, hw):
    """x and dy are slices of NaN-filled allocations (a read outside them poisons the result); dw and the NaN-prefilled
    workspace sit in NaN-filled allocations: dw fully written, the guards untouched, the bits those of a tight run."""
    B, (H, W) = 2, hw
    xs, dys = ref.inputs("plain", B, H, W, c, c, seed=6)
    guard = 4096

    def guarded(values):
        n = values.size
        big = torch.full((n + 2 * guard,), float("nan"), device=DEV)
        big[guard:guard + n] = torch.from_numpy(values).to(DEV).reshape(-1)
        return big, big[guard:guard + n]

    xbig, x = guarded(xs)
    dbig, dyv = guarded(dys)
    ndw = c * c * 9
    wbig = torch.full((ndw + 2 * guard,), float("nan"), device=DEV)
    nws = bct.workspace_bytes(B, H, W, c, c)
    assert nws % 4 == 0
    wsbig = torch.full((nws // 4 + 2 * guard,), float("nan"), device=DEV)
    ws = wsbig[guard:guard + nws // 4]
    _lib.call("mssvt_bev_conv_wgrad", x.data_ptr(), dyv.data_ptr(), B, H, W, c, c, 3, d, wbig[guard:guard + ndw].data_ptr(),
              ws.data_ptr(), _lib.stream())
    got = wbig[guard:guard + ndw].view(c, c, 3, 3).cpu().numpy()
    assert np.isfinite(got).all()
    for big, n in ((wbig, ndw), (wsbig, nws // 4), (xbig, xs.size), (dbig, dys.size)):
        assert bool(torch.isnan(big[:guard]).all()) and bool(torch.isnan(big[guard + n:]).all())
    np.testing.assert_array_equal(got, wgrad(xs, dys, d))
    zeroed = torch.zeros(nws, dtype=torch.uint8, device=DEV)
    np.testing.assert_array_equal(got, wgrad(xs, dys, d, zeroed))  # whatever the workspace held


def test_bit_identical_across_calls_and_streams():
    c, d = 128, 1
    sl = bct.slice_pixels(c, c)
    xs, dys = ref.inputs("plain", 2, 50, (sl + 100) // 50, c, c, seed=12)  # three slices
    x = torch.from_numpy(xs).to(DEV).permute(0, 3, 1, 2)
    dy = torch.from_numpy(dys).to(DEV).permute(0, 3, 1, 2)
    first = bct.conv_wgrad(x, dy, d)
    again = bct.conv_wgrad(x, dy, d)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(bct.conv_wgrad(x, dy, d))
        s.synchronize()
    for o in [again] + outs:
        assert torch.equal(first, o)


def test_weight_gradient_never_synchronises_the_host():
    c = 64
    xs, dys = ref.inputs("plain", 2, 9, 40, c, c, seed=15)
    x = torch.from_numpy(xs).to(DEV).permute(0, 3, 1, 2)
    dy = torch.from_numpy(dys).to(DEV).permute(0, 3, 1, 2)
    warm = bct.conv_wgrad(x, dy, 2)
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
            out = bct.conv_wgrad(x, dy, 2)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    assert torch.equal(warm, out)


def test_every_status_code_is_reached_and_nothing_is_launched():
    lib = _lib.lib()
    for c, _ in SHAPES:
        assert lib.mssvt_bev_conv_wgrad_supported(3, c, c, 1, 1) == 1 and lib.mssvt_bev_conv_wgrad_supported(3, c, c, 1, 2) == 1
    for bad in [(3, 128, 256, 1, 1), (3, 48, 48, 1, 1), (3, 128, 128, 2, 1), (3, 128, 128, 1, 3), (1, 128, 128, 1, 1), (3, 32, 64, 1, 1)]:
        assert lib.mssvt_bev_conv_wgrad_supported(*bad) == 0, bad
    assert lib.mssvt_bev_conv_wgrad_workspace_bytes(1, 4, 4, 3, 48, 48) == 0
    assert lib.mssvt_bev_conv_wgrad_workspace_bytes(0, 4, 4, 3, 32, 32) == 0
    assert lib.mssvt_bev_conv_wgrad_workspace_bytes(1 << 15, 1 << 8, 1 << 8, 3, 32, 32) == 0
    x = torch.ones(1, 4, 4, 32, device=DEV)
    dy = torch.ones(1, 4, 4, 32, device=DEV)
    dw = torch.full((32, 32, 3, 3), 7.0, device=DEV)
    ws = torch.full((bct.workspace_bytes(1, 4, 4, 32, 32) // 4,), 7.0, device=DEV)
    st = _lib.stream()
    xp, dp, wp, sp = x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr()
    BAD, BIG = -1, -2
    f = lib.mssvt_bev_conv_wgrad
    assert f(None, dp, 1, 4, 4, 32, 32, 3, 1, wp, sp, st) == BAD
    assert f(xp, None, 1, 4, 4, 32, 32, 3, 1, wp, sp, st) == BAD
    assert f(xp, dp, 1, 4, 4, 32, 32, 3, 1, None, sp, st) == BAD
    assert f(xp, dp, 1, 4, 4, 32, 32, 3, 1, wp, None, st) == BAD
    assert f(xp, dp, 0, 4, 4, 32, 32, 3, 1, wp, sp, st) == BAD
    assert f(xp, dp, 1, 4, -4, 32, 32, 3, 1, wp, sp, st) == BAD
    assert f(xp, dp, 1, 4, 4, 32, 32, 3, 0, wp, sp, st) == BAD
    for k in range(4):  # each pointer unaligned in turn
        ptrs = [xp, dp, wp, sp]
        ptrs[k] += 4
        assert f(ptrs[0], ptrs[1], 1, 4, 4, 32, 32, 3, 1, ptrs[2], ptrs[3], st) == BAD, k
    assert f(xp, dp, 1, 4, 4, 48, 48, 3, 1, wp, sp, st) == BIG
    assert f(xp, dp, 1, 4, 4, 32, 64, 3, 1, wp, sp, st) == BIG
    assert f(xp, dp, 1, 4, 4, 32, 32, 1, 1, wp, sp, st) == BIG
    assert f(xp, dp, 1, 4, 4, 32, 32, 3, 3, wp, sp, st) == BIG
    assert f(xp, dp, 1 << 15, 1 << 8, 1 << 8, 32, 32, 3, 1, wp, sp, st) == BIG  # 2^31 pixels
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((ws == 7.0).all())
    # the Python layer: no CPU path, channels-last fp32 only
    xc = torch.zeros(1, 32, 4, 4, device=DEV)
    good = xc.contiguous(memory_format=torch.channels_last)
    for wrong in (xc, good.cpu(), good.double(), xc[0]):
        with pytest.raises(MssvtHipError):
            bct.conv_wgrad(wrong, good, 1)
    with pytest.raises(MssvtHipError):
        bct.conv_wgrad(good, torch.zeros(1, 32, 4, 5, device=DEV).contiguous(memory_format=torch.channels_last), 1)
    with pytest.raises(MssvtHipError):
        bct.conv_wgrad(good, good, 1, torch.zeros(16, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("c,d", [(32, 1), (64, 2), (128, 2), (256, 1)])
@pytest.mark.parametrize("input_grad,nchw_grad", [(True, False), (False, False), (True, True)])
def test_function_matches_the_statement(c, d, input_grad, nchw_grad):
    """y, dX (through the forward kernel on the rotated weights: the forward's bound on (dY, rotated w)) and dW (the bound of
    the weight gradient), with and without an input gradient and with an NCHW-contiguous incoming gradient."""
    B, H, W = 2, 9, 11
    xs, dys = ref.inputs("plain", B, H, W, c, c, seed=c + d)
    ws = (np.random.default_rng(c).standard_normal((c, c, 3, 3)) * 0.05).astype(np.float32)
    x = torch.from_numpy(xs).to(DEV).permute(0, 3, 1, 2).requires_grad_(input_grad)
    w = torch.from_numpy(ws).to(DEV).requires_grad_(True)
    y = bct.Conv3x3Function.apply(x, w, d)
    assert bev_conv.is_channels_last(y) and tuple(y.shape) == (B, c, H, W)
    want_y, a_y = bev_conv_ref.conv(xs, ws, 1, d)
    assert (np.abs(y.detach().permute(0, 2, 3, 1).cpu().numpy() - want_y) <= bev_conv_ref.error_bound(a_y, xs, ws, 3, c)).all()
    g = torch.from_numpy(dys).to(DEV).permute(0, 3, 1, 2)
    if nchw_grad:
        g = g.contiguous()
        assert not bev_conv.is_channels_last(g)
    y.backward(g)
    dw = w.grad.cpu().numpy()
    assert (np.abs(dw - ref.dw_ref(xs, dys, d)) <= ref.dw_bound(xs, dys, d, bct.slice_pixels(c, c))).all()
    np.testing.assert_array_equal(dw, wgrad(xs, dys, d))
    if not input_grad:
        assert x.grad is None
        return
    rot = np.ascontiguousarray(ws[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))
    want_dx, a_dx = bev_conv_ref.conv(dys, rot, 1, d)
    np.testing.assert_allclose(want_dx, ref.dx_ref(dys, ws, d), rtol=0, atol=1e-12 * np.abs(want_dx).max())
    dx = x.grad.permute(0, 2, 3, 1).cpu().numpy()
    assert (np.abs(dx - want_dx) <= bev_conv_ref.error_bound(a_dx, dys, rot, 3, c)).all()


def test_routing_predicates():
    from torch import nn
    ok = nn.Conv2d(32, 32, 3, padding=2, dilation=2, bias=False).to(DEV)
    assert bct.train_supported(ok) and bct.train_routed(ok)
    padded = nn.Conv2d(64, 64, 3, padding=0, bias=False).to(DEV)
    assert bct.train_supported(padded, 1) and not bct.train_supported(padded)
    for no in (nn.Conv2d(32, 32, 3, padding=1, bias=True), nn.Conv2d(32, 64, 3, padding=1, bias=False),
               nn.Conv2d(32, 32, 3, stride=2, padding=1, bias=False), nn.Conv2d(32, 32, 1, bias=False),
               nn.Conv2d(32, 32, 3, padding=2, bias=False), nn.ConvTranspose2d(32, 32, 1, bias=False)):
        assert not bct.train_supported(no.to(DEV)), no
    assert not bct.train_supported(nn.Conv2d(32, 32, 3, padding=1, bias=False))  # parameters on the CPU
    wide = nn.Conv2d(128, 128, 3, padding=1, bias=False).to(DEV)
    assert bct.train_supported(wide) and bct.train_routed(wide) == ((3, 128, 128, 1, 1) in bct.ROUTED_TRAIN)
