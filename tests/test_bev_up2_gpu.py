"""mssvt_bev_up2 (the 2 x 2 stride-2 transposed deblock on the split-fp16 kernel) and the into-forms (``out=, channel=``) of
csrc/bev_conv.hip against the float64 statement of tests/bev_up2_ref.py.

The error bound, per output element, with a = sum_c |x| |w[c, n, dy, dx]| and S = Cin / 32 + 2:

    |got - ref| <= (3 2^-22 + S 2^-24) a + 2^-24 max|x| sum_c |w[c, n, dy, dx]|

-- the derivation of tests/test_bev_conv_gpu.py at ONE tap: every output element of a kernel-2 stride-2 transposed convolution
is reached by exactly one input pixel through exactly one weight plane."""
import numpy as np
import pytest
import torch
from torch import nn

from mssvt_amd import _lib, bev_conv
from mssvt_amd._lib import MssvtHipError
from tests import bev_conv_ref
from tests import bev_up2_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(64, 32), (256, 256)]
# (B, H, W) input sizes: the smallest grids and odd sizes; either side of the wave tile (32 input pixels) and of the workgroup
# tile (256); sample boundaries inside a tile
SIZES = [(1, 1, 1), (1, 2, 3), (3, 5, 7), (1, 1, 31), (1, 1, 32), (1, 1, 33), (1, 15, 17), (1, 16, 16), (1, 1, 257), (3, 9, 10)]
SENTINEL = 0x7FC12345  # a NaN no computation produces


def make_up2(cin, cout, seed, bias=False, bn=False, wscale=1.0):
    g = torch.Generator().manual_seed(seed)
    conv = nn.ConvTranspose2d(cin, cout, 2, stride=2, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * wscale)
        if bias:
            conv.bias.copy_(torch.randn(cout, generator=g))
    norm = None
    if bn:
        norm = nn.BatchNorm2d(cout, eps=1e-3)
        with torch.no_grad():
            norm.weight.copy_(torch.rand(cout, generator=g) + 0.5)
            norm.bias.copy_(torch.randn(cout, generator=g) * 0.3)
            norm.running_mean.copy_(torch.randn(cout, generator=g) * 0.5)
            norm.running_var.copy_(torch.rand(cout, generator=g) * 1.7 + 0.3)
        norm = norm.to(DEV).eval()
    return conv.to(DEV).eval(), norm


def make_conv(k, cin, cout, stride, seed, transposed=False):
    g = torch.Generator().manual_seed(seed)
    conv = nn.ConvTranspose2d(cin, cout, 1, stride=1, bias=False) if transposed else \
        nn.Conv2d(cin, cout, k, stride=stride, padding=1 if k == 3 else 0, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
    return conv.to(DEV).eval()


def activations(shape, seed):
    """Non-negative, half of them zero (what a ReLU leaves)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g).clamp_(min=0.0) * 3.0).contiguous()


def run(x_nhwc, conv, norm, relu):
    """x (B, H, W, C) host tensor -> y (B, 2H, 2W, Cout) numpy through pack_up2 + up2_bn_act."""
    x = x_nhwc.to(DEV).permute(0, 3, 1, 2)
    y = bev_conv.up2_bn_act(x, bev_conv.pack_up2(conv, norm), relu)
    assert bev_conv.is_channels_last(y) and y.dtype == torch.float32
    return y.permute(0, 2, 3, 1).cpu().numpy()


def statement(x_nhwc, conv, norm, relu):
    w = conv.weight.detach().cpu().numpy()
    bn = None
    if norm is not None:
        bn = dict(mean=norm.running_mean.cpu().numpy(), var=norm.running_var.cpu().numpy(), eps=norm.eps,
                  weight=norm.weight.detach().cpu().numpy(), bias=norm.bias.detach().cpu().numpy())
    scale, shift = ref.fold(conv.out_channels, None if conv.bias is None else conv.bias.detach().cpu().numpy(), bn)
    y, a = ref.up2(x_nhwc.numpy(), w, scale, shift, relu)
    return y, a, scale, shift


def library(x_nhwc, conv, relu):
    with torch.no_grad():
        y = conv(x_nhwc.to(DEV).permute(0, 3, 1, 2))
        y = torch.relu(y) if relu else y
    return y.permute(0, 2, 3, 1).cpu().numpy()


def guarded(n, fill, dtype=torch.float32, guard=4096):
    """(whole allocation, the n-element slice in its middle): what lies around the slice must come back untouched."""
    big = torch.full((n + 2 * guard,), fill, dtype=dtype, device=DEV)
    return big, big[guard:guard + n]


def untouched(big, n, fill, guard=4096):
    head, tail = big[:guard], big[guard + n:]
    if isinstance(fill, float) and fill != fill:
        return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())
    return bool((head == fill).all()) and bool((tail == fill).all())


def sentinel_rows(B, ho, wo, C):
    """A NaN-guarded (B, ho, wo, C) output whose every element holds SENTINEL's bits."""
    big, flat = guarded(B * ho * wo * C, float("nan"))
    flat.view(torch.int32).fill_(SENTINEL)
    return big, flat.view(B, ho, wo, C)


def check_slice(big, rows, channel, cout):
    """Inside [channel, channel + cout) every element written and finite, outside it every bit as before, the guards NaN."""
    B, ho, wo, C = rows.shape
    bits = rows.view(torch.int32)
    assert bool((bits[..., :channel] == SENTINEL).all()) and bool((bits[..., channel + cout:] == SENTINEL).all())
    inside = rows[..., channel:channel + cout]
    assert bool(torch.isfinite(inside).all())
    assert untouched(big, rows.numel(), float("nan"))
    return inside


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_error_bound_at_every_size(cin, cout):
    """Non-negative activations, signed weights, scale 1 / shift 0: the bound of the module docstring, at every size."""
    conv, _ = make_up2(cin, cout, seed=cin + cout)
    w = conv.weight.detach().cpu().numpy()
    worst, worst_lib = 0.0, 0.0
    for i, (B, H, W) in enumerate(SIZES):
        relu = bool(i % 2)
        x = activations((B, H, W, cin), seed=i + cin)
        got = run(x, conv, None, relu)
        want, a, _, _ = statement(x, conv, None, relu)
        assert got.shape == want.shape == (B, 2 * H, 2 * W, cout)
        bound = ref.error_bound(a, x.numpy(), w)
        ratio = np.abs(got - want) / np.maximum(bound, 1e-300)
        worst = max(worst, float(ratio.max()))
        if i == len(SIZES) - 1:  # the library's fp32 path under the same measure, for the record (not the limit)
            worst_lib = float((np.abs(library(x, conv, relu) - want) / np.maximum(bound, 1e-300)).max())
        print("up2 %d->%d %s: worst error / bound %.3f" % (cin, cout, (B, H, W), float(ratio.max())))
        assert (np.abs(got - want) <= bound).all(), ((B, H, W), float(ratio.max()))
    print("up2 %d->%d: worst error / bound: kernel %.3f (all sizes), library fp32 %.3f (last size)" % (cin, cout, worst, worst_lib))


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_impulse_lands_in_its_four_output_pixels_on_the_right_phase(cin, cout):
    """One input pixel, one channel = 1 + 2^-12 (hi = 1, lo = 2^-12) per sample, at the corners, on the edges and inside a 5 x 7
    grid; w[c, n, dy, dx] = +-(1 + q / 64)(1 + 2^-13) with q and the sign functions of (c, n, dy, dx), so a value read from another
    input channel, output channel or phase is another number, and each weight has hi = +-(1 + q / 64) and a non-zero lo: a dropped
    hi lo or lo hi term is 2^-12 or 2^-13 off (2048 / 1024 ulp).  Every reached output is the product within 1 ulp (the dropped
    lo lo term is < 2^-24 of it, the join of the two sums rounds once), every other one exactly 0."""
    H, W = 5, 7
    spots = [(0, 0), (0, 6), (4, 0), (4, 6), (0, 3), (2, 0), (4, 3), (2, 6), (2, 3)]
    conv, _ = make_up2(cin, cout, seed=1)
    c, n, dy, dx = np.meshgrid(np.arange(cin), np.arange(cout), np.arange(2), np.arange(2), indexing="ij")
    ph = dy * 2 + dx
    q = (c * 7 + n * 13 + ph * 29) % 64
    wv = np.where((c + n + ph) % 2 == 0, 1.0, -1.0) * (1.0 + q / 64.0) * (1.0 + 2.0 ** -13)
    assert (wv.astype(np.float32) == wv).all()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(wv.astype(np.float32)))
    x = torch.zeros(len(spots), H, W, cin)
    for b, (iy, ix) in enumerate(spots):
        x[b, iy, ix, (7 * b + 3) % cin] = 1.0 + 2.0 ** -12
    got = run(x, conv, None, False)
    want, _, _, _ = statement(x, conv, None, False)
    hit = np.zeros(want.shape, bool)
    for b, (iy, ix) in enumerate(spots):
        hit[b, 2 * iy:2 * iy + 2, 2 * ix:2 * ix + 2] = True
    assert ((want != 0.0) == hit).all()
    assert (got[~hit] == 0.0).all()
    ulp = 2.0 ** (np.floor(np.log2(np.abs(want[hit]))) - 23)
    assert (np.abs(got - want)[hit] <= ulp).all(), float((np.abs(got - want)[hit] / ulp).max())


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_batch_norm_fold_with_bias(cin, cout):
    """Scale and shift are the float64 fold rounded once to fp32 (2^-24 each): |scale| * bound + 2^-23 (|scale| a + |shift|);
    the blob read back on the host holds the folded values once per phase and the weights at column ph Cout + n."""
    conv, norm = make_up2(cin, cout, seed=5 + cin, bias=True, bn=True, wscale=0.05)
    x = activations((2, 9, 11, cin), seed=17)
    w = conv.weight.detach().cpu().numpy()
    for relu in (False, True):
        got = run(x, conv, norm, relu)
        want, a, scale, shift = statement(x, conv, norm, relu)
        bound = np.abs(scale) * ref.error_bound(a, x.numpy(), w) + 2.0 ** -23 * (np.abs(scale) * a + np.abs(shift))
        assert (np.abs(got - want) <= bound).all()
    packed = bev_conv.pack_up2(conv, norm)
    assert packed.blob.numel() == _lib.lib().mssvt_bev_up2_pack_bytes(cin, cout) == 64 + 32 * cout + 16 * cin * cout
    # the blob is the BEV blob of the 1 x 1 layer (4 cout, cin, 1, 1) with row ph cout + n = w[:, n, dy, dx]
    as_1x1 = np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(4 * cout, cin, 1, 1))
    s4, t4 = np.tile(scale.astype(np.float32), 4), np.tile(shift.astype(np.float32), 4)
    blob = packed.blob.cpu().numpy()
    np.testing.assert_array_equal(blob[64:64 + 16 * cout].view(np.float32), s4)
    np.testing.assert_array_equal(blob[64 + 16 * cout:64 + 32 * cout].view(np.float32), t4)
    if cout >= 128:  # (the host writer slices the columns 128 wide, as the kernel does from cout = 128 on)
        np.testing.assert_array_equal(blob, bev_conv_ref.host_pack(as_1x1, s4, t4))


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_power_of_two_scaling_is_exact_and_mixed_ranges_stay_inside_the_bound(cin, cout):
    conv, _ = make_up2(cin, cout, seed=9)
    x = activations((2, 11, 13, cin), seed=4) + 2.0 ** -6  # (no zeros: every element really scales)
    base = run(x, conv, None, False)
    for p in (18, -20):
        assert np.array_equal(run(x * 2.0 ** p, conv, None, False), base * np.float32(2.0 ** p)), p
    mixed = x.clone()
    mixed[:, :, :6] *= 2.0 ** 10
    mixed[:, :, 6:] *= 2.0 ** -10
    got = run(mixed, conv, None, True)
    want, a, _, _ = statement(mixed, conv, None, True)
    assert (np.abs(got - want) <= ref.error_bound(a, mixed.numpy(), conv.weight.detach().cpu().numpy())).all()
    # one input pixel is the whole receptive field: the small region keeps its own relative accuracy everywhere
    small = want[:, :, 12:]
    assert (np.abs(got[:, :, 12:] - small) <= 2.0 ** -18 * np.abs(small).max()).all()


@pytest.mark.parametrize("relu", [False, True])
def test_non_finite_inputs_never_come_out_finite(relu):
    conv, norm = make_up2(64, 32, seed=2, bn=True)
    x = activations((2, 6, 9, 64), seed=8)
    x[0, 2, 3, 5] = float("nan")
    x[1, 4, 8, 63] = float("inf")
    x[1, 0, 0, 0] = float("-inf")
    got = run(x, conv, norm, relu)
    want, _, _, _ = statement(x, conv, norm, relu)
    bad = ~np.isfinite(want)
    assert bad.sum() > 0 and not np.isfinite(got[bad]).any()
    clean = np.isfinite(want).all(axis=3)
    assert np.isfinite(got[clean]).all()  # and the other pixels are untouched by them


@pytest.mark.parametrize("cin,cout,hw", [(64, 32, (6, 7)), (256, 256, (17, 19))])
def test_up2_reads_stay_inside_and_only_its_channel_slice_is_written(cin, cout, hw):
    """Input, exponent workspace and output sit in NaN / -1 guarded allocations, the output is pre-filled with a sentinel: the
    slice [channel, channel + cout) is fully written, every other channel and everything around keeps its bits."""
    conv, _ = make_up2(cin, cout, seed=3)
    packed = bev_conv.pack_up2(conv, None)
    B, (H, W) = 2, hw
    xs = activations((B, H, W, cin), seed=6)
    xbig, xflat = guarded(xs.numel(), float("nan"))
    xflat.copy_(xs.to(DEV).reshape(-1))
    ebig, e = guarded(B * H * W, -1, torch.int32)
    channel, C = 8, cout + 20
    ybig, rows = sentinel_rows(B, 2 * H, 2 * W, C)
    _lib.call("mssvt_bev_up2", xflat.data_ptr(), B, H, W, cin, packed.blob.data_ptr(), cout, 0, e.data_ptr(), rows.data_ptr(), C,
              channel, _lib.stream())
    inside = check_slice(ybig, rows, channel, cout)
    assert untouched(ebig, B * H * W, -1) and bool((e >= 0).all())
    np.testing.assert_array_equal(inside.cpu().numpy(), run(xs, conv, None, False))  # the bits of a tight allocation


@pytest.mark.parametrize("k,cin,cout,stride,transposed,hw", [(1, 128, 256, 1, True, (17, 19)), (3, 32, 64, 2, False, (9, 7)),
                                                             (3, 128, 256, 2, False, (5, 6))])
def test_into_form_writes_only_its_channel_slice_and_equals_the_allocating_form(k, cin, cout, stride, transposed, hw):
    conv = make_conv(k, cin, cout, stride, seed=4, transposed=transposed)
    packed = bev_conv.pack(conv, None)
    B, (H, W) = 2, hw
    xs = activations((B, H, W, cin), seed=7)
    xbig, xflat = guarded(xs.numel(), float("nan"))
    xflat.copy_(xs.to(DEV).reshape(-1))
    x = xflat.view(B, H, W, cin).permute(0, 3, 1, 2)
    ho, wo = packed.out_size(H, W)
    channel, C = 12, cout + 16
    ebig, e = guarded(B * H * W, -1, torch.int32)
    ybig, rows = sentinel_rows(B, ho, wo, C)
    _lib.call("mssvt_bev_conv_into", xflat.data_ptr(), B, H, W, cin, packed.blob.data_ptr(), k, cout, stride, 1, 1, e.data_ptr(),
              rows.data_ptr(), C, channel, _lib.stream())
    inside = check_slice(ybig, rows, channel, cout)
    assert untouched(ebig, B * H * W, -1)
    want = bev_conv.conv_bn_act(x, packed, True)
    assert torch.equal(inside.permute(0, 3, 1, 2), want)
    # and through the Python layer: the returned view is the slice
    ybig2, rows2 = sentinel_rows(B, ho, wo, C)
    view = bev_conv.conv_bn_act(x, packed, True, out=rows2.permute(0, 3, 1, 2), channel=channel)
    assert view.data_ptr() == rows2.data_ptr() + 4 * channel and tuple(view.shape) == (B, cout, ho, wo)
    assert torch.equal(view, want) and torch.equal(check_slice(ybig2, rows2, channel, cout).permute(0, 3, 1, 2), want)


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_bit_identical_across_forms_calls_and_streams(cin, cout):
    conv, norm = make_up2(cin, cout, seed=12, bn=True)
    x = activations((3, 21, 23, cin), seed=13).to(DEV).permute(0, 3, 1, 2)
    packed = bev_conv.pack_up2(conv, norm)
    first = bev_conv.up2_bn_act(x, packed, True)
    exact = torch.empty(3, 42, 46, cout, device=DEV).permute(0, 3, 1, 2)
    view = bev_conv.up2_bn_act(x, packed, True, out=exact, channel=0)
    assert view.data_ptr() == exact.data_ptr() and torch.equal(exact, first)
    wide = torch.zeros(3, 42, 46, cout + 8, device=DEV).permute(0, 3, 1, 2)
    assert torch.equal(bev_conv.up2_bn_act(x, packed, True, out=wide, channel=4), first)
    assert float(wide[:, :4].abs().max()) == 0.0 and float(wide[:, 4 + cout:].abs().max()) == 0.0
    torch.cuda.synchronize()
    outs = [bev_conv.up2_bn_act(x, packed, True)]
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(bev_conv.up2_bn_act(x, packed, True))
        s.synchronize()
    for o in outs:
        assert torch.equal(first, o)


def test_pack_and_up2_never_synchronise_the_host():
    conv, norm = make_up2(64, 32, seed=14, bn=True)
    one = make_conv(1, 32, 32, 1, seed=15, transposed=True)
    x = activations((2, 9, 9, 64), seed=15).to(DEV).permute(0, 3, 1, 2)
    x1 = activations((2, 18, 18, 32), seed=16).to(DEV).permute(0, 3, 1, 2)

    def both():
        out = torch.empty(2, 18, 18, 64, device=DEV).permute(0, 3, 1, 2)
        bev_conv.conv_bn_act(x1, bev_conv.pack(one, None), True, out=out, channel=0)
        bev_conv.up2_bn_act(x, bev_conv.pack_up2(conv, norm), True, out=out, channel=32)
        return out

    warm = both()
    torch.cuda.synchronize()
    with torch.no_grad():
        conv.weight.mul_(1.0)  # a new version: the pack below really runs
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
            out = both()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    assert torch.equal(warm, out)


def test_every_status_code_is_reached_and_nothing_is_launched():
    lib = _lib.lib()
    assert lib.mssvt_bev_up2_supported(256, 256) == 1 and lib.mssvt_bev_up2_supported(64, 32) == 1
    for bad in [(128, 256), (256, 128), (64, 64), (32, 32), (0, 0), (48, 32)]:
        assert lib.mssvt_bev_up2_supported(*bad) == 0 and lib.mssvt_bev_up2_pack_bytes(*bad) == 0, bad
    assert lib.mssvt_bev_up2_pack_bytes(256, 256) == 64 + 8 * 1024 + 4 * 256 * 1024
    conv, _ = make_up2(64, 32, seed=1)
    packed = bev_conv.pack_up2(conv, None)
    before = packed.blob.clone()
    x = torch.zeros(1, 4, 4, 64, device=DEV)
    y = torch.full((1, 8, 8, 40), 7.0, device=DEV)
    e = torch.full((16,), -1, dtype=torch.int32, device=DEV)
    st = _lib.stream()
    xp, yp, ep, bp, wp = x.data_ptr(), y.data_ptr(), e.data_ptr(), packed.blob.data_ptr(), conv.weight.data_ptr()
    BAD, BIG = -1, -2
    up2 = lib.mssvt_bev_up2
    assert up2(None, 1, 4, 4, 64, bp, 32, 0, ep, yp, 40, 8, st) == BAD
    assert up2(xp, 1, 4, 4, 64, None, 32, 0, ep, yp, 40, 8, st) == BAD
    assert up2(xp, 1, 4, 4, 64, bp, 32, 0, None, yp, 40, 8, st) == BAD
    assert up2(xp, 1, 4, 4, 64, bp, 32, 0, ep, None, 40, 8, st) == BAD
    assert up2(xp + 4, 1, 4, 4, 64, bp, 32, 0, ep, yp, 40, 8, st) == BAD  # unaligned
    assert up2(xp, 1, 4, 4, 64, bp, 32, 0, ep, yp + 8, 40, 8, st) == BAD
    assert up2(xp, 0, 4, 4, 64, bp, 32, 0, ep, yp, 40, 8, st) == BAD
    assert up2(xp, 1, 4, -4, 64, bp, 32, 0, ep, yp, 40, 8, st) == BAD
    assert up2(xp, 1, 4, 4, 64, bp, 32, 0, ep, yp, 42, 8, st) == BAD  # ystride % 4
    assert up2(xp, 1, 4, 4, 64, bp, 32, 0, ep, yp, 40, 6, st) == BAD  # ybase % 4
    assert up2(xp, 1, 4, 4, 64, bp, 32, 0, ep, yp, 40, -4, st) == BAD
    assert up2(xp, 1, 4, 4, 64, bp, 32, 0, ep, yp, 40, 12, st) == BAD  # ybase + cout > ystride
    assert up2(xp, 1, 4, 4, 64, bp, 64, 0, ep, yp, 64, 0, st) == BIG  # uncovered shape
    assert up2(xp, 1, 4, 4, 128, bp, 32, 0, ep, yp, 40, 8, st) == BIG
    assert up2(xp, 1 << 13, 1 << 8, 1 << 8, 64, bp, 32, 0, ep, yp, 40, 8, st) == BIG  # 2^29 input = 2^31 OUTPUT pixels
    into = lib.mssvt_bev_conv_into
    c1 = make_conv(1, 32, 32, 1, seed=2, transposed=True)
    p1 = bev_conv.pack(c1, None)
    x1 = torch.zeros(1, 8, 8, 32, device=DEV)
    e1 = torch.full((64,), -1, dtype=torch.int32, device=DEV)
    b1 = p1.blob.data_ptr()
    assert into(None, 1, 8, 8, 32, b1, 1, 32, 1, 1, 0, e1.data_ptr(), yp, 40, 8, st) == BAD
    assert into(x1.data_ptr(), 1, 8, 8, 32, b1, 1, 32, 1, 1, 0, e1.data_ptr(), yp + 4, 40, 8, st) == BAD
    assert into(x1.data_ptr(), 1, 8, 8, 32, b1, 1, 32, 1, 1, 0, e1.data_ptr(), yp, 38, 4, st) == BAD
    assert into(x1.data_ptr(), 1, 8, 8, 32, b1, 1, 32, 1, 1, 0, e1.data_ptr(), yp, 40, 2, st) == BAD
    assert into(x1.data_ptr(), 1, 8, 8, 32, b1, 1, 32, 1, 1, 0, e1.data_ptr(), yp, 40, 12, st) == BAD
    assert into(x1.data_ptr(), 1, 8, 8, 32, b1, 1, 32, 1, 1, 0, e1.data_ptr(), yp, 0, 0, st) == BAD
    assert into(x1.data_ptr(), 1, 8, 8, 32, b1, 1, 32, 2, 1, 0, e1.data_ptr(), yp, 40, 8, st) == BIG
    assert into(x1.data_ptr(), 1 << 15, 1 << 8, 1 << 8, 32, b1, 1, 32, 1, 1, 0, e1.data_ptr(), yp, 40, 8, st) == BIG
    pk = lib.mssvt_bev_up2_pack
    assert pk(None, None, None, None, None, None, 0.0, 64, 32, bp, st) == BAD
    assert pk(wp, None, None, None, None, None, 0.0, 64, 32, None, st) == BAD
    assert pk(wp, None, None, None, None, None, 0.0, 64, 32, bp + 4, st) == BAD
    assert pk(wp, None, wp, None, None, None, 0.0, 64, 32, bp, st) == BAD  # affine without statistics
    assert pk(wp, None, None, None, wp, None, 0.0, 64, 32, bp, st) == BAD  # mean without variance
    assert pk(wp, None, None, None, None, None, 0.0, 0, 32, bp, st) == BAD
    assert pk(wp, None, None, None, None, None, 0.0, 64, 64, bp, st) == BIG
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((e == -1).all()) and bool((e1 == -1).all()) and torch.equal(packed.blob, before)
    # the Python layer: no CPU path, channels-last fp32 only, `out` dense, aligned and wide enough
    xl = x.permute(0, 3, 1, 2)
    good = torch.zeros(1, 8, 8, 40, device=DEV).permute(0, 3, 1, 2)
    assert tuple(bev_conv.up2_bn_act(xl, packed, True, out=good, channel=8).shape) == (1, 32, 8, 8)
    wrong_out = [(torch.zeros(1, 40, 8, 8, device=DEV), 8), (good, 6), (good, 12), (good, -4), (good.double(), 8), (good.cpu(), 8),
                 (torch.zeros(1, 8, 8, 48, device=DEV).permute(0, 3, 1, 2)[:, :40], 8),  # pixel stride != C
                 (torch.zeros(1, 8, 9, 40, device=DEV).permute(0, 3, 1, 2), 8), (torch.zeros(2, 8, 8, 40, device=DEV).permute(0, 3, 1, 2), 8),
                 (torch.zeros(8 * 8 * 40 + 1, device=DEV)[1:].view(1, 8, 8, 40).permute(0, 3, 1, 2), 8),  # 4 bytes off
                 (good[0], 8)]
    for out, ch in wrong_out:
        with pytest.raises(MssvtHipError):
            bev_conv.up2_bn_act(xl, packed, True, out=out, channel=ch)
    with pytest.raises(MssvtHipError):
        bev_conv.up2_bn_act(xl, packed, True, channel=4)  # channel without out
    with pytest.raises(MssvtHipError):
        bev_conv.conv_bn_act(x1.permute(0, 3, 1, 2), p1, True, out=good, channel=12)
    for wrong in (x, xl.cpu(), xl.double(), torch.zeros(1, 4, 4, 32, device=DEV).permute(0, 3, 1, 2), xl[0]):
        with pytest.raises(MssvtHipError):
            bev_conv.up2_bn_act(wrong, packed, True)
    with pytest.raises(MssvtHipError):
        bev_conv.up2_bn_act(xl, p1, True)  # a blob of the other family
    with pytest.raises(MssvtHipError):
        bev_conv.up2_bn_act(xl.clone(memory_format=torch.preserve_format).requires_grad_(True), packed, True)
    with pytest.raises(MssvtHipError):
        bev_conv.pack_up2(nn.ConvTranspose2d(64, 64, 2, stride=2).to(DEV))
    assert not bev_conv.up2_supported(nn.ConvTranspose2d(64, 32, 2, stride=2))  # parameters on the CPU
    assert bev_conv.up2_supported(conv, None) and not bev_conv.up2_supported(conv, nn.BatchNorm2d(64).to(DEV))
    assert float(good[:, :8].abs().max()) == 0.0 and float(good[:, 40:].abs().sum()) == 0.0


def test_pack_up2_is_cached_and_rebuilt_after_load_state_dict():
    conv, norm = make_up2(64, 32, seed=21, bn=True)
    p0 = bev_conv.pack_up2(conv, norm)
    assert bev_conv.pack_up2(conv, norm) is p0
    with torch.no_grad():
        norm.running_var.add_(0.25)
    p1 = bev_conv.pack_up2(conv, norm)
    assert p1 is not p0 and not torch.equal(p1.blob, p0.blob)
    sd = {k: v.clone() for k, v in conv.state_dict().items()}
    sd["weight"] *= -0.5
    conv.load_state_dict(sd)
    p2 = bev_conv.pack_up2(conv, norm)
    assert p2 is not p1 and not torch.equal(p2.blob, p1.blob) and bev_conv.pack_up2(conv, norm) is p2
    x = activations((1, 3, 4, 64), seed=1)
    want, a, scale, shift = statement(x, conv, norm, True)
    w = conv.weight.detach().cpu().numpy()
    bound = np.abs(scale) * ref.error_bound(a, x.numpy(), w) + 2.0 ** -23 * (np.abs(scale) * a + np.abs(shift))
    assert (np.abs(run(x, conv, norm, True) - want) <= bound).all()
    assert bev_conv.pack_up2(conv, None) is not p2  # another fold of the same layer
