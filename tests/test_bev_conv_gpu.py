"""csrc/bev_conv.hip (split-fp16 BEV convolution, its weight pack) and mssvt_dense_bev_nhwc against the float64 statement of
tests/bev_conv_ref.py.

The error bound, per output element, with A = (|x| conv |w|) and S = taps * Cin / 32 + 2:

    |got - ref| <= (3 2^-22 + S 2^-24) A + 2^-24 max|x| sum|w|

Derivation.  An operand v (normalised by an exact power of two into (-2, 2)) is carried as hi = fp16(v) and
lo = fp16((v - hi) 2^11), both rounded to nearest: hi is off by at most 2^-11 |v|, the residual has at most 12 bits and a
sign, one more than lo holds, so hi + lo / 2^11 is off by at most 2^-23 |v|.  A product x w is computed as
hi hi + (hi lo + lo hi) / 2^11: the dropped lo lo term is at most 2^-11 2^-11 = 2^-22 of |x w|, the two operand errors add
2 * 2^-23: together 2 * 2^-22 <= 3 * 2^-22 of A.  The sums are fp32 accumulators of the matrix instruction: one rounding
(2^-24 of the partial sum, itself at most A) per k step of 32 input channels and per tap -- taps * Cin / 32 steps in the
hi hi chain (the cross-term chain is 2^-11 of that and disappears in the slack) -- plus the join of the two chains and the
scale / shift fma of the epilogue: S steps.  Operands far below their normalisation (another region of the image, a small
weight) land in fp16's denormal range, where hi and lo are off by 2^-25 absolute: 2^-36 of the largest operand after the
lo half, covered -- with room -- by the last term, 2^-24 max|x| sum|w|.
"""
import numpy as np
import pytest
import torch
from torch import nn

from mssvt_amd import _lib, bev_conv
from mssvt_amd._lib import MssvtHipError
from tests import bev_conv_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

TAPS = [(3, 1, 1), (3, 2, 1), (3, 1, 2), (3, 2, 2), (1, 1, 1)]  # (ksize, stride, dilation)
WP, BP = bev_conv.WAVE_PIXELS, bev_conv.BLOCK_PIXELS
# (B, H, W): the smallest grids, grids below the dilated footprint, odd and even sizes, and output pixel counts one below,
# at and one above the wave tile (32) and the workgroup tile (256) at stride 1
SIZES = [(1, 1, 1), (1, 2, 3), (3, 5, 7), (1, 2, 2), (3, 4, 6), (1, 1, WP - 1), (1, 1, WP), (1, 1, WP + 1), (1, 15, 17),
         (1, 16, BP // 16), (1, 1, BP + 1), (3, 9, 10)]


def make_layer(k, cin, cout, stride, dilation, seed, bias=False, bn=False, transposed=False, wscale=1.0):
    g = torch.Generator().manual_seed(seed)
    if transposed:
        conv = nn.ConvTranspose2d(cin, cout, 1, stride=1, bias=bias)
    else:
        conv = nn.Conv2d(cin, cout, k, stride=stride, padding=dilation if k == 3 else 0, dilation=dilation, bias=bias)
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


def activations(shape, seed):
    """Non-negative, half of them zero (what a ReLU leaves)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g).clamp_(min=0.0) * 3.0).contiguous()


def run(x_nhwc, conv, norm, relu):
    """x (B, H, W, C) host tensor -> y (B, Ho, Wo, Cout) numpy through pack + conv_bn_act."""
    x = x_nhwc.to(DEV).permute(0, 3, 1, 2)
    y = bev_conv.conv_bn_act(x, bev_conv.pack(conv, norm), relu)
    assert bev_conv.is_channels_last(y) and y.dtype == torch.float32
    return y.permute(0, 2, 3, 1).cpu().numpy()


def statement(x_nhwc, conv, norm, relu, stride, dilation):
    w = conv.weight.detach().cpu().numpy()
    bn = None
    if norm is not None:
        bn = dict(mean=norm.running_mean.cpu().numpy(), var=norm.running_var.cpu().numpy(), eps=norm.eps,
                  weight=norm.weight.detach().cpu().numpy(), bias=norm.bias.detach().cpu().numpy())
    scale, shift = ref.fold(conv.out_channels, None if conv.bias is None else conv.bias.detach().cpu().numpy(), bn)
    tr = isinstance(conv, nn.ConvTranspose2d)
    y, a = ref.conv(x_nhwc.numpy(), w, stride, dilation, scale=scale, shift=shift, relu=relu, transposed=tr)
    return y, a, scale, shift


def library(x_nhwc, conv, relu):
    with torch.no_grad():
        y = conv(x_nhwc.to(DEV).permute(0, 3, 1, 2))
        y = torch.relu(y) if relu else y
    return y.permute(0, 2, 3, 1).cpu().numpy()


@pytest.mark.parametrize("cin,cout", bev_conv.CHANNEL_SHAPES)
@pytest.mark.parametrize("k,stride,dilation", TAPS)
def test_error_bound_on_every_tap_set_channel_shape_and_size(k, stride, dilation, cin, cout):
    """Non-negative activations, signed weights, scale 1 / shift 0: the bound of the module docstring, at every size."""
    conv, _ = make_layer(k, cin, cout, stride, dilation, seed=k + stride + dilation + cin)
    w = conv.weight.detach().cpu().numpy()
    worst, worst_lib = 0.0, 0.0
    for i, (B, H, W) in enumerate(SIZES):
        relu = bool(i % 2)
        x = activations((B, H, W, cin), seed=i + cin)
        got = run(x, conv, None, relu)
        want, a, _, _ = statement(x, conv, None, relu, stride, dilation)
        assert got.shape == want.shape == (B, (H - 1) // stride + 1, (W - 1) // stride + 1, cout)
        bound = ref.error_bound(a, x.numpy(), w, k, cin)
        err = np.abs(got - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        if i == len(SIZES) - 1:  # the library's fp32 convolution under the same measure, for the record (not the limit)
            worst_lib = float((np.abs(library(x, conv, relu) - want) / np.maximum(bound, 1e-300)).max())
        assert (err <= bound).all(), ((B, H, W), float((err / np.maximum(bound, 1e-300)).max()))
    print("k%d s%d d%d %d->%d: worst error / bound: kernel %.3f (all sizes), library fp32 %.3f (last size)" % (k, stride, dilation, cin, cout, worst, worst_lib))


@pytest.mark.parametrize("cin,cout,transposed", [(32, 64, False), (128, 256, True), (256, 256, False)])
def test_batch_norm_fold_bias_and_transposed_layout(cin, cout, transposed):
    """The fold adds two roundings of its own: scale and shift are the float64 fold rounded once to fp32 (2^-24 each), so the
    bound becomes |scale| * bound + 2^-23 (|scale| A + |shift|); the blob read back on the host holds the folded values."""
    k, stride, dilation = (1, 1, 1) if transposed else (3, 2, 1)
    conv, norm = make_layer(k, cin, cout, stride, dilation, seed=5 + cin, bias=True, bn=True, transposed=transposed, wscale=0.05)
    x = activations((2, 9, 11, cin), seed=17)
    for relu in (False, True):
        got = run(x, conv, norm, relu)
        want, a, scale, shift = statement(x, conv, norm, relu, stride, dilation)
        w = conv.weight.detach().cpu().numpy()
        bound = np.abs(scale) * ref.error_bound(a, x.numpy(), w, k, cin, transposed) + 2.0 ** -23 * (np.abs(scale) * a + np.abs(shift))
        assert (np.abs(got - want) <= bound).all()
    packed = bev_conv.pack(conv, norm)
    wb, sb, tb = ref.unpack(packed.blob.cpu().numpy(), k, cin, cout)
    wl = w.transpose(1, 0, 2, 3) if transposed else w
    assert (np.abs(wb - wl) <= 2.0 ** -23 * np.abs(wl) + 2.0 ** -35 * np.abs(wl).max()).all()
    np.testing.assert_array_equal(sb, scale.astype(np.float32))
    np.testing.assert_array_equal(tb, shift.astype(np.float32))
    # and the device pack is the host pack, bit for bit
    np.testing.assert_array_equal(packed.blob.cpu().numpy(), ref.host_pack(w, sb, tb, transposed))


@pytest.mark.parametrize("cin,cout", [(32, 32), (128, 256)])
@pytest.mark.parametrize("k,stride,dilation", TAPS)
def test_impulse_pins_the_tap_geometry_and_both_cross_terms(k, stride, dilation, cin, cout):
    """One input pixel, one channel = 1 + 2^-12 (hi = 1, lo = 2^-12), every weight 1 + 2^-13: each output the impulse reaches
    is the float32 product within 1 ulp, every other one exactly 0 -- at every position of a 5 x 7 grid (sample b holds the
    impulse at position b).  A dropped hi lo or lo hi term is 2^-12 or 2^-13 off: 2048 / 1024 ulp."""
    H, W = 5, 7
    conv, _ = make_layer(k, cin, cout, stride, dilation, seed=1)
    with torch.no_grad():
        conv.weight.fill_(1.0 + 2.0 ** -13)
    x = torch.zeros(H * W, H, W, cin)
    for b in range(H * W):
        x[b, b // W, b % W, (7 * b) % cin] = 1.0 + 2.0 ** -12
    got = run(x, conv, None, False)
    want, _, _, _ = statement(x, conv, None, False, stride, dilation)
    assert set(np.unique(want)) <= {0.0, (1.0 + 2.0 ** -12) * (1.0 + 2.0 ** -13)}
    assert (got[want == 0.0] == 0.0).all()
    assert (np.abs(got - want)[want != 0.0] <= 2.0 ** -23).all()  # 1 ulp of a float32 in [1, 2)
    assert (want != 0.0).sum() > 0


@pytest.mark.parametrize("cin,cout,k,stride,dilation", [(128, 128, 3, 1, 2), (64, 64, 3, 2, 1), (128, 256, 1, 1, 1)])
def test_power_of_two_scaling_is_exact_and_mixed_ranges_stay_inside_the_bound(cin, cout, k, stride, dilation):
    conv, _ = make_layer(k, cin, cout, stride, dilation, seed=9)
    x = activations((2, 11, 13, cin), seed=4) + 2.0 ** -6  # (no zeros: every element really scales)
    base = run(x, conv, None, False)
    for p in (18, -20):
        assert np.array_equal(run(x * 2.0 ** p, conv, None, False), base * np.float32(2.0 ** p)), p
    mixed = x.clone()
    mixed[:, :, :6] *= 2.0 ** 10
    mixed[:, :, 6:] *= 2.0 ** -10
    got = run(mixed, conv, None, True)
    want, a, _, _ = statement(mixed, conv, None, True, stride, dilation)
    assert (np.abs(got - want) <= ref.error_bound(a, mixed.numpy(), conv.weight.detach().cpu().numpy(), k, cin)).all()
    # the small region keeps its own relative accuracy where no large pixel is in reach (per-pixel normalisation)
    far = want[:, :, (8 + dilation) // stride + 1:]
    assert (np.abs(got[:, :, (8 + dilation) // stride + 1:] - far) <= 2.0 ** -18 * np.abs(far).max()).all()


@pytest.mark.parametrize("relu", [False, True])
def test_non_finite_inputs_never_come_out_finite(relu):
    conv, norm = make_layer(3, 32, 64, 1, 1, seed=2, bn=True)
    x = activations((2, 6, 9, 32), seed=8)
    x[0, 2, 3, 5] = float("nan")
    x[1, 4, 8, 31] = float("inf")
    x[1, 0, 0, 0] = float("-inf")
    got = run(x, conv, norm, relu)
    want, _, _, _ = statement(x, conv, norm, relu, 1, 1)
    bad = ~np.isfinite(want)
    assert bad.sum() > 0 and not np.isfinite(got[bad]).any()
    clean = np.isfinite(want).all(axis=3) & (np.abs(want).max(axis=3) > 0)
    assert np.isfinite(got[clean]).all()  # and pixels out of their reach are untouched


def _raw_call(x, packed, relu, y, emap):
    B, H, W, C = x.shape
    _lib.call("mssvt_bev_conv", x.data_ptr(), B, H, W, C, packed.blob.data_ptr(), packed.ksize, packed.cout, packed.stride,
              packed.dilation, int(relu), emap.data_ptr(), y.data_ptr(), _lib.stream())


@pytest.mark.parametrize("cin,cout,k,stride,dilation,hw", [(128, 128, 3, 1, 2, (17, 19)), (32, 64, 3, 2, 2, (6, 7)),
                                                           (256, 256, 3, 1, 1, (3, 5))])
def test_reads_stay_inside_the_input_and_every_output_element_is_written(cin, cout, k, stride, dilation, hw):
    """The input is a slice of a NaN-filled allocation (a read outside it poisons the result); the output and the exponent
    workspace sit in NaN / -1 filled allocations: fully written inside, untouched outside."""
    conv, _ = make_layer(k, cin, cout, stride, dilation, seed=3)
    packed = bev_conv.pack(conv, None)
    B, (H, W) = 2, hw
    xs = activations((B, H, W, cin), seed=6)
    n, guard = xs.numel(), 4096
    big = torch.full((n + 2 * guard,), float("nan"), device=DEV)
    big[guard:guard + n] = xs.to(DEV).reshape(-1)
    x = big[guard:guard + n].view(B, H, W, cin)
    ho, wo = packed.out_size(H, W)
    ny = B * ho * wo * cout
    ybig = torch.full((ny + 2 * guard,), float("nan"), device=DEV)
    ebig = torch.full((B * H * W + 2 * guard,), -1, dtype=torch.int32, device=DEV)
    _raw_call(x, packed, False, ybig[guard:guard + ny], ebig[guard:guard + B * H * W])
    got = ybig[guard:guard + ny].view(B, ho, wo, cout).cpu().numpy()
    assert np.isfinite(got).all()
    assert bool(torch.isnan(ybig[:guard]).all()) and bool(torch.isnan(ybig[guard + ny:]).all())
    assert bool((ebig[:guard] == -1).all()) and bool((ebig[guard + B * H * W:] == -1).all())
    np.testing.assert_array_equal(got, run(xs, conv, None, False))  # the same bits as from a tight allocation


def test_bit_identical_across_calls_and_streams():
    conv, norm = make_layer(3, 128, 256, 2, 1, seed=12, bn=True)
    x = activations((3, 21, 23, 128), seed=13).to(DEV).permute(0, 3, 1, 2)
    packed = bev_conv.pack(conv, norm)
    first = bev_conv.conv_bn_act(x, packed, True)
    again = bev_conv.conv_bn_act(x, packed, True)
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(bev_conv.conv_bn_act(x, packed, True))
        s.synchronize()
    for o in [again] + outs:
        assert torch.equal(first, o)


def test_pack_and_convolution_never_synchronise_the_host():
    conv, norm = make_layer(3, 64, 64, 1, 2, seed=14, bn=True)
    x = activations((2, 9, 9, 64), seed=15).to(DEV).permute(0, 3, 1, 2)
    warm = bev_conv.conv_bn_act(x, bev_conv.pack(conv, norm), True)
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
            out = bev_conv.conv_bn_act(x, bev_conv.pack(conv, norm), True)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    assert torch.equal(warm, out)


def test_every_status_code_is_reached_and_nothing_is_launched():
    lib = _lib.lib()
    assert lib.mssvt_bev_conv_supported(3, 128, 128, 1, 1) == 1 and lib.mssvt_bev_conv_supported(1, 128, 256, 1, 1) == 1
    for bad in [(3, 48, 32, 1, 1), (3, 128, 128, 3, 1), (3, 128, 128, 1, 3), (1, 128, 128, 2, 1), (5, 128, 128, 1, 1), (2, 256, 256, 2, 1)]:
        assert lib.mssvt_bev_conv_supported(*bad) == 0, bad
    assert lib.mssvt_bev_conv_pack_bytes(3, 128, 256) == 64 + 8 * 256 + 4 * 9 * 128 * 256 == ref.pack_bytes(3, 128, 256)
    assert lib.mssvt_bev_conv_pack_bytes(3, 48, 32) == 0
    conv, _ = make_layer(3, 32, 32, 1, 1, seed=1)
    packed = bev_conv.pack(conv, None)
    before = packed.blob.clone()
    x = torch.zeros(1, 4, 4, 32, device=DEV)
    y = torch.full((1, 4, 4, 32), 7.0, device=DEV)
    e = torch.zeros(16, dtype=torch.int32, device=DEV)
    st = _lib.stream()
    xp, yp, ep, bp, wp = x.data_ptr(), y.data_ptr(), e.data_ptr(), packed.blob.data_ptr(), conv.weight.data_ptr()
    BAD, BIG = -1, -2
    assert lib.mssvt_bev_conv(None, 1, 4, 4, 32, bp, 3, 32, 1, 1, 0, ep, yp, st) == BAD
    assert lib.mssvt_bev_conv(xp, 0, 4, 4, 32, bp, 3, 32, 1, 1, 0, ep, yp, st) == BAD
    assert lib.mssvt_bev_conv(xp, 1, 4, 4, 32, bp, 3, 32, 1, 1, 0, None, yp, st) == BAD
    assert lib.mssvt_bev_conv(xp + 4, 1, 4, 4, 32, bp, 3, 32, 1, 1, 0, ep, yp, st) == BAD  # unaligned
    assert lib.mssvt_bev_conv(xp, 1, 4, 4, 48, bp, 3, 32, 1, 1, 0, ep, yp, st) == BIG
    assert lib.mssvt_bev_conv(xp, 1, 4, 4, 32, bp, 3, 32, 3, 1, 0, ep, yp, st) == BIG
    assert lib.mssvt_bev_conv(xp, 1 << 15, 1 << 8, 1 << 8, 32, bp, 3, 32, 1, 1, 0, ep, yp, st) == BIG  # 2^31 pixels
    assert lib.mssvt_bev_conv_pack(None, 0, None, None, None, None, None, 0.0, 3, 32, 32, bp, st) == BAD
    assert lib.mssvt_bev_conv_pack(wp, 1, None, None, None, None, None, 0.0, 3, 32, 32, bp, st) == BAD  # transposed needs k = 1
    assert lib.mssvt_bev_conv_pack(wp, 0, None, wp, None, None, None, 0.0, 3, 32, 32, bp, st) == BAD  # affine without statistics
    assert lib.mssvt_bev_conv_pack(wp, 0, None, None, None, wp, None, 0.0, 3, 32, 32, bp, st) == BAD  # mean without variance
    assert lib.mssvt_bev_conv_pack(wp, 0, None, None, None, None, None, 0.0, 3, 48, 32, bp, st) == BIG
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and torch.equal(packed.blob, before)
    assert b"bad argument" in lib.mssvt_hip_status_string(BAD)
    # the Python layer: no CPU path, channels-last fp32 only
    xc = torch.zeros(1, 32, 4, 4, device=DEV)
    for wrong in (xc, xc.cpu().contiguous(memory_format=torch.channels_last), xc.double().contiguous(memory_format=torch.channels_last),
                  torch.zeros(1, 64, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last), xc[0]):
        with pytest.raises(MssvtHipError):
            bev_conv.conv_bn_act(wrong, packed, True)
    with pytest.raises(MssvtHipError):
        bev_conv.pack(nn.Conv2d(48, 32, 3, padding=1).to(DEV))
    assert not bev_conv.supported(nn.Conv2d(32, 32, 3, padding=1))  # parameters on the CPU
    assert bev_conv.supported(conv, None) and not bev_conv.supported(conv, nn.BatchNorm2d(64).to(DEV))


def test_pack_is_cached_and_rebuilt_when_a_tensor_changes():
    conv, norm = make_layer(3, 32, 32, 1, 1, seed=21, bn=True)
    p0 = bev_conv.pack(conv, norm)
    assert bev_conv.pack(conv, norm) is p0
    with torch.no_grad():
        norm.running_var.add_(0.25)
    p1 = bev_conv.pack(conv, norm)
    assert p1 is not p0 and not torch.equal(p1.blob, p0.blob)
    with torch.no_grad():
        conv.weight.mul_(2.0)
    p2 = bev_conv.pack(conv, norm)
    assert p2 is not p1 and bev_conv.pack(conv, norm) is p2
    conv.load_state_dict(conv.state_dict())
    assert bev_conv.pack(conv, norm) is not p2
    p3 = bev_conv.pack(conv, None)  # another fold of the same convolution
    assert p3 is not p2 and float(ref.unpack(p3.blob.cpu().numpy(), 3, 32, 32)[1].min()) == 1.0


# ---- mssvt_dense_bev_nhwc -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,B,C,empty", [([8, 9, 1], 3, 40, 1), ([7, 9, 4], 2, 32, None), ([16, 5, 4], 3, 8, 0), ([33, 31, 1], 2, 128, None)])
def test_dense_bev_nhwc_is_the_dense_grid_made_channels_last(grid, B, C, empty):
    """Bit for bit dense().view(B, C Z, Y, X) in channels-last memory: Z = 1 and Z = 4, grids that end inside a tile, a sample
    without voxels."""
    from mssvt_amd.mssvt_utils import SparseTensor
    g = torch.Generator().manual_seed(sum(grid) + C)
    X, Y, Z = grid
    rows = []
    for b in range(B):
        if b == empty:
            continue
        cells = torch.randperm(X * Y * Z, generator=g)[:max(1, int(0.3 * X * Y * Z))].sort().values
        x, y, z = cells // (Y * Z), (cells // Z) % Y, cells % Z
        rows.append(torch.stack([torch.full_like(x, b), z, y, x], dim=1))
    vc = torch.cat(rows).int()
    feats = torch.randn(vc.shape[0], C, generator=g).to(DEV)
    sp = SparseTensor(features=feats, indices=vc.to(DEV), spatial_shape=grid, voxel_size=[0.3, 0.3, 0.2],
                      point_cloud_range=[0, 0, 0, 0.3 * X, 0.3 * Y, 0.2 * Z], batch_size=B, hash_size=100003)
    want = sp.dense().view(B, C * Z, Y, X)
    got = sp.dense_nhwc()
    assert got.shape == want.shape and bev_conv.is_channels_last(got)
    assert torch.equal(got, want)
    assert torch.equal(got.permute(0, 2, 3, 1).contiguous(), want.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1))
    if empty is not None:
        assert float(got[empty].abs().max()) == 0.0
    # the NaN-prefilled form: every element is written
    out = torch.full((B, Y, X, C * Z), float("nan"), device=DEV)
    _lib.call("mssvt_dense_bev_nhwc", feats.data_ptr(), C, sp.map_table.data_ptr(), int(sp.hash_size), sp.v_bs_cnt.data_ptr(), B,
              X, Y, Z, out.data_ptr(), _lib.stream())
    assert torch.equal(out.permute(0, 3, 1, 2), want)
    lib = _lib.lib()
    assert lib.mssvt_dense_bev_nhwc(None, C, sp.map_table.data_ptr(), 100003, sp.v_bs_cnt.data_ptr(), B, X, Y, Z, out.data_ptr(), None) == -1
    assert lib.mssvt_dense_bev_nhwc(feats.data_ptr(), 6, sp.map_table.data_ptr(), 100003, sp.v_bs_cnt.data_ptr(), B, X, Y, Z,
                                    out.data_ptr(), None) == -2
