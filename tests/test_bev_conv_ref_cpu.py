"""tests/bev_conv_ref.py (the float64 statement the GPU tests hold csrc/bev_conv.hip to) against
torch.nn.functional.conv2d + BatchNorm2d.eval() in float64 on the CPU, and the blob format's host-side writer / reader."""
import os
import re

import numpy as np
import pytest
import torch

from tests import bev_conv_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bn(rng, c, affine=True):
    return dict(mean=rng.normal(0, 0.5, c), var=rng.uniform(0.3, 2.0, c), eps=1e-3,
                weight=rng.uniform(0.5, 1.5, c) if affine else None, bias=rng.normal(0, 0.3, c) if affine else None)


def _torch_bn(bn, c):
    m = torch.nn.BatchNorm2d(c, eps=bn["eps"], affine=bn["weight"] is not None).double().eval()
    with torch.no_grad():
        m.running_mean.copy_(torch.from_numpy(bn["mean"]))
        m.running_var.copy_(torch.from_numpy(bn["var"]))
        if bn["weight"] is not None:
            m.weight.copy_(torch.from_numpy(bn["weight"]))
            m.bias.copy_(torch.from_numpy(bn["bias"]))
    return m


@pytest.mark.parametrize("k,stride,dilation", [(3, 1, 1), (3, 2, 1), (3, 1, 2), (3, 2, 2), (1, 1, 1)])
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 7), (6, 8), (9, 4)])
def test_statement_matches_torch_in_float64(k, stride, dilation, hw):
    rng = np.random.default_rng(k * 100 + stride * 10 + dilation + hw[0])
    B, cin, cout = 2, 6, 5
    x = rng.normal(size=(B,) + hw + (cin,))
    w = rng.normal(size=(cout, cin, k, k))
    bias = rng.normal(size=cout) if hw[0] % 2 else None
    bn = _bn(rng, cout, affine=hw[1] % 2 == 1)
    scale, shift = ref.fold(cout, bias, bn)
    for relu in (False, True):
        got, a = ref.conv(x, w, stride, dilation, scale=scale, shift=shift, relu=relu)
        pad = dilation if k == 3 else 0
        with torch.no_grad():
            t = torch.nn.functional.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w),
                                           None if bias is None else torch.from_numpy(bias), stride, pad, dilation)
            t = _torch_bn(bn, cout)(t)
            t = torch.relu(t) if relu else t
            ta = torch.nn.functional.conv2d(torch.from_numpy(np.abs(x)).permute(0, 3, 1, 2), torch.from_numpy(np.abs(w)), None,
                                            stride, pad, dilation)
        want = t.permute(0, 2, 3, 1).numpy()
        assert got.shape == want.shape
        assert got.shape[1] == (hw[0] + 2 * pad - dilation * (k - 1) - 1) // stride + 1
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(a, ta.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)


def test_zero_pad_then_padding_zero_is_the_padding_one_case():
    rng = np.random.default_rng(3)
    x, w = rng.normal(size=(1, 7, 6, 4)), rng.normal(size=(3, 4, 3, 3))
    got, _ = ref.conv(x, w, stride=2)
    with torch.no_grad():
        t = torch.nn.functional.conv2d(torch.nn.ZeroPad2d(1)(torch.from_numpy(x).permute(0, 3, 1, 2)), torch.from_numpy(w), None, 2, 0)
    np.testing.assert_allclose(got, t.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)


def test_transposed_1x1_layout_is_conv_transpose2d():
    rng = np.random.default_rng(4)
    x, wt = rng.normal(size=(2, 5, 3, 6)), rng.normal(size=(6, 4, 1, 1))
    got, _ = ref.conv(x, wt, transposed=True)
    with torch.no_grad():
        t = torch.nn.functional.conv_transpose2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wt), None, 1)
    np.testing.assert_allclose(got, t.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("k,cin,cout,transposed", [(3, 32, 32, False), (3, 32, 64, False), (1, 64, 64, True), (3, 128, 256, False),
                                                   (1, 256, 256, False)])
def test_host_unpacking_of_the_blob_returns_the_folded_weights(k, cin, cout, transposed):
    rng = np.random.default_rng(cin + cout + k)
    w = (rng.normal(size=(cout, cin, k, k)) * 37.0).astype(np.float32)
    w[0, 0, 0, 0] = 0.0
    w[1, 1, 0, 0] = 1e-9  # far below the tensor's power of two: an fp16 denormal hi, the lo half carries the rest
    wl = np.ascontiguousarray(w.transpose(1, 0, 2, 3)) if transposed else w
    scale, shift = ref.fold(cout, rng.normal(size=cout), _bn(rng, cout))
    blob = ref.host_pack(wl, scale.astype(np.float32), shift.astype(np.float32), transposed)
    assert blob.dtype == np.uint8 and blob.size == ref.pack_bytes(k, cin, cout)
    back, s2, t2 = ref.unpack(blob, k, cin, cout)
    np.testing.assert_array_equal(s2, scale.astype(np.float32))
    np.testing.assert_array_equal(t2, shift.astype(np.float32))
    # hi + lo / 2^11 with both halves rounded to nearest: the residual has up to 12 bits + sign, one more than lo holds, so
    # a value is off by at most 2^-23 of itself (a tie), or 2^-36 of the tensor's power of two where lo is an fp16 denormal
    top = 2.0 ** np.floor(np.log2(np.abs(w).max()))
    assert (np.abs(back - w) <= 2.0 ** -23 * np.abs(w) + 2.0 ** -35 * top).all()
    assert back[0, 0, 0, 0] == 0.0


def test_python_tile_constants_are_the_header_s():
    from mssvt_amd import bev_conv
    hdr = open(os.path.join(ROOT, "include", "mssvt_hip.h")).read()
    assert int(re.search(r"#define MSSVT_BEV_CONV_WAVE_PIXELS (\d+)", hdr).group(1)) == bev_conv.WAVE_PIXELS
    assert int(re.search(r"#define MSSVT_BEV_CONV_BLOCK_PIXELS (\d+)", hdr).group(1)) == bev_conv.BLOCK_PIXELS


def test_layer_shape_reads_the_tap_sets():
    from torch import nn
    from mssvt_amd import bev_conv
    assert bev_conv.layer_shape(nn.Conv2d(128, 128, 3, padding=2, dilation=2, bias=False)) == (3, 128, 128, 1, 2, False)
    assert bev_conv.layer_shape(nn.Conv2d(128, 256, 3, stride=2, padding=0), pad=1) == (3, 128, 256, 2, 1, False)
    assert bev_conv.layer_shape(nn.Conv2d(128, 256, 3, stride=2, padding=0)) is None  # padding != dilation
    assert bev_conv.layer_shape(nn.ConvTranspose2d(128, 256, 1, stride=1, bias=False)) == (1, 128, 256, 1, 1, True)
    assert bev_conv.layer_shape(nn.ConvTranspose2d(256, 256, 2, stride=2, bias=False)) is None
    assert bev_conv.layer_shape(nn.Conv2d(64, 64, 3, padding=1, groups=2)) is None
    assert bev_conv.layer_shape(nn.Conv2d(64, 64, (3, 1), padding=(1, 0))) is None
    for shape in bev_conv.ROUTED:
        assert shape[1:3] in bev_conv.CHANNEL_SHAPES and shape[1:3] not in bev_conv.GOLDEN_CHANNELS
