"""tests/head_conv_train_ref.py held to torch autograd in float64 (conv2d + bias; the trunk as nb modules reading one tensor)
and to a float32 emulation of the kernels' order, which must stay inside the statement's bounds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bev_conv_train_ref as tref, head_conv_train_ref as ref

SIZES = [(1, 1, 1), (2, 3, 5), (1, 4, 6), (2, 5, 4)]  # one pixel, odd, even, mixed


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def nchw(a):
    return t64(a).permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_shared_layer_matches_torch_autograd_in_float64(size, bias):
    B, H, W = size
    cin, s = 8, 4
    rng = np.random.default_rng(H * 10 + W + bias)
    x, dy = rng.standard_normal((B, H, W, cin)), rng.standard_normal((B, H, W, s))
    w = rng.standard_normal((s, cin, 3, 3))
    b = rng.standard_normal(s) if bias else None
    xt, wt = nchw(x).requires_grad_(), t64(w).requires_grad_()
    bt = t64(b).requires_grad_() if bias else None
    yt = F.conv2d(xt, wt, bt, padding=1)
    yt.backward(nchw(dy))
    np.testing.assert_allclose(ref.forward(x, w, b)[0], nhwc(yt.detach()), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref.dx(dy, w)[0], nhwc(xt.grad), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref.dw(x, dy)[0], wt.grad.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(tref.dx_ref(dy, w, 1), nhwc(xt.grad), rtol=1e-12, atol=1e-12)  # the two statements of dX agree
    if bias:
        np.testing.assert_allclose(ref.db(dy)[0], bt.grad.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_trunk_matches_nb_modules_reading_one_tensor(size, nb, bias):
    B, H, W = size
    s = 4
    rng = np.random.default_rng(H * 10 + W + nb)
    y = rng.standard_normal((B, H, W, s))
    ws = [rng.standard_normal((s, s, 3, 3)) for _ in range(nb)]
    bs = [rng.standard_normal(s) if bias else None for _ in range(nb)]
    dts = [rng.standard_normal((B, H, W, s)) for _ in range(nb)]
    yt = nchw(y).requires_grad_()
    mods = []
    for w, b in zip(ws, bs):
        m = torch.nn.Conv2d(s, s, 3, padding=1, bias=bias).double()
        with torch.no_grad():
            m.weight.copy_(t64(w))
            if bias:
                m.bias.copy_(t64(b))
        mods.append(m)
    outs = [m(yt) for m in mods]
    torch.autograd.backward(outs, [nchw(d) for d in dts])
    for (t, _), o in zip(ref.trunk_forward(y, ws, bs), outs):
        np.testing.assert_allclose(t, nhwc(o.detach()), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref.trunk_dy(dts, ws)[0], nhwc(yt.grad), rtol=1e-12, atol=1e-12)
    for (g, _), (gb, _), m in zip(ref.trunk_dw(y, dts), ref.trunk_db(dts), mods):
        np.testing.assert_allclose(g, m.weight.grad.numpy(), rtol=1e-12, atol=1e-12)
        if bias:
            np.testing.assert_allclose(gb, m.bias.grad.numpy(), rtol=1e-12, atol=1e-12)


def inside(got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: worst error / bound %.3f" % (what, ratio))
    assert (err <= bound).all(), (what, ratio)
    assert (bound > 0).any()


@pytest.mark.parametrize("kind", ["plain", "tail"])
def test_the_emulated_convolutions_stay_inside_the_bounds(kind):
    """The shared forward (with bias), its dX and the trunk's dy (three branches, one 2^20 above the others) in the kernel's
    order of float32 operations."""
    cin, s, nb = 64, 32, 3
    x, dy = tref.inputs(kind, 2, 3, 5, cin, s, seed=3)
    w = ref.weights(s, cin, 4)
    bias = np.random.default_rng(5).standard_normal(s).astype(np.float32)
    want, bound = ref.forward(x, w, bias)
    inside(ref.conv_emulated([x], [w], bias), want, bound, "y %s" % kind)
    want, bound = ref.dx(dy, w)
    inside(ref.conv_emulated([dy], [ref.rot_t(w)]), want, bound, "dX %s" % kind)
    ws = [ref.weights(s, s, 6 + b) for b in range(nb)]
    dts = [tref.inputs(kind, 2, 3, 5, s, s, seed=10 + b)[1] * np.float32(2.0 ** (20 * (b == 1))) for b in range(nb)]
    want, bound = ref.trunk_dy(dts, ws)
    inside(ref.conv_emulated(dts, [ref.rot_t(w) for w in ws]), want, bound, "trunk dy %s" % kind)


@pytest.mark.parametrize("kind", ["plain", "tail", "spike"])
def test_the_emulated_gradients_of_the_parameters_stay_inside_the_bounds(kind):
    """dW on a rectangular (S, cin) problem either side of a slice and db in the kernel's order, with short slices / pieces."""
    cin, s = 64, 32
    x, dy = tref.inputs(kind, 2, 7, 5, cin, s, seed=8)  # 70 pixels: three slices of 32, the second spans both samples
    want, bound = ref.dw(x, dy, 32)
    inside(tref.dw_emulated(x, dy, 1, 32), want, bound, "dW %s" % kind)
    for piece in (32, 64, 2048):
        want, bound = ref.db(dy, piece)
        inside(ref.db_emulated(dy, piece), want, bound, "db %s piece %d" % (kind, piece))


def test_the_bias_bound_follows_the_stated_depth():
    assert ref.db_depth(1, 32) == 0 + 31 + 0
    assert ref.db_depth(2048, 64) == 127 + 15 + 0
    assert ref.db_depth(2049, 32) == 63 + 31 + 1
    assert ref.db_depth(470 * 470, 64) == 127 + 15 + 107
