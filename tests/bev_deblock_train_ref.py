"""A numpy float64 statement of a transposed deblock whose kernel equals its stride, ``ConvTranspose2d(cin, cout, s, stride=s)``
with s in {1, 2} and no bias, on channels-last tensors, and of its backward -- what ``bev_deblock_train.DeblockFunction``,
mssvt_bev_deblock_dgrad and mssvt_bev_deblock_wgrad compute.  x (B, H, W, cin), w (cin, cout, s, s), y / dy (B, s H, s W, cout):

    y[b, s iy + dy, s ix + dx, n] = sum_c x[b, iy, ix, c] w[c, n, dy, dx]
    dX[b, iy, ix, c]              = sum_{n, dy, dx} dY[b, s iy + dy, s ix + dx, n] w[c, n, dy, dx]
    dW[c, n, dy, dx]              = sum_{b, iy, ix} x[b, iy, ix, c] dY[b, s iy + dy, s ix + dx, n]

dX is an ordinary convolution of dY whose Conv2d weight is w exactly as stored, (cin, cout, s, s) read as (out, in, ky, kx),
at stride s with no padding: ``bev_conv_ref.conv(dy, w, stride=s, dilation=1, pad=0)``; its bound is that file's
``error_bound(a, dy, w, ksize=s, cin=cout)``, S = s^2 cout / 32 + 2.  The forward's bound is ``bev_conv_ref.error_bound(...,
transposed=True)`` (s = 1) / ``bev_up2_ref.error_bound`` (s = 2).

The weight gradient runs the arithmetic of csrc/split_wgrad.hip.h with the phases (dy, dx) as taps, x as the plain operand
(one power of two per slice of the B H W input pixels) and dY as the tapped one (one power of two per (slice, phase), over the
dY rows that phase reads).  The bound per element is therefore tests/bev_conv_train_ref.py's -- its docstring derives it -- with
a = |x|^T |dY_phase|:

    (3 2^-22 + S 2^-24) a + 2^-34 sum_s (max_s|x| sum_{p in s} |dY_p,n| + max_s|dY_phase| sum_{p in s} |x_p,c|)
    S = slice_pixels / 32 + slices + 2
"""
import numpy as np

from tests import bev_conv_ref, bev_up2_ref
from tests.bev_conv_train_ref import _pow2, _split, num_slices

SHAPES = ((1, 128, 256), (2, 256, 256), (1, 32, 64), (2, 64, 32))  # (stride, cin, cout)
SLICE_PIXELS = {(1, 128, 256): 1024, (2, 256, 256): 2048, (1, 32, 64): 256, (2, 64, 32): 256}  # as the header publishes them


def phases(s):
    return [(py, px) for py in range(s) for px in range(s)]


def phase_rows(dy, s, py, px):
    """The dY rows phase (py, px) reads, in the memory order of the input pixels: (B H W, cout)."""
    return dy[:, py::s, px::s].reshape(-1, dy.shape[3])


def y_ref(x, w, s):
    """(y, a, bound): (B, s H, s W, cout) float64 each."""
    if s == 1:
        y, a = bev_conv_ref.conv(x, w, transposed=True)
        return y, a, bev_conv_ref.error_bound(a, x, w, 1, x.shape[3], transposed=True)
    y, a = bev_up2_ref.up2(x, w)
    return y, a, bev_up2_ref.error_bound(a, x, w)


def dx_ref(dy, w, s):
    """(dx, a, bound): (B, H, W, cin) float64 each."""
    dx, a = bev_conv_ref.conv(dy, w, stride=s, dilation=1, pad=0)
    return dx, a, bev_conv_ref.error_bound(a, dy, w, ksize=s, cin=dy.shape[3])


def dw_ref(x, dy, s):
    """(cin, cout, s, s) float64."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    cin, cout = x.shape[3], dy.shape[3]
    dw = np.zeros((cin, cout, s, s))
    xr = x.reshape(-1, cin)
    with np.errstate(invalid="ignore", over="ignore"):
        for py, px in phases(s):
            dw[:, :, py, px] = xr.T @ phase_rows(dy, s, py, px)
    return dw


def dw_abs(x, dy, s):
    """a = |x|^T |dY_phase| per element."""
    return dw_ref(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(dy, np.float64)), s)


def dw_bound(x, dy, s, slice_pixels):
    """The bound of the module docstring, (cin, cout, s, s) float64."""
    x, dy = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(dy, np.float64))
    cin, cout = x.shape[3], dy.shape[3]
    xr = x.reshape(-1, cin)
    M = xr.shape[0]
    S = slice_pixels // 32 + num_slices(M, slice_pixels) + 2
    bound = np.zeros((cin, cout, s, s))
    for py, px in phases(s):
        rows = phase_rows(dy, s, py, px)
        u = np.zeros((cin, cout))
        for s0 in range(0, M, slice_pixels):
            xs, ys = xr[s0:s0 + slice_pixels], rows[s0:s0 + slice_pixels]
            u += 2.0 ** -34 * (xs.max() * ys.sum(0)[None, :] + ys.max() * xs.sum(0)[:, None])
        bound[:, :, py, px] = (3 * 2.0 ** -22 + S * 2.0 ** -24) * (xr.T @ rows) + u
    return bound


def dw_emulated(x, dy, s, slice_pixels):
    """(cin, cout, s, s) float32 as the split arithmetic gives it (the order inside a 32-pixel step is not modelled: the step's
    products are summed exactly and rounded once)."""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    cin, cout = x.shape[3], dy.shape[3]
    xr = x.reshape(-1, cin)
    M = xr.shape[0]
    dw = np.zeros((cin, cout, s, s), np.float32)
    for py, px in phases(s):
        rows = phase_rows(dy, s, py, px)
        out = None
        for s0 in range(0, M, slice_pixels):
            xs, ys = xr[s0:s0 + slice_pixels], rows[s0:s0 + slice_pixels]
            xi, xu = _pow2(np.abs(xs).max())
            yi, yu = _pow2(np.abs(ys).max())
            xh, xl = _split(xs * xi)
            yh, yl = _split(ys * yi)
            mm, cr = np.zeros((cin, cout), np.float32), np.zeros((cin, cout), np.float32)
            for k0 in range(0, len(xs), 32):
                k1 = k0 + 32
                mm = (mm.astype(np.float64) + xh[k0:k1].T @ yh[k0:k1]).astype(np.float32)
                cr = (cr.astype(np.float64) + xh[k0:k1].T @ yl[k0:k1] + xl[k0:k1].T @ yh[k0:k1]).astype(np.float32)
            part = (mm + cr * np.float32(1.0 / 2048)) * xu * yu
            out = part if out is None else out + part
        dw[:, :, py, px] = out
    return dw


def inputs(kind, B, H, W, s, cin, cout, seed):
    """x (B, H, W, cin), dy (B, s H, s W, cout) float32 of one of the three input kinds: Gaussian, heavy-tailed (2^-30 .. 1)
    and spiked."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, H, W, cin)).astype(np.float32)
    dy = rng.standard_normal((B, s * H, s * W, cout)).astype(np.float32)
    if kind == "tail":
        x *= (2.0 ** rng.integers(-24, 1, (B, H, W, 1))).astype(np.float32)
        dy *= (2.0 ** rng.integers(-30, 1, dy.shape)).astype(np.float32)
    elif kind == "spike":
        dy *= np.float32(1e-7)
        flat = dy.reshape(-1, cout)
        flat[rng.integers(0, flat.shape[0], 5)] = 1.0
    else:
        assert kind == "plain"
    return x, dy


def weights(s, cin, cout, seed):
    return (np.random.default_rng(seed).standard_normal((cin, cout, s, s)) * 0.05).astype(np.float32)
