"""A numpy float64 statement of the 3 x 3 stride-2 convolution ``Conv2d(cin, cout, 3, stride=2, padding=1, bias=False)`` on
channels-last tensors and of its backward -- what ``bev_down_train.DownFunction``, mssvt_bev_down_dgrad and
mssvt_bev_down_wgrad compute.  x (B, H, W, cin), w (cout, cin, 3, 3), y / dy (B, Ho, Wo, cout), Ho = (H - 1) // 2 + 1:

    y [b, oy, ox, o]  = sum_{c, ky, kx} x[b, 2 oy + ky - 1, 2 ox + kx - 1, c] w[o, c, ky, kx]              (outside the image: 0)
    dW[o, c, ky, kx]  = sum_{b, oy, ox} dY[b, oy, ox, o] x[b, 2 oy + ky - 1, 2 ox + kx - 1, c]
    dX[b, iy, ix, c]  = sum_o sum_{(ky, oy): 2 oy + ky - 1 = iy} sum_{(kx, ox): 2 ox + kx - 1 = ix} dY[b, oy, ox, o] w[o, c, ky, kx]

y is ``bev_conv_ref.conv(x, w, stride=2)`` with ``bev_conv_ref.error_bound(a, x, w, 3, cin)``.

dX (``dx_ref`` is the direct sum, ``dx_phases`` the form the kernel runs).  By the parity (py, px) of (iy, ix) dX falls into
four phases: iy = 2 j takes ky = 1 at oy = j; iy = 2 j + 1 takes ky = 2 at oy = j and ky = 0 at oy = j + 1 (absent when
j + 1 = Ho); the same in x (``PHASE_TAPS``).  Phase (py, px) is a dense (1 + py) x (1 + px) convolution cout -> cin over dY
with t = (1 + py)(1 + px) taps, run on the arithmetic of csrc/split_conv.hip.h (tests/bev_conv_ref.py's ``error_bound``
states it): one accumulation chain per element with one step per (tap, 32 channels of dY) and the epilogue's two,

    (3 2^-22 + S 2^-24) a + 2^-24 max|dY| sum_{o, taps of the phase} |w[o, c, ky, kx]|,     S = t cout / 32 + 2,

a = |dY| conv |w| over the phase's taps.  This is ``error_bound(a, dy, w, ksize=3, cin=cout)`` on the rotated weights with
the phase's own step count (t <= 4 < 9) and the phase's own weights in the absolute term (a subset of the nine taps): never
looser than it.

dW runs the arithmetic of csrc/split_wgrad.hip.h with dY as the plain operand (one power of two per slice of the B Ho Wo
OUTPUT pixels in memory order) and x as the tapped one, read at (2 oy + ky - 1, 2 ox + kx - 1) (one power of two per
(slice, tap), over the x rows that tap reads; a tap outside the image loads neither row).  The bound per element is therefore
tests/bev_conv_train_ref.py's -- its docstring derives every constant -- with the tap rows read at stride 2 and the slices cut
over the output pixels:

    (3 2^-22 + S 2^-24) a + 2^-34 sum_s (max_s|dY| sum_{p in s} |X_p,c| + max_s|X| sum_{p in s} |dY_p,o|)
    S = slice_pixels / 32 + slices + 2
"""
import numpy as np

from tests import bev_conv_ref, bev_conv_train_ref
from tests.bev_conv_train_ref import _pow2, _split, num_slices

SHAPES = ((128, 256), (32, 64))  # (cin, cout)
SLICE_PIXELS = {(128, 256): 2048, (32, 64): 256}  # as the header publishes them
TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]
AXIS_TAPS = {0: [(1, 0)], 1: [(2, 0), (0, 1)]}  # parity -> [(k, offset into the dY grid)]
PHASES = [(py, px) for py in range(2) for px in range(2)]
# phase -> [(ky, kx, offset y, offset x)]
PHASE_TAPS = {(py, px): [(ky, kx, oy, ox) for ky, oy in AXIS_TAPS[py] for kx, ox in AXIS_TAPS[px]] for py, px in PHASES}


def out_size(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def y_ref(x, w):
    """(y, a, bound): (B, Ho, Wo, cout) float64 each."""
    y, a = bev_conv_ref.conv(x, w, stride=2)
    return y, a, bev_conv_ref.error_bound(a, x, w, 3, x.shape[3])


def tap_rows(x, ky, kx):
    """The rows the tap reads: (B Ho Wo, C) with row (b, oy, ox) = x[b, 2 oy + ky - 1, 2 ox + kx - 1] or zeros outside the
    image, and the (B Ho Wo,) mask of the output pixels whose tap falls inside."""
    B, H, W, C = x.shape
    Ho, Wo = out_size(H, W)
    xp = np.zeros((B, 2 * Ho + 1, 2 * Wo + 1, C), x.dtype)
    inside = np.zeros((2 * Ho + 1, 2 * Wo + 1), bool)
    xp[:, 1:1 + H, 1:1 + W] = x
    inside[1:1 + H, 1:1 + W] = True
    rows = xp[:, ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2]
    mask = np.broadcast_to(inside[ky:ky + 2 * Ho - 1:2, kx:kx + 2 * Wo - 1:2], (B, Ho, Wo))
    return rows.reshape(B * Ho * Wo, C), mask.reshape(-1)


def dw_ref(x, dy):
    """(cout, cin, 3, 3) float64."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    cout, cin = dy.shape[3], x.shape[3]
    dw = np.zeros((cout, cin, 3, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for ky, kx in TAPS:
            rows, mask = tap_rows(x, ky, kx)
            dw[:, :, ky, kx] = np.where(mask[:, None], dy.reshape(-1, cout), 0.0).T @ rows  # (no term, not a zero factor)
    return dw


def dw_abs(x, dy):
    """a = |dY|^T |X| per element."""
    return dw_ref(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(dy, np.float64)))


def dx_ref(dy, w, H, W):
    """The direct sum: (B, H, W, cin) float64."""
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    B, Ho, Wo, _ = dy.shape
    assert (Ho, Wo) == out_size(H, W)
    dx = np.zeros((B, H, W, w.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for oy in range(Ho):
            for ox in range(Wo):
                for ky, kx in TAPS:
                    iy, ix = 2 * oy + ky - 1, 2 * ox + kx - 1
                    if 0 <= iy < H and 0 <= ix < W:
                        dx[:, iy, ix] += dy[:, oy, ox] @ w[:, :, ky, kx]
    return dx


def phase_size(H, W, py, px):
    """The phase's grid: the pixels of an H x W image with that parity."""
    return (H + 1 - py) // 2, (W + 1 - px) // 2


def dx_phases(dy, w, H, W):
    """(dx, a, bound): (B, H, W, cin) float64 each, by the four phases; a tap beyond the dY grid adds no term."""
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    B, Ho, Wo, cout = dy.shape
    assert (Ho, Wo) == out_size(H, W)
    cin = w.shape[1]
    dx, a, bound = np.zeros((B, H, W, cin)), np.zeros((B, H, W, cin)), np.zeros((B, H, W, cin))
    dmax = np.abs(dy).max()
    with np.errstate(invalid="ignore", over="ignore"):
        for py, px in PHASES:
            hp, wp = phase_size(H, W, py, px)
            if hp == 0 or wp == 0:
                continue
            taps = PHASE_TAPS[(py, px)]
            v, av, wsum = np.zeros((B, hp, wp, cin)), np.zeros((B, hp, wp, cin)), np.zeros(cin)
            for ky, kx, oy, ox in taps:
                h1, w1 = min(hp, Ho - oy), min(wp, Wo - ox)  # the pixels whose tap lies inside the dY grid
                rows = dy[:, oy:oy + h1, ox:ox + w1]
                v[:, :h1, :w1] += rows @ w[:, :, ky, kx]
                av[:, :h1, :w1] += np.abs(rows) @ np.abs(w[:, :, ky, kx])
                wsum += np.abs(w[:, :, ky, kx]).sum(0)
            S = len(taps) * cout // 32 + 2
            dx[:, py::2, px::2], a[:, py::2, px::2] = v, av
            bound[:, py::2, px::2] = (3 * 2.0 ** -22 + S * 2.0 ** -24) * av + 2.0 ** -24 * dmax * wsum
    return dx, a, bound


def dx_bound_3x3(a, dy, w):
    """The 3 x 3 bound on the rotated weights (ksize 3, cin = cout): what ``dx_phases``' bound may never exceed."""
    rot = np.asarray(w, np.float64)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3)
    return bev_conv_ref.error_bound(a, dy, rot, 3, dy.shape[3])


def dw_bound(x, dy, slice_pixels):
    """The bound of the module docstring, (cout, cin, 3, 3) float64."""
    x, dy = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(dy, np.float64))
    cout, cin = dy.shape[3], x.shape[3]
    dyr = dy.reshape(-1, cout)
    M = dyr.shape[0]
    S = slice_pixels // 32 + num_slices(M, slice_pixels) + 2
    bound = np.zeros((cout, cin, 3, 3))
    for ky, kx in TAPS:
        rows, mask = tap_rows(x, ky, kx)
        dym = np.where(mask[:, None], dyr, 0.0)
        u = np.zeros((cout, cin))
        for s0 in range(0, M, slice_pixels):
            xs, ys, yall = rows[s0:s0 + slice_pixels], dym[s0:s0 + slice_pixels], dyr[s0:s0 + slice_pixels]
            u += 2.0 ** -34 * (yall.max() * xs.sum(0)[None, :] + xs.max() * ys.sum(0)[:, None])
        bound[:, :, ky, kx] = (3 * 2.0 ** -22 + S * 2.0 ** -24) * (dym.T @ rows) + u
    return bound


def dw_emulated(x, dy, slice_pixels):
    """(cout, cin, 3, 3) float32 as the split arithmetic gives it (the order inside a 32-pixel step is not modelled: the step's
    products are summed exactly and rounded once)."""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    cout, cin = dy.shape[3], x.shape[3]
    dyr = dy.reshape(-1, cout)
    M = dyr.shape[0]
    dw = np.zeros((cout, cin, 3, 3), np.float32)
    for ky, kx in TAPS:
        rows, mask = tap_rows(x, ky, kx)
        dym = np.where(mask[:, None], dyr, np.float32(0))
        out = None
        for s0 in range(0, M, slice_pixels):
            xs, ys = rows[s0:s0 + slice_pixels], dym[s0:s0 + slice_pixels]
            xi, xu = _pow2(np.abs(xs).max())
            yi, yu = _pow2(np.abs(dyr[s0:s0 + slice_pixels]).max())
            xh, xl = _split(xs * xi)
            yh, yl = _split(ys * yi)
            mm, cr = np.zeros((cout, cin), np.float32), np.zeros((cout, cin), np.float32)
            for k0 in range(0, len(xs), 32):
                k1 = k0 + 32
                mm = (mm.astype(np.float64) + yh[k0:k1].T @ xh[k0:k1]).astype(np.float32)
                cr = (cr.astype(np.float64) + yh[k0:k1].T @ xl[k0:k1] + yl[k0:k1].T @ xh[k0:k1]).astype(np.float32)
            part = (mm + cr * np.float32(1.0 / 2048)) * yu * xu
            out = part if out is None else out + part
        dw[:, :, ky, kx] = out
    return dw


def inputs(kind, B, H, W, cin, cout, seed):
    """x (B, H, W, cin), dy (B, Ho, Wo, cout) float32 of one of bev_conv_train_ref's three input kinds."""
    Ho, Wo = out_size(H, W)
    x = bev_conv_train_ref.inputs(kind, B, H, W, cin, cout, seed)[0]
    dy = bev_conv_train_ref.inputs(kind, B, Ho, Wo, cin, cout, seed + 1000)[1]
    return x, dy


def weights(cin, cout, seed):
    return (np.random.default_rng(seed).standard_normal((cout, cin, 3, 3)) * 0.05).astype(np.float32)
