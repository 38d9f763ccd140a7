"""A numpy float64 statement of the backward of a 3 x 3, stride-1 convolution with dilation d and zero padding d on
channels-last tensors -- what mssvt_bev_conv_wgrad and ``bev_conv_train.Conv3x3Function`` compute -- and of the error bound
the weight-gradient kernel is held to.  x (B, H, W, cin), dy (B, H, W, cout), w (cout, cin, 3, 3):

    dW[o, c, ky, kx] = sum_{b, y, x} dY[b, y, x, o] X[b, y + (ky - 1) d, x + (kx - 1) d, c]            (outside the image: 0)
    dX[b, y, x, c]   = sum_{o, ky, kx} dY[b, y - (ky - 1) d, x - (kx - 1) d, o] W[o, c, ky, kx]        (outside the image: 0)

The bound (``dw_bound``), per element, with a = |dY|^T |X| of the tap and the slices s of the kernel's slice rule (the B H W
pixels in memory order cut every ``slice_pixels``):

    (3 2^-22 + S 2^-24) a + 2^-34 sum_s (max_s|dY| sum_{p in s} |X_p,c| + max_s|X| sum_{p in s} |dY_p,o|)
    S = slice_pixels / 32 + slices + 2

Where the constants come from (the arithmetic of csrc/split_wgrad.hip.h):
  * a slice's dY rows are scaled by the exact power of two 2^-e, e the exponent of max_s|dY| over the slice's pixels (all
    channels), the X rows the tap reads by that of max_s|X| over those rows: every scaled value lies in (-2, 2).  The scaling
    and its undoing are exact, so they add nothing;
  * a scaled operand v is carried as hi = fp16(v), lo = fp16((v - hi) 2^11), both rounded to nearest.  With normal halves
    |v - hi| <= 2^-11 |v| and lo is off by at most 2^-11 of that: hi + 2^-11 lo is off by at most 2^-23 |v|.  Where a half
    falls into fp16's subnormal range its error is absolute, at most 2^-25 for hi -- which lo then carries -- and at most
    2^-25 2^-11 = 2^-36 for lo: |error of v| <= 2^-23 |v| + 2^-36;
  * a product is hi hi + 2^-11 (hi lo + lo hi); the dropped lo lo is at most 2^-22 of it (plus such an absolute term).  Per
    product: (2^-23 + 2^-23 + 2^-22) = 2 2^-22 of |dY X|, and 2^-36 (|dY~| + |X~|) + 2^-36 |X~| in scaled units; undone by
    2^e_d 2^e_x with 2^e_d <= max_s|dY| and 2^e_x <= max_s|X| that is at most 3 2^-36 (max_s|dY| |X| + max_s|X| |dY|).  The
    statement keeps 3 2^-22 (one 2^-22 for the second-order terms) and 2^-34;
  * the fp16 products are exact in fp32 and every K step of 32 pixels adds one rounded sum to an fp32 accumulator whose
    magnitude never exceeds a: 2^-24 a per step, slice_pixels / 32 steps; then one rounding per slice added in the ordered
    sum over slices, one for cr 2^-11 + mm and one spare: S.
"""
import numpy as np

TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def tap_rows(x, ky, kx, d):
    """The rows the tap reads: (B H W, C) with row (b, y, x) = x[b, y + (ky - 1) d, x + (kx - 1) d] or zeros outside the image,
    and the (B H W,) mask of the pixels whose tap falls inside."""
    B, H, W, C = x.shape
    out = np.zeros_like(x)
    mask = np.zeros((B, H, W), dtype=bool)
    oy, ox = (ky - 1) * d, (kx - 1) * d
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 < y1 and x0 < x1:
        out[:, y0:y1, x0:x1] = x[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        mask[:, y0:y1, x0:x1] = True
    return out.reshape(B * H * W, C), mask.reshape(-1)


def dw_ref(x, dy, d):
    """(cout, cin, 3, 3) float64."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    cout, cin = dy.shape[3], x.shape[3]
    dw = np.zeros((cout, cin, 3, 3))
    for ky, kx in TAPS:
        rows, mask = tap_rows(x, ky, kx, d)
        dw[:, :, ky, kx] = np.where(mask[:, None], dy.reshape(-1, cout), 0.0).T @ rows  # (no term, not a zero factor)
    return dw


def dw_abs(x, dy, d):
    """a = |dY|^T |X| per element."""
    return dw_ref(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(dy, np.float64)), d)


def dx_ref(dy, w, d):
    """(B, H, W, cin) float64."""
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    B, H, W, cout = dy.shape
    dx = np.zeros((B * H * W, w.shape[1]))
    for ky, kx in TAPS:
        rows, _ = tap_rows(dy, 2 - ky, 2 - kx, d)  # dY[b, y - (ky - 1) d, x - (kx - 1) d]
        dx += rows @ w[:, :, ky, kx]
    return dx.reshape(B, H, W, -1)


def num_slices(pixels, slice_pixels):
    return -(-pixels // slice_pixels)


def dw_bound(x, dy, d, slice_pixels):
    """The bound of the module docstring, (cout, cin, 3, 3) float64."""
    x, dy = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(dy, np.float64))
    cout, cin = dy.shape[3], x.shape[3]
    M = x.shape[0] * x.shape[1] * x.shape[2]
    S = slice_pixels // 32 + num_slices(M, slice_pixels) + 2
    dyr = dy.reshape(M, cout)
    bound = np.zeros((cout, cin, 3, 3))
    for ky, kx in TAPS:
        rows, mask = tap_rows(x, ky, kx, d)
        dym = np.where(mask[:, None], dyr, 0.0)
        u = np.zeros((cout, cin))
        for s0 in range(0, M, slice_pixels):
            xs, ys, yall = rows[s0:s0 + slice_pixels], dym[s0:s0 + slice_pixels], dyr[s0:s0 + slice_pixels]
            u += 2.0 ** -34 * (yall.max() * xs.sum(0)[None, :] + xs.max() * ys.sum(0)[:, None])
        bound[:, :, ky, kx] = (3 * 2.0 ** -22 + S * 2.0 ** -24) * (dym.T @ rows) + u
    return bound


# ---- an emulation of the kernel's arithmetic in numpy (fp16 casts, fp32 accumulation per 32-pixel step, ordered slice sums)
def _pow2(m):
    e = np.float32(m).view(np.uint32) & np.uint32(0x7F800000)
    if e == 0 or e >= 0x7F000000:
        return np.float32(1), np.float32(1)
    return np.uint32(0x7F000000 - e).view(np.float32), np.uint32(e).view(np.float32)


def _split(v):
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def dw_emulated(x, dy, d, slice_pixels):
    """(cout, cin, 3, 3) float32 as the split arithmetic gives it (the order inside a 32-pixel step is not modelled: the step's
    products are summed exactly and rounded once)."""
    x, dy = np.asarray(x, np.float32), np.asarray(dy, np.float32)
    cout, cin = dy.shape[3], x.shape[3]
    M = x.shape[0] * x.shape[1] * x.shape[2]
    dyr = dy.reshape(M, cout)
    dw = np.zeros((cout, cin, 3, 3), np.float32)
    for ky, kx in TAPS:
        rows, mask = tap_rows(x, ky, kx, d)
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
    """x, dy float32 of one of the three input kinds: Gaussian, heavy-tailed (2^-30 .. 1) and spiked."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, H, W, cin)).astype(np.float32)
    dy = rng.standard_normal((B, H, W, cout)).astype(np.float32)
    if kind == "tail":
        x *= (2.0 ** rng.integers(-24, 1, (B, H, W, 1))).astype(np.float32)
        dy *= (2.0 ** rng.integers(-30, 1, (B, H, W, cout))).astype(np.float32)
    elif kind == "spike":
        dy *= np.float32(1e-7)
        flat = dy.reshape(-1, cout)
        flat[rng.integers(0, flat.shape[0], 5)] = 1.0
    else:
        assert kind == "plain"
    return x, dy
