"""float64 numpy statement of the up-2 operator (csrc/bev_conv.hip, mssvt_bev_up2): a 2 x 2 stride-2 transposed convolution
with the eval-mode BatchNorm fold on NHWC tensors,

    y[b, 2 iy + dy, 2 ix + dx, n] = act(scale[n] * sum_c x[b, iy, ix, c] w[c, n, dy, dx] + shift[n]),

plus a = sum_c |x| |w| per output element (the measure of the operator's error bound).  Every output element has ONE tap, so
the bound is the family's (tests/test_bev_conv_gpu.py) at one tap: S = cin / 32 + 2 accumulation steps.
Not a test module: tests/test_bev_up2_ref_cpu.py holds it to torch in float64, the GPU tests hold the kernel to it."""
import numpy as np

from tests.bev_conv_ref import fold  # noqa: F401  (the BatchNorm fold is the family's)


def up2(x, w, scale=None, shift=None, relu=False):
    """x (B, H, W, Cin), w (Cin, Cout, 2, 2) as ConvTranspose2d holds it.  Returns (y, a), both (B, 2H, 2W, Cout) float64."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    B, H, W, cin = x.shape
    assert w.shape[0] == cin and w.shape[2:] == (2, 2)
    cout = w.shape[1]
    y = np.zeros((B, 2 * H, 2 * W, cout))
    a = np.zeros((B, 2 * H, 2 * W, cout))
    with np.errstate(invalid="ignore", over="ignore"):
        for dy in range(2):
            for dx in range(2):
                y[:, dy::2, dx::2] = x @ w[:, :, dy, dx]
                a[:, dy::2, dx::2] = np.abs(x) @ np.abs(w[:, :, dy, dx])
        if scale is not None:
            y = y * np.asarray(scale, np.float64)
        if shift is not None:
            y = y + np.asarray(shift, np.float64)
        if relu:
            y = np.where(y < 0, 0.0, y)  # a NaN stays a NaN
    return y, a


def steps(cin):
    """Accumulation steps per output element: one per 32 input channels (one tap), + the epilogue's two."""
    return cin // 32 + 2


def error_bound(a, x, w):
    """(3 2^-22 + S 2^-24) a + 2^-24 max|x| sum_c |w[c, n, dy, dx]| per output element (B, 2H, 2W, Cout)."""
    w = np.abs(np.asarray(w, np.float64))
    cin = w.shape[0]
    wsum = np.zeros(a.shape[1:])  # (2H, 2W, Cout): the output element's own phase
    for dy in range(2):
        for dx in range(2):
            wsum[dy::2, dx::2] = w[:, :, dy, dx].sum(axis=0)
    return (3 * 2.0 ** -22 + steps(cin) * 2.0 ** -24) * a + 2.0 ** -24 * np.abs(np.asarray(x, np.float64)).max() * wsum
