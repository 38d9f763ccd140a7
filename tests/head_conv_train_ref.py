"""A numpy float64 statement of CenterHead's shared layer and trunk in training mode (csrc/head_conv.hip's mssvt_head_conv_*_train,
*_dgrad, *_wgrad and mssvt_head_conv_bgrad; ``mssvt_amd.head_conv_train``) with per-element error bounds taken from the project's
own statements.  All tensors channels-last: x (B, H, W, cin), w (S, cin, 3, 3), bias (S) or None; the trunk: y (B, H, W, S),
ws = nb tensors (S, S, 3, 3), dts = nb tensors (B, H, W, S).

    y  = conv3x3(x, w) + bias                                           bound: tests/head_conv_ref.py's ``stage`` (the bound
                                                                        ``bev_conv_ref.error_bound(a, x, w, 3, cin)``; with a bias
                                                                        the fold's 2^-23 (a + |bias|) on top, scale = 1)
    dX = conv3x3(dY, rot(w)^T)     (bev_conv_train_ref.dx_ref)           bound: ``bev_conv_ref.error_bound(a, dY, rot(w)^T, 3, S)``
    dW = bev_conv_train_ref.dw_ref(x, dY, 1)                            bound: ``bev_conv_train_ref.dw_bound`` with this layer's
                                                                        slice length
    db = sum over the pixels of dY                                      bound: below
    trunk: t_b = conv3x3(y, w_b) + bias_b;  dy = sum_b dX(dT_b, w_b) -- ONE convolution of nb S input channels over the dT_b side
    by side: bound ``bev_conv_ref.error_bound(a, dT, W, 3, nb S)`` with max|dT| over ALL branches (the kernel's chain and its
    power of two are shared);  dW_b = dw_ref(y, dT_b) with ``dw_bound(y, dT_b)``: each branch's own dT_b (the kernel normalises
    every branch's rows of a slice on that branch alone, so a branch 2^20 below another keeps its own bound).

The bias gradient's bound.  The kernel cuts the P = B H W rows into pieces of R = ``bias_piece_rows`` rows; in a piece the
G = 1024 / S threads of a column each add their rows g, g + G, ... in row order (at most ceil(R / G) terms: ceil(R / G) - 1
additions, the first term is added to 0 exactly), the G partial sums are added in order of g (G - 1 additions), and the pieces'
sums are added in piece order (pieces - 1 additions).  Every addition rounds once (2^-24 relative) a partial sum whose magnitude is
at most the sum of |dY| over the terms it holds, and every term passes through at most
    D = (ceil(R / G) - 1) + (G - 1) + (pieces - 1)
additions, so by the standard bound for a summation tree of depth D
    |db - exact| <= gamma_D sum_p |dY_p,c|,   gamma_D = D u / (1 - D u),  u = 2^-24.
Not a test module: tests/test_head_conv_train_ref_cpu.py holds it to torch autograd in float64."""
import numpy as np

from tests import bev_conv_ref, bev_conv_train_ref as tref, head_conv_ref

SHARED_SHAPES = ((64, 32), (256, 64), (384, 32), (512, 64))  # (cin, S)
TRUNK_S = (32, 64)
SLICE_PIXELS = 2048  # mssvt_head_conv_train_wgrad_slice_pixels for every covered shape
BIAS_PIECE_ROWS = 2048  # mssvt_head_conv_train_bias_piece_rows
DB_THREADS = 256


def rot_t(w):
    """The weight tensor of the input gradient as a convolution: (cin, S, 3, 3), taps rotated by 180 degrees, axes swapped."""
    return np.ascontiguousarray(np.asarray(w)[:, :, ::-1, ::-1].transpose(1, 0, 2, 3))


def forward(x, w, bias=None):
    """(y, bound)."""
    return head_conv_ref.stage(x, w, bias, None, relu=False)


def dx(dy, w):
    """(dX, bound)."""
    wt = rot_t(w)
    val, a = bev_conv_ref.conv(dy, wt, 1, 1)
    return val, bev_conv_ref.error_bound(a, dy, wt, 3, wt.shape[1])


def dw(x, dy, slice_pixels=SLICE_PIXELS):
    """(dW (S, cin, 3, 3), bound)."""
    return tref.dw_ref(x, dy, 1), tref.dw_bound(x, dy, 1, slice_pixels)


def db_depth(pixels, s, piece_rows=BIAS_PIECE_ROWS):
    g = DB_THREADS // (s // 4)
    pieces = -(-pixels // piece_rows)
    return (-(-min(piece_rows, pixels) // g) - 1) + (g - 1) + (pieces - 1)


def db(dy, piece_rows=BIAS_PIECE_ROWS):
    """(db (S), bound)."""
    d = np.asarray(dy, np.float64).reshape(-1, np.asarray(dy).shape[-1])
    D = max(db_depth(d.shape[0], d.shape[1], piece_rows), 1)
    u = 2.0 ** -24
    with np.errstate(invalid="ignore", over="ignore"):
        return d.sum(0), D * u / (1 - D * u) * np.abs(d).sum(0)


def db_emulated(dy, piece_rows=BIAS_PIECE_ROWS):
    """float32 in the kernel's order."""
    d = np.asarray(dy, np.float32).reshape(-1, np.asarray(dy).shape[-1])
    s = d.shape[1]
    g = DB_THREADS // (s // 4)
    total = None
    for r0 in range(0, d.shape[0], piece_rows):
        piece = d[r0:r0 + piece_rows]
        lanes = np.zeros((g, s), np.float32)
        for r in range(piece.shape[0]):
            lanes[r % g] = lanes[r % g] + piece[r]
        t = lanes[0].copy()
        for j in range(1, g):
            t = t + lanes[j]
        total = t if total is None else total + t
    return total


# ---- the trunk --------------------------------------------------------------------------------------------------------------------
def trunk_forward(y, ws, biases):
    """[(t_b, bound_b)] per branch."""
    return [forward(y, w, b) for w, b in zip(ws, biases)]


def trunk_dy(dts, ws):
    """(dy, bound): the convolution of nb S input channels over the dT_b side by side."""
    dt = np.concatenate([np.asarray(d) for d in dts], axis=3)
    wt = np.concatenate([rot_t(w) for w in ws], axis=1)  # (S, nb S, 3, 3)
    val, a = bev_conv_ref.conv(dt, wt, 1, 1)
    return val, bev_conv_ref.error_bound(a, dt, wt, 3, wt.shape[1])


def trunk_dw(y, dts, slice_pixels=SLICE_PIXELS):
    """[(dW_b, bound_b)]: every branch on its own dT_b."""
    return [dw(y, d, slice_pixels) for d in dts]


def trunk_db(dts, piece_rows=BIAS_PIECE_ROWS):
    return [db(d, piece_rows) for d in dts]


# ---- a float32 emulation of the convolution kernel's order (per output pixel one power of two, a step = 32 input channels) ----
def conv_emulated(xs, ws_t, bias=None):
    """xs: the input tensors (B, H, W, C_i) of ONE accumulation chain (the shared layer / its dX: one; the trunk's dy: the nb
    dT_b), ws_t: per input tensor the (cout, C_i, 3, 3) weights of the convolution that reads it.  Stage order (tap, tensor,
    32-channel step); the products of a step are summed exactly and rounded once into mm (hi hi) and cr (the cross terms)."""
    xs = [np.asarray(x, np.float32) for x in xs]
    B, H, W, _ = xs[0].shape
    cout = ws_t[0].shape[0]
    wmax = max(float(np.abs(np.asarray(w, np.float32)).max()) for w in ws_t)
    wi, wu = tref._pow2(wmax)
    wsplit = [tref._split(np.asarray(w, np.float32) * wi) for w in ws_t]
    e = np.zeros((B, H + 2, W + 2), np.float32)
    e[:, 1:-1, 1:-1] = np.max([np.abs(x).max(axis=3) for x in xs], axis=0)
    out = np.zeros((B, H, W, cout), np.float32)
    for b in range(B):
        for yy in range(H):
            for xx in range(W):
                si, su = tref._pow2(e[b, yy:yy + 3, xx:xx + 3].max())
                mm, cr = np.zeros(cout, np.float32), np.zeros(cout, np.float32)
                for ky in range(3):
                    for kx in range(3):
                        iy, ix = yy + ky - 1, xx + kx - 1
                        inside = 0 <= iy < H and 0 <= ix < W
                        for x, (wh, wl) in zip(xs, wsplit):
                            row = x[b, iy, ix] * si if inside else np.zeros(x.shape[3], np.float32)
                            xh, xl = tref._split(row)
                            for c0 in range(0, x.shape[3], 32):
                                c1 = c0 + 32
                                mm = (mm.astype(np.float64) + wh[:, c0:c1, ky, kx] @ xh[c0:c1]).astype(np.float32)
                                cr = (cr.astype(np.float64) + wh[:, c0:c1, ky, kx] @ xl[c0:c1]
                                      + wl[:, c0:c1, ky, kx] @ xh[c0:c1]).astype(np.float32)
                r = (mm + cr * np.float32(1.0 / 2048)) * (su * wu)
                out[b, yy, xx] = r if bias is None else r + np.asarray(bias, np.float32)
    return out


def weights(s, cin, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((s, cin, 3, 3)) * (2.0 / (9 * cin)) ** 0.5).astype(np.float32)
