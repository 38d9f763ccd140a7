"""float64 numpy statement of the BEV convolution operator (csrc/bev_conv.hip): y = act(scale * conv(x, w) + shift) on
NHWC tensors with the eval-mode BatchNorm fold, plus (|x| conv |w|) per output element (the measure of the operator's
error bound), and a host-side writer / reader of the packed weight blob (include/mssvt_hip.h, mssvt_bev_conv_pack_bytes).
Not a test module: tests/test_bev_conv_ref_cpu.py holds it to torch in float64, the GPU tests hold the kernel to it."""
import numpy as np

HDR_BYTES = 64


def fold(cout, bias=None, bn=None):
    """(scale, shift) float64 of conv bias + BatchNorm2d in eval mode; bn = dict(mean, var, eps, weight or None, bias or None)."""
    scale = np.ones(cout, np.float64)
    shift = np.zeros(cout, np.float64) if bias is None else np.asarray(bias, np.float64).copy()
    if bn is not None:
        g = np.ones(cout) if bn.get("weight") is None else np.asarray(bn["weight"], np.float64)
        b = np.zeros(cout) if bn.get("bias") is None else np.asarray(bn["bias"], np.float64)
        scale = g / np.sqrt(np.asarray(bn["var"], np.float64) + float(bn["eps"]))
        shift = (shift - np.asarray(bn["mean"], np.float64)) * scale + b
    return scale, shift


def out_size(h, ksize, stride, dilation, pad):
    return (h + 2 * pad - dilation * (ksize - 1) - 1) // stride + 1


def conv(x, w, stride=1, dilation=1, pad=None, scale=None, shift=None, relu=False, transposed=False):
    """x (B, H, W, Cin), w (Cout, Cin, k, k) -- or (Cin, Cout, 1, 1) with `transposed` (ConvTranspose2d, k = 1, stride 1).
    Returns (y, a): y (B, Ho, Wo, Cout) float64 = act(scale * conv + shift), a = (|x| conv |w|)."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    if transposed:
        w = w.transpose(1, 0, 2, 3)
    cout, cin, k, _ = w.shape
    pad = (dilation if k == 3 else 0) if pad is None else pad
    B, H, W, _ = x.shape
    ho, wo = out_size(H, k, stride, dilation, pad), out_size(W, k, stride, dilation, pad)
    xp = np.zeros((B, H + 2 * pad, W + 2 * pad, cin))
    xp[:, pad:pad + H, pad:pad + W] = x
    y = np.zeros((B, ho, wo, cout))
    a = np.zeros((B, ho, wo, cout))
    with np.errstate(invalid="ignore", over="ignore"):
        for ky in range(k):
            for kx in range(k):
                xs = xp[:, ky * dilation:ky * dilation + (ho - 1) * stride + 1:stride,
                        kx * dilation:kx * dilation + (wo - 1) * stride + 1:stride]
                y += xs @ w[:, :, ky, kx].T
                a += np.abs(xs) @ np.abs(w[:, :, ky, kx]).T
        if scale is not None:
            y = y * np.asarray(scale, np.float64)
        if shift is not None:
            y = y + np.asarray(shift, np.float64)
        if relu:
            y = np.where(y < 0, 0.0, y)  # a NaN stays a NaN
    return y, a


def steps(ksize, cin):
    """Accumulation steps of the kernel's chain per output element: one per (tap, 32 input channels), + the epilogue's two."""
    return ksize * ksize * cin // 32 + 2


def error_bound(a, x, w, ksize, cin, transposed=False):
    """(3 2^-22 + S 2^-24) (|x| conv |w|) + 2^-24 max|x| sum|w| per output element (the sum over the output channel's weights)."""
    w = np.abs(np.asarray(w, np.float64))
    wsum = w.sum(axis=(0, 2, 3)) if transposed else w.sum(axis=(1, 2, 3))
    return (3 * 2.0 ** -22 + steps(ksize, cin) * 2.0 ** -24) * a + 2.0 ** -24 * np.abs(np.asarray(x, np.float64)).max() * wsum


# ---- the packed blob ----------------------------------------------------------------------------------------------------
def _geometry(ksize, cin, cout):
    kc, ns = min(cin, 128), min(cout, 128)
    return kc, ns, kc // 32, ns // 16, cin // kc, cout // ns


def pack_bytes(ksize, cin, cout):
    return HDR_BYTES + 8 * cout + 4 * ksize * ksize * cin * cout


def _fragment_index(ksize, cin, cout):
    """Index arrays (n, c, tap) of every half of the hi (or lo) images, in blob order."""
    kc, ns, ks, nt, chunks, slices = _geometry(ksize, cin, cout)
    taps = ksize * ksize
    sl, tap, ch, P, t, ln, i = np.meshgrid(np.arange(slices), np.arange(taps), np.arange(chunks), np.arange(ks), np.arange(nt),
                                           np.arange(64), np.arange(8), indexing="ij")
    n = sl * ns + 16 * t + (ln & 15)
    c = ch * kc + 32 * P + 8 * (ln >> 4) + i
    return n, c, tap  # shape (slices, taps, chunks, ks, nt, 64, 8): one block = [.., ks, nt, 64, 8] hi then the same lo


def host_pack(w, scale, shift, transposed=False):
    """The blob mssvt_bev_conv_pack writes for weights w (Cout, Cin, k, k) (or transposed (Cin, Cout, 1, 1)) and an
    already folded float32 scale / shift: uint8 array."""
    w = np.asarray(w, np.float32)
    if transposed:
        w = w.transpose(1, 0, 2, 3)
    cout, cin, k, _ = w.shape
    m = np.abs(w).max()
    e = (np.float32(m).view(np.uint32) & 0x7F800000).astype(np.uint32)
    norm = e != 0 and e < 0x7F000000
    w_in = np.uint32(0x7F000000 - e).view(np.float32) if norm else np.float32(1)
    w_un = np.uint32(e).view(np.float32) if norm else np.float32(1)
    n, c, tap = _fragment_index(k, cin, cout)
    v = (w.reshape(cout, cin, k * k)[n, c, tap] * w_in).astype(np.float32)  # exact: a power of two
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    blocks = np.stack([hi, lo], axis=3)  # (slices, taps, chunks, [hi, lo], ks, nt, 64, 8)
    hdr = np.zeros(16, np.float32)
    hdr[0], hdr[1] = w_in, w_un
    return np.concatenate([hdr.view(np.uint8), np.asarray(scale, np.float32).view(np.uint8),
                           np.asarray(shift, np.float32).view(np.uint8), np.ascontiguousarray(blocks).view(np.uint8).ravel()])


def unpack(blob, ksize, cin, cout):
    """(w (Cout, Cin, k, k) float64 = 2^e (hi + lo / 2048), scale, shift) from a blob."""
    blob = np.ascontiguousarray(np.asarray(blob, np.uint8))
    assert blob.size == pack_bytes(ksize, cin, cout)
    hdr = blob[:HDR_BYTES].view(np.float32)
    scale = blob[HDR_BYTES:HDR_BYTES + 4 * cout].view(np.float32).copy()
    shift = blob[HDR_BYTES + 4 * cout:HDR_BYTES + 8 * cout].view(np.float32).copy()
    assert float(hdr[0]) * float(hdr[1]) == 1.0
    n, c, tap = _fragment_index(ksize, cin, cout)
    kc, ns, ks, nt, chunks, slices = _geometry(ksize, cin, cout)
    halves = blob[HDR_BYTES + 8 * cout:].view(np.float16).reshape(slices, ksize * ksize, chunks, 2, ks, nt, 64, 8)
    val = (halves[:, :, :, 0].astype(np.float64) + halves[:, :, :, 1].astype(np.float64) / 2048.0) * float(hdr[1])
    w = np.full((cout, cin, ksize * ksize), np.nan)
    w[n, c, tap] = val
    assert not np.isnan(w).any()  # every weight has exactly one place
    return w.reshape(cout, cin, ksize, ksize), scale, shift
