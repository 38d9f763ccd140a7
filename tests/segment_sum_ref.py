"""Plain references of the training path's segmented row sum (csrc/segment_reduce.hip), CPU, torch only.

    dst[d] = sum_{e in [start[d], end[d])} w[e] * src[idx[e]]          (w optional; ascending e)

Three statements of it:

* ``ref64``: the sum and the sum of absolute values in float64, on arbitrary ranges (overlapping, out of order, empty).
* ``ordered32``: the unweighted sum in float32, added strictly in ascending e from 0.0.  Without weights the kernel's
  ``fmaf(1.0f, v, acc)`` is exactly ``round(v + acc)``, so this function states the kernel's BITS: it pins the ORDER.
* ``bound``: (L + extra) 2^-24 mag, the standard bound of a length-L chain of fused multiply-adds: every step rounds a
  partial sum that is at most mag in absolute value (relative error 2^-24, the products of fp32 factors are exact inside
  the fma), `extra` pays for the second-order terms and for every further rounding of the caller's (an epilogue, an input
  that was itself rounded).  Derived, not measured.
"""
import torch

U32 = 2.0 ** -24  # unit roundoff of float32


def _lists(start, end):
    start, end = start.reshape(-1).long().cpu(), end.reshape(-1).long().cpu()
    length = (end - start).clamp(min=0)
    return start, length, (int(length.max()) if length.numel() else 0)


def lengths(start, end):
    """Entries per destination row (0 for an empty or reversed range), int64."""
    return _lists(start, end)[1]


def ref64(start, end, idx, w, src):
    """(sum, mag) in float64: sum[d] = sum_e w[e] src[idx[e]] over e in [start[d], end[d]), mag the same over absolute
    values.  `w` None = ones.  `src` (n_src, C); the result is (n_dst, C)."""
    start, length, longest = _lists(start, end)
    idx = idx.reshape(-1).long().cpu()
    src = src.detach().cpu().double()
    wd = None if w is None else w.detach().reshape(-1).cpu().double()
    n_dst = start.numel()
    total = torch.zeros((n_dst, src.shape[1]), dtype=torch.float64)
    mag = torch.zeros_like(total)
    for j in range(longest):  # vectorised across rows, one list position at a time
        rows = torch.nonzero(length > j, as_tuple=True)[0]
        e = start[rows] + j
        v = src[idx[e]]
        if wd is not None:
            v = v * wd[e].unsqueeze(1)
        total[rows] += v
        mag[rows] += v.abs()
    return total, mag


def ordered32(start, end, idx, src):
    """The unweighted sum in float32, one IEEE add per entry in ascending e, starting from 0.0."""
    start, length, longest = _lists(start, end)
    idx = idx.reshape(-1).long().cpu()
    src = src.detach().cpu().float()
    acc = torch.zeros((start.numel(), src.shape[1]), dtype=torch.float32)
    for j in range(longest):
        rows = torch.nonzero(length > j, as_tuple=True)[0]
        acc[rows] = acc[rows] + src[idx[start[rows] + j]]  # one rounding per entry: round(v + acc)
    return acc


def bound(L, mag, extra=1):
    """(L + extra) 2^-24 mag, elementwise; L an int or one length per row of `mag`."""
    if torch.is_tensor(L):
        L = L.reshape(-1).double().cpu()
        while L.dim() < mag.dim():
            L = L.unsqueeze(-1)
    return (L + extra) * U32 * mag
