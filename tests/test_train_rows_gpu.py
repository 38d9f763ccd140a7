"""The row kernels every gradient of the backbone flows through, kernel by kernel, against ordered float64 references
(tests/segment_sum_ref.py):

a. k_segment_sum_rows (csrc/segment_reduce.hip): every instantiation x every entry form (_ranges, prefix sum, _strided
   write / accumulate, _residual), the refusals and run-to-run bits;
b. train_path.Segments: the cut of lists longer than CHUNK at its boundaries;
c. mssvt_layer_norm_backward_residual with the residual gradient (csrc/rowops.hip), and the autograd functions on it;
d. the index kernels of csrc/train_tok.hip (interp_compact, query_sets, unique_inverse), bit-exact;
e. _BlockTail and _RepeatRows as autograd nodes.

Every tolerance is `segment_sum_ref.bound` (derived: a chain of L fused multiply-adds) or copied from the existing test
of the same kernel; where the kernel adds without weights its BITS are pinned (`ordered32`), which pins the add order.
All shapes are small; none is the workload's."""
import functools
import math
import types

import pytest
import torch

from mssvt_amd import _lib
from tests import segment_sum_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, BADARG, TOOLARGE = 0, -1, -2
NAN = float("nan")  # prefill of every output: an element the kernel does not write fails every comparison
SENT = -777.25  # prefill of the columns / rows a kernel must leave alone


def _tp():
    from mssvt_amd import train_path
    return train_path


def _inside(got, want, lim, what):
    """|got - want| <= lim elementwise; prints the worst ratio first (the figure to read when it fails)."""
    err = (got.detach().cpu().double() - want).abs()
    ratio = float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print("%s: worst |err| / bound = %.3f" % (what, ratio))
    assert bool((err <= lim).all()), (what, ratio)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _junk():
    """An unrelated allocation between two runs: the second run's buffers land elsewhere."""
    return torch.empty(1 << 18, device=DEV).normal_()


# ---------------------------------------------------------------------------------------------------------
# a. segmented sums: every instantiation x every entry form
# ---------------------------------------------------------------------------------------------------------

WIDTHS = (12, 16, 20, 32, 48, 64, 96, 128, 136, 256, 260, 512)  # LPR 4 / 4 / 8 / 8 / 16 / 16 / 32 / 32 / 64 ...; 260, 512: two passes
LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 15, 16, 17, 24, 25, 255, 256)
N_FULL = 37  # no multiple of 64 / LPR for LPR < 64 (LPR = 64 has one row per wavefront: every count is a multiple)
N_SRC = 50


def _lpr(C):
    q = C // 4
    return 4 if q <= 4 else 8 if q <= 8 else 16 if q <= 16 else 32 if q <= 32 else 64


@functools.lru_cache(maxsize=None)
def _seg_case(C, mode):
    """Inputs and references of one case, built once and left unchanged.  mode "full": one row per length of LENS plus
    random short lists, in shuffled row order; "one": n_dst = 1 (13 entries: the eight-, the four-wide loop and one guarded
    add).  The ranges are no prefix sum: they lie in permuted order with gaps, and two rows overlap."""
    g = torch.Generator().manual_seed(1000 * C + (1 if mode == "one" else 0))
    if mode == "one":
        length = torch.tensor([13])
    else:
        pad = torch.randint(0, 7, (N_FULL - len(LENS),), generator=g)
        length = torch.cat([torch.tensor(LENS), pad])[torch.randperm(N_FULL, generator=g)]
    n_dst = length.numel()
    assert mode == "one" or _lpr(C) == 64 or n_dst % (64 // _lpr(C)) != 0
    start = torch.zeros(n_dst, dtype=torch.long)
    at = 2
    for d in torch.randperm(n_dst, generator=g).tolist():
        start[d] = at
        at += int(length[d]) + d % 3
    nnz = at + 4
    if n_dst > 1:  # a five-entry row inside the tail of the 256-entry row's range
        a, b = int((length == 256).nonzero()[0]), int((length == 5).nonzero()[0])
        start[b] = start[a] + 250
    end = start + length
    assert int(end.max()) <= nnz
    idx = torch.randint(0, N_SRC, (nnz,), generator=g)  # repeats: 50 rows, hundreds of entries
    w = torch.randn(nnz, generator=g)
    src = torch.randn(N_SRC, C, generator=g) * torch.exp2(torch.randint(-8, 9, (N_SRC, 1), generator=g).float())
    res = torch.randn(n_dst, C, generator=g) * torch.exp2(torch.randint(-8, 9, (n_dst, 1), generator=g).float())
    pick = torch.randint(0, 4, (n_dst,), generator=g)
    row_b = torch.where(pick < 3, torch.tensor([0.0, 1.0, 1.0 / 0.7])[pick.clamp(max=2)], torch.randn(n_dst, generator=g))
    if n_dst > 3:
        row_b[:3] = torch.tensor([0.0, 1.0, 1.0 / 0.7])
    row_a = torch.where(torch.randint(0, 2, (n_dst,), generator=g) == 0, torch.ones(n_dst), 1.0 + row_b)
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(length, 0)])  # the prefix-sum form's own lists
    c = types.SimpleNamespace(C=C, n_dst=n_dst, L=length, start=start, end=end, idx=idx, w=w, src=src, res=res, row_a=row_a,
                              row_b=row_b, off=off)
    c.sum_w, c.mag_w = ref.ref64(start, end, idx, w, src)
    c.sum_u, c.mag_u = ref.ref64(start, end, idx, None, src)
    c.ord32 = ref.ordered32(start, end, idx, src)
    c.d = types.SimpleNamespace(start=start.int().to(DEV), end=end.int().to(DEV), idx=idx.int().to(DEV), w=w.to(DEV),
                                src=src.to(DEV), res=res.to(DEV), row_a=row_a.to(DEV), row_b=row_b.to(DEV),
                                off=off.int().to(DEV))
    return c


def _run_ranges(c, weighted, start=None, end=None):
    d = c.d
    dst = torch.full((c.n_dst, c.C), NAN, device=DEV)
    _lib.call("mssvt_segment_sum_rows_ranges", c.C, c.n_dst, _lib.ptr(d.start if start is None else start),
              _lib.ptr(d.end if end is None else end), _lib.ptr(d.idx), _lib.ptr(d.w) if weighted else None, _lib.ptr(d.src),
              _lib.ptr(dst), _lib.stream())
    return dst


def _run_prefix(c, weighted):
    d = c.d
    dst = torch.full((c.n_dst, c.C), NAN, device=DEV)
    _lib.call("mssvt_segment_sum_rows", c.C, c.n_dst, _lib.ptr(d.off), _lib.ptr(d.idx), _lib.ptr(d.w) if weighted else None,
              _lib.ptr(d.src), _lib.ptr(dst), _lib.stream())
    return dst


SRC_PAD, SRC_C0, DST_PAD, DST_C0 = 8, 4, 12, 8  # src rows C + 8 wide, the columns at 4; dst rows C + 12 wide, the columns at 8


def _src_wide(c):
    wide = torch.full((N_SRC, c.C + SRC_PAD), 1e30, device=DEV)  # (a read outside the column range wrecks the sum)
    wide[:, SRC_C0:SRC_C0 + c.C] = c.d.src
    return wide


def _run_strided(c, weighted, dst, accumulate):
    d = c.d
    wide = _src_wide(c)
    _lib.call("mssvt_segment_sum_rows_strided", c.C, c.n_dst, _lib.ptr(d.start), _lib.ptr(d.end), _lib.ptr(d.idx),
              _lib.ptr(d.w) if weighted else None, wide.data_ptr() + 4 * SRC_C0, wide.stride(0), dst.data_ptr() + 4 * DST_C0,
              dst.stride(0), 1 if accumulate else 0, _lib.stream())
    return dst


def _run_residual(c, weighted):
    d = c.d
    dst = torch.full((c.n_dst, c.C), NAN, device=DEV)
    _lib.call("mssvt_segment_sum_rows_residual", c.C, c.n_dst, _lib.ptr(d.start), _lib.ptr(d.end), _lib.ptr(d.idx),
              _lib.ptr(d.w) if weighted else None, _lib.ptr(d.src), _lib.ptr(d.res), _lib.ptr(d.row_a), _lib.ptr(d.row_b),
              _lib.ptr(dst), _lib.stream())
    return dst


seg_cases = pytest.mark.parametrize("C,mode", [(C, m) for C in WIDTHS for m in ("full", "one")])


@seg_cases
def test_segment_sum_ranges_form(C, mode):
    """Weighted: inside bound(L, mag) of the float64 sum.  Unweighted: the bits of the ascending float32 chain -- the add
    ORDER.  Empty ranges: exact zero rows."""
    c = _seg_case(C, mode)
    got = _run_ranges(c, True).cpu()
    _inside(got, c.sum_w, ref.bound(c.L, c.mag_w), "ranges, weighted")
    plain = _run_ranges(c, False).cpu()
    assert torch.equal(plain, c.ord32)
    empty = c.L == 0
    assert torch.equal(_bits(got[empty]), torch.zeros_like(_bits(got[empty])))
    assert torch.equal(_bits(plain[empty]), torch.zeros_like(_bits(plain[empty])))


@seg_cases
def test_segment_sum_prefix_form_is_the_ranges_form(C, mode):
    """mssvt_segment_sum_rows(off) = _ranges(off[:-1], off[1:]) bit for bit, and the unweighted one = the ordered chain."""
    c = _seg_case(C, mode)
    for weighted in (True, False):
        a = _run_prefix(c, weighted)
        b = _run_ranges(c, weighted, c.d.off[:-1], c.d.off[1:])
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(a.cpu(), ref.ordered32(c.off[:-1], c.off[1:], c.idx, c.src))


@seg_cases
def test_segment_sum_strided_form(C, mode):
    """src_stride > C, dst_stride > C, dst a column range of a wider buffer.  Write: the range obeys the bound (its
    unweighted bits the ordered chain's), every other column keeps the sentinel.  Accumulate: fl32(prefill + written) bit
    for bit, an empty range leaves dst bit-unchanged."""
    c = _seg_case(C, mode)
    cols = slice(DST_C0, DST_C0 + C)
    outside = torch.ones(C + DST_PAD, dtype=torch.bool)
    outside[cols] = False
    written = {}
    for weighted in (True, False):
        dst = _run_strided(c, weighted, torch.full((c.n_dst, C + DST_PAD), SENT, device=DEV), False).cpu()
        written[weighted] = dst[:, cols].contiguous()
        assert bool((dst[:, outside] == SENT).all())
    _inside(written[True], c.sum_w, ref.bound(c.L, c.mag_w), "strided write, weighted")
    assert torch.equal(written[False], c.ord32)
    g = torch.Generator().manual_seed(C)
    pre = torch.randn(c.n_dst, C + DST_PAD, generator=g) * 4.0
    for weighted in (True, False):
        dst = _run_strided(c, weighted, pre.to(DEV), True).cpu()
        assert torch.equal(_bits(dst[:, outside]), _bits(pre[:, outside]))
        assert torch.equal(_bits(dst[:, cols]), _bits(pre[:, cols] + written[weighted]))  # one float32 add per element
        empty = c.L == 0
        assert torch.equal(_bits(dst[empty]), _bits(pre[empty]))


@seg_cases
def test_segment_sum_residual_form(C, mode):
    """dst = row_a res + row_b sum inside (L + 3) 2^-24 (|row_b| mag + |row_a res|): the chain, the rounded product
    row_a res, the last fma; a row with an empty range is fl32(row_a res) exactly."""
    c = _seg_case(C, mode)
    ra, rb, res = c.row_a.double().unsqueeze(1), c.row_b.double().unsqueeze(1), c.res.double()
    for weighted, total, mag in ((True, c.sum_w, c.mag_w), (False, c.sum_u, c.mag_u)):
        got = _run_residual(c, weighted).cpu()
        _inside(got, ra * res + rb * total, ref.bound(c.L, rb.abs() * mag + (ra * res).abs(), extra=3),
                "residual, %s" % ("weighted" if weighted else "plain"))
        empty = c.L == 0
        assert torch.equal(got[empty], (c.row_a.unsqueeze(1) * c.res)[empty])


@seg_cases
def test_segment_sum_forms_are_bit_identical_run_to_run(C, mode):
    c = _seg_case(C, mode)
    pre = torch.randn(c.n_dst, C + DST_PAD, generator=torch.Generator().manual_seed(C))
    runs = []
    for _ in range(2):
        out = []
        for weighted in (True, False):
            out += [_run_ranges(c, weighted), _run_prefix(c, weighted), _run_residual(c, weighted),
                    _run_strided(c, weighted, torch.full((c.n_dst, C + DST_PAD), SENT, device=DEV), False),
                    _run_strided(c, weighted, pre.to(DEV), True)]
        runs.append(out)
        keep = _junk()  # alive during the second run
    assert keep.numel()
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))


def test_segment_sum_refusals_leave_dst_untouched():
    """MSSVT_E_BADARG before any launch: C % 4 != 0, a stride that is no multiple of 4 or < C, NULL res / row_a / row_b on
    the residual entry, NULL csr_idx; n_dst = 0 is MSSVT_OK and writes nothing."""
    c = _seg_case(16, "full")
    d, lib, st = c.d, _lib.lib(), _lib.stream()
    dst = torch.full((c.n_dst, 2 * c.C), SENT, device=DEV)  # (room for every stride below)
    wide = torch.full((N_SRC, 2 * c.C), 1.0, device=DEV)
    p = _lib.ptr
    rng = (p(d.start), p(d.end))
    strided = lambda C, ss, ds, acc=0, n=c.n_dst, idx=p(d.idx): lib.mssvt_segment_sum_rows_strided(
        C, n, rng[0], rng[1], idx, p(d.w), p(wide), ss, p(dst), ds, acc, st)
    residual = lambda res, ra, rb, idx=p(d.idx): lib.mssvt_segment_sum_rows_residual(
        c.C, c.n_dst, rng[0], rng[1], idx, p(d.w), p(d.src), res, ra, rb, p(dst), st)
    calls = {
        "C % 4": lambda: strided(10, 32, 32),
        "C % 4, ranges": lambda: lib.mssvt_segment_sum_rows_ranges(14, c.n_dst, rng[0], rng[1], p(d.idx), p(d.w), p(wide), p(dst), st),
        "C % 4, prefix": lambda: lib.mssvt_segment_sum_rows(6, c.n_dst, p(d.off), p(d.idx), p(d.w), p(wide), p(dst), st),
        "src stride % 4": lambda: strided(16, 18, 32),
        "dst stride % 4": lambda: strided(16, 32, 30),
        "src stride < C": lambda: strided(16, 12, 32),
        "dst stride < C": lambda: strided(16, 32, 12, 1),
        "NULL res": lambda: residual(None, p(d.row_a), p(d.row_b)),
        "NULL row_a": lambda: residual(p(d.res), None, p(d.row_b)),
        "NULL row_b": lambda: residual(p(d.res), p(d.row_a), None),
        "NULL csr_idx, residual": lambda: residual(p(d.res), p(d.row_a), p(d.row_b), idx=None),
        "NULL csr_idx, strided": lambda: strided(16, 32, 32, idx=None),
        "NULL csr_idx, ranges": lambda: lib.mssvt_segment_sum_rows_ranges(16, c.n_dst, rng[0], rng[1], None, p(d.w), p(wide), p(dst), st),
        "NULL csr_off": lambda: lib.mssvt_segment_sum_rows(16, c.n_dst, None, p(d.idx), p(d.w), p(wide), p(dst), st),
        "n_dst < 0": lambda: strided(16, 32, 32, n=-1),
    }
    for what, fn in calls.items():
        assert fn() == BADARG, what
        assert bool((dst == SENT).all()), what
    assert strided(16, 32, 32, n=0) == OK and strided(16, 32, 32, acc=1, n=0) == OK
    assert lib.mssvt_segment_sum_rows_residual(c.C, 0, rng[0], rng[1], p(d.idx), p(d.w), p(d.src), p(d.res), p(d.row_a),
                                               p(d.row_b), p(dst), st) == OK
    assert bool((dst == SENT).all())
    assert strided(16, 32, 32) == OK  # the same call with nothing wrong does write
    assert not bool((dst[:, :16] == SENT).any()) and bool((dst[:, 16:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------
# b. Segments: the cut of long lists
# ---------------------------------------------------------------------------------------------------------

CUT_SETS = {
    "256_is_not_cut": [3, 256, 0, 256, 5],
    "257": [2, 257, 4],
    "512": [1, 512, 3],
    "513": [513, 2],
    "three_heavy_first_middle_last": [300, 4, 0, 700, 7, 257],
    "one_row_1000": [1000],  # n_dst = 1: every padding row of the tables lands on row 0
    "total_is_257_k": [257, 257, 257],  # as many long lists as the entry count allows
}


@functools.lru_cache(maxsize=None)
def _cut_case(name):
    counts = torch.tensor(CUT_SETS[name])
    g = torch.Generator().manual_seed(len(name) + int(counts.sum()))
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0)])
    nnz, n_src, C = int(off[-1]), 40, 20
    idx = torch.randint(0, n_src, (nnz,), generator=g)
    w = torch.randn(nnz, generator=g)
    # (row scales 2^-2 .. 2^2 here: the bound of a 513-long list over scales 2^-8 .. 2^8 would swallow one small entry whole,
    # and a lost entry at a chunk's edge is what this section looks for)
    src = torch.randn(n_src, C, generator=g) * torch.exp2(torch.randint(-2, 3, (n_src, 1), generator=g).float())
    c = types.SimpleNamespace(counts=counts, off=off, idx=idx, w=w, src=src, C=C, n_dst=counts.numel())
    c.refs = {True: ref.ref64(off[:-1], off[1:], idx, w, src), False: ref.ref64(off[:-1], off[1:], idx, None, src)}
    # the cut's own order, in bits: every list in chunks of 256 entries, each chunk an ascending chain from 0.0, a row the
    # ascending chain of its chunk sums from 0.0 (a list of one chunk: 0.0 + its sum, exact)
    chunk = 256
    nch = (counts + chunk - 1) // chunk
    row_of = torch.repeat_interleave(torch.arange(counts.numel()), nch)
    p_off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(nch, 0)])
    c_start = off[:-1][row_of] + (torch.arange(int(nch.sum())) - p_off[:-1][row_of]) * chunk
    c_end = torch.minimum(c_start + chunk, off[1:][row_of])
    part = ref.ordered32(c_start, c_end, idx, src)
    c.cut32 = ref.ordered32(p_off[:-1], p_off[1:], torch.arange(part.shape[0]), part)
    c.d = types.SimpleNamespace(off=off.int().to(DEV), idx=idx.int().to(DEV), w=w.to(DEV), src=src.to(DEV))
    return c


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", sorted(CUT_SETS))
def test_segments_cut_at_its_boundaries(name, weighted):
    """Lists of 256 entries are not cut, 257 / 512 / 513 are; heavy first, middle and last rows; n_dst = 1; a total of
    exactly 257 k.  Against float64 with bound(L + ceil(L / 256) + 1, mag) (the chunk sums add one more chain);
    Segments.sum = _sum_into bit for bit; the three ways of supplying `longest` agree in bits and in `heavy is None`."""
    tp = _tp()
    c = _cut_case(name)
    d = c.d
    w = d.w if weighted else None
    longest = int(c.counts.max())
    seg = tp.Segments(d.off, d.idx, w)
    assert (seg.heavy is None) == (longest <= tp.CHUNK) and seg.pending is None
    got = seg.sum(d.src)
    total, mag = c.refs[weighted]
    L = c.counts
    _inside(got, total, ref.bound(L + (L + tp.CHUNK - 1) // tp.CHUNK + 1, mag), "Segments.sum %s" % name)
    assert torch.equal(_bits(got), _bits(seg.sum(d.src)))
    if not weighted:  # the ORDER: chunks of 256 in ascending entries, the chunk sums in chunk order
        assert tp.CHUNK == 256 and torch.equal(got.cpu(), c.cut32)
    # written / added to a column range
    wide = torch.full((c.n_dst, c.C + 8), SENT, device=DEV)
    tp._sum_into(seg, d.src, wide, 4, False)
    assert torch.equal(_bits(wide[:, 4:4 + c.C]), _bits(got))
    assert bool((wide[:, :4] == SENT).all()) and bool((wide[:, 4 + c.C:] == SENT).all())
    pre = torch.randn(c.n_dst, c.C + 8, generator=torch.Generator().manual_seed(1)).to(DEV)
    acc = pre.clone()
    tp._sum_into(seg, d.src, acc, 4, True)
    assert torch.equal(_bits(acc[:, 4:4 + c.C]), _bits(pre[:, 4:4 + c.C] + got))  # one add per element either way
    assert torch.equal(_bits(acc[:, :4]), _bits(pre[:, :4])) and torch.equal(_bits(acc[:, 4 + c.C:]), _bits(pre[:, 4 + c.C:]))
    # `longest` as an int, as the device word read with the next sizes, and as the device word read on first use
    word = lambda: torch.tensor([longest if longest > tp.CHUNK else 0], dtype=torch.int32, device=DEV)  # what mssvt_csr_transpose leaves
    by_int = tp.Segments(d.off, d.idx, w, longest=longest)
    by_word = tp.Segments(d.off, d.idx, w, longest=word())
    assert by_word.pending is not None and by_word.heavy is None
    tp._deferred.append(by_word)
    assert tp._read_sizes(torch.tensor([5, 9], dtype=torch.int32, device=DEV)) == [5, 9]
    assert by_word.pending is None and not tp._deferred
    on_use = tp.Segments(d.off, d.idx, w, longest=word())
    for other in (by_int, by_word, on_use):
        assert torch.equal(_bits(other.sum(d.src)), _bits(got))
        assert other.pending is None and (other.heavy is None) == (seg.heavy is None)


def test_segments_of_an_empty_index_set_give_zeros():
    tp = _tp()
    off = torch.zeros(8, dtype=torch.int32, device=DEV)
    none = torch.zeros(0, dtype=torch.int32, device=DEV)
    src = torch.randn(3, 20, device=DEV)
    # (the last: the inverse of a gather of zero distinct rows -- one index per destination, every range empty, NO source row)
    for seg in (tp.Segments(off, none, None), tp.Segments(off, none, None, longest=1), tp.Segments(off, None, None, longest=1),
                tp._gather_unique(none, 7).bwd):
        if seg.idx is not None and seg.idx.numel():
            src = src[:0]
        got = seg.sum(src)
        assert got.shape == (7, 20) and got.dtype == torch.float32 and bool((got == 0).all())
        wide = torch.full((7, 28), SENT, device=DEV)
        tp._sum_into(seg, src, wide, 4, True)
        assert bool((wide == SENT).all())
        tp._sum_into(seg, src, wide, 4, False)
        assert bool((wide[:, 4:24] == 0).all()) and bool((wide[:, :4] == SENT).all()) and bool((wide[:, 24:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------
# c. LayerNorm backward with the residual gradient
# ---------------------------------------------------------------------------------------------------------

def _ln_backward(x, dy, dres, w, eps, plain=False):
    N, C = x.shape
    dx = torch.full((max(N, 1), C), NAN, device=DEV)[:N]
    dw, db = torch.full((C,), NAN, device=DEV), torch.full((C,), NAN, device=DEV)
    ws = torch.empty((512 * 2 * 256,), dtype=torch.float32, device=DEV)
    if plain:
        _lib.call("mssvt_layer_norm_backward", _lib.ptr(x), _lib.ptr(dy), N, C, _lib.ptr(w), eps, _lib.ptr(dx), _lib.ptr(dw),
                  _lib.ptr(db), _lib.ptr(ws), _lib.stream())
    else:
        _lib.call("mssvt_layer_norm_backward_residual", _lib.ptr(x), _lib.ptr(dy), _lib.ptr(dres), N, C, _lib.ptr(w), eps,
                  _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), _lib.stream())
    return dx, dw, db


def _ln_tol(ref_t, N):
    """The project's own tolerance of this kernel (test_train_path_gpu.py::test_layer_norm_backward_kernel)."""
    return 3e-6 * max(1.0, float(ref_t.abs().max())) * max(1.0, N ** 0.5 / 16)


LN_ROWS = ("1", "rpi-1", "rpi", "rpi+1", "512rpi", "512rpi+1")


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("C", [16, 32, 64, 128, 256])
def test_layer_norm_backward_with_the_residual_gradient(C, rows):
    """mssvt_layer_norm_backward_residual with dres against float64 autograd of (LN(x) dy).sum() + (x dres).sum(), at the
    row counts where the launch changes: one row, around one workgroup instruction (rpi rows), 512 rpi (the last count with
    rpi rows per workgroup) and 512 rpi + 1 (2 rpi rows per workgroup, a ragged last one)."""
    rpi = 4 * 64 // (C // 4)
    N = {"1": 1, "rpi-1": rpi - 1, "rpi": rpi, "rpi+1": rpi + 1, "512rpi": 512 * rpi, "512rpi+1": 512 * rpi + 1}[rows]
    g = torch.Generator().manual_seed(N + C)
    x0 = torch.randn(N, C, generator=g) * 2 + 0.3
    dy0, dres0 = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)
    w0, eps = torch.rand(C, generator=g) + 0.5, 1e-5
    x, dy, dres, w = x0.to(DEV), dy0.to(DEV), dres0.to(DEV), w0.to(DEV)
    got = _ln_backward(x, dy, dres, w, eps)
    xd, wd, bd = x0.double().requires_grad_(True), w0.double().requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    ((torch.nn.functional.layer_norm(xd, (C,), wd, bd, eps) * dy0.double()).sum() + (xd * dres0.double()).sum()).backward()
    for t, want, what in zip(got, (xd.grad, wd.grad, bd.grad), ("dx", "dweight", "dbias")):
        err = float((t.cpu().double() - want).abs().max())
        print("%s: err %.3e of %.3e" % (what, err, _ln_tol(want, N)))
        assert err <= _ln_tol(want, N), (what, err)
    keep = _junk()
    again = _ln_backward(x, dy, dres, w, eps)
    none = _ln_backward(x, dy, None, w, eps)
    plain = _ln_backward(x, dy, None, w, eps, plain=True)
    assert keep.numel()
    for a, b in zip(got, again):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(_bits(got[1]), _bits(none[1])) and torch.equal(_bits(got[2]), _bits(none[2]))  # dres touches dx only
    for a, b in zip(none, plain):
        assert torch.equal(_bits(a), _bits(b))
    # without dres: the LayerNorm's own gradient (so dres is what separates the two dx: it is added, not dropped)
    xd.grad = None
    (torch.nn.functional.layer_norm(xd, (C,), wd, bd, eps) * dy0.double()).sum().backward()
    assert float((none[0].cpu().double() - xd.grad).abs().max()) <= _ln_tol(xd.grad, N)


def test_layer_norm_backward_refuses_other_widths_and_zeroes_on_no_rows():
    lib, st, p = _lib.lib(), _lib.stream(), _lib.ptr
    x, dy, dres = (torch.randn(8, 48, device=DEV) for _ in range(3))
    w = torch.ones(48, device=DEV)
    dx, dw, db = (torch.full(s, SENT, device=DEV) for s in ((8, 48), (48,), (48,)))
    ws = torch.empty((512 * 2 * 256,), dtype=torch.float32, device=DEV)
    assert lib.mssvt_layer_norm_backward_residual(p(x), p(dy), p(dres), 8, 48, p(w), 1e-5, p(dx), p(dw), p(db), p(ws), st) == TOOLARGE
    assert all(bool((t == SENT).all()) for t in (dx, dw, db))
    for C in (16, 256):
        dw, db = torch.full((C,), SENT, device=DEV), torch.full((C,), SENT, device=DEV)
        dx = torch.full((1, C), SENT, device=DEV)
        x, w = torch.randn(1, C, device=DEV), torch.ones(C, device=DEV)
        assert lib.mssvt_layer_norm_backward_residual(p(x), p(x), p(x), 0, C, p(w), 1e-5, p(dx), p(dw), p(db), p(ws), st) == OK
        assert bool((dw == 0).all()) and bool((db == 0).all()) and bool((dx == SENT).all())


class _FfnBlock(torch.nn.Module):
    """What train_path.ffn_residual reads of a Block."""

    def __init__(self, C):
        super().__init__()
        self.norm2 = torch.nn.LayerNorm(C)
        self.linear1, self.linear2 = torch.nn.Linear(C, 2 * C), torch.nn.Linear(2 * C, C)
        self.activation, self.dropout1 = torch.nn.ReLU(), torch.nn.Identity()


def test_layer_norm_residual_node_against_float64():
    """layer_norm_residual(norm, x) used as (x_ret a).sum() + (y b).sum(): x's two uses meet inside the backward kernel."""
    tp = _tp()
    N, C = 301, 64
    g = torch.Generator().manual_seed(11)
    norm = torch.nn.LayerNorm(C)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(C, generator=g) + 0.5)
        norm.bias.copy_(torch.randn(C, generator=g))
    x0, a, b = (torch.randn(N, C, generator=g) * s for s in (2.0, 1.0, 1.0))
    norm64 = torch.nn.LayerNorm(C).double()
    norm64.load_state_dict(norm.state_dict())
    xd = x0.double().requires_grad_(True)
    yd = norm64(xd)
    ((xd * a.double()).sum() + (yd * b.double()).sum()).backward()
    norm = norm.to(DEV)
    runs = []
    for _ in range(2):
        norm.zero_grad(set_to_none=True)
        x = x0.to(DEV).requires_grad_(True)
        x_ret, y = tp.layer_norm_residual(norm, x)
        assert "_LayerNorm" in type(y.grad_fn).__name__ and torch.equal(x_ret.detach(), x.detach())
        ((x_ret * a.to(DEV)).sum() + (y * b.to(DEV)).sum()).backward()
        runs.append((y.detach(), x.grad.clone(), norm.weight.grad.clone(), norm.bias.grad.clone()))
    for t, u in zip(*runs):
        assert torch.equal(_bits(t), _bits(u))
    for t, want, what in zip(runs[0], (yd.detach(), xd.grad, norm64.weight.grad, norm64.bias.grad), ("y", "dx", "dweight", "dbias")):
        err = float((t.cpu().double() - want).abs().max())
        assert err <= _ln_tol(want, N), (what, err)


def test_ffn_residual_against_float64():
    """ffn_residual(block, x) = (x, linear2(relu(linear1(norm2(x))))) used as (x_ret a).sum() + (z b).sum(): values, input
    gradient, every parameter gradient.  Tolerances: those of the package-level checks of train_path.linear in
    test_train_path_gpu.py (1e-4 scale for values and input gradients, 2e-4 max(1, sqrt(M) / 16) scale for parameter
    gradients); LayerNorm's own parameters at the LayerNorm kernel's."""
    tp = _tp()
    M, C = 300, 128
    torch.manual_seed(5)
    blk = _FfnBlock(C)
    g = torch.Generator().manual_seed(12)
    x0, a = torch.randn(M, C, generator=g) * 2.0, torch.randn(M, C, generator=g)
    b = torch.randn(M, C, generator=g)
    blk64 = _FfnBlock(C).double()
    blk64.load_state_dict(blk.state_dict())
    xd = x0.double().requires_grad_(True)
    zd = blk64.linear2(blk64.activation(blk64.linear1(blk64.norm2(xd))))
    ((xd * a.double()).sum() + (zd * b.double()).sum()).backward()
    blk = blk.to(DEV)
    x = x0.to(DEV).requires_grad_(True)
    x_ret, z = tp.ffn_residual(blk, x)
    assert torch.equal(x_ret.detach(), x.detach())
    ((x_ret * a.to(DEV)).sum() + (z * b.to(DEV)).sum()).backward()
    scale = lambda t: max(1.0, float(t.abs().max()))
    assert float((z.detach().cpu().double() - zd.detach()).abs().max()) <= 1e-4 * scale(zd.detach())
    assert float((x.grad.cpu().double() - xd.grad).abs().max()) <= 1e-4 * scale(xd.grad)
    want = dict(blk64.named_parameters())
    for name, prm in blk.named_parameters():
        err, wg = float((prm.grad.cpu().double() - want[name].grad).abs().max()), want[name].grad
        tol = 2e-4 * max(1.0, M ** 0.5 / 16) * scale(wg)
        print("%s: err %.3e of %.3e" % (name, err, tol))
        assert err <= tol, (name, err)


def test_add_drop_path_with_an_active_drop_path():
    """x + drop_path(z) in one launch, rate 0.3 in training mode: against x + z mask with the module's own mask under the
    same seed -- two roundings at most (the product, the add); dx = g exactly, dz = g mask (one rounding)."""
    tp = _tp()
    from mssvt_amd.mssvt_backbone import DropPath
    blk = types.SimpleNamespace(drop_path=DropPath(0.3).train())
    N, C = 257, 32
    g = torch.Generator().manual_seed(13)
    x = torch.randn(N, C, generator=g).to(DEV).requires_grad_(True)
    z = torch.randn(N, C, generator=g).to(DEV).requires_grad_(True)
    gr = torch.randn(N, C, generator=g).to(DEV)
    torch.manual_seed(77)
    out = tp.add_drop_path(blk, x, z)
    out.backward(gr)
    torch.manual_seed(77)
    mask = torch.empty((N, 1), device=DEV).bernoulli_(0.7).div_(0.7)
    kept = int((mask > 0).sum())
    assert 0 < kept < N and bool(((mask == 0) | ((mask - 1.0 / 0.7).abs() <= 2e-7)).all())
    xd, zd, md = x.detach().double(), z.detach().double(), mask.double()
    err = (out.detach().double() - (xd + zd * md)).abs()
    assert bool((err <= 2 * ref.U32 * (xd.abs() + (zd * md).abs())).all())
    assert torch.equal(out.detach()[mask[:, 0] == 0], x.detach()[mask[:, 0] == 0])  # a dropped row is x
    assert torch.equal(x.grad, gr) and torch.equal(z.grad, gr * mask)
    blk.drop_path.eval()
    assert torch.equal(tp.add_drop_path(blk, x, z).detach(), (x + z).detach())


# ---------------------------------------------------------------------------------------------------------
# d. index kernels (csrc/train_tok.hip): bit-exact against the torch statement
# ---------------------------------------------------------------------------------------------------------

SIZES = (0, 1, 255, 256, 257, 1000)


@pytest.mark.parametrize("N", SIZES)
def test_train_interp_compact(N):
    """idx3 / w3 / owned of owned and untouched voxels (.x < 0 with garbage in .y / .z / .w and in the weights); `inv`
    sends some padded rows to R; nothing is written past N."""
    g = torch.Generator().manual_seed(N)
    R, P = 37, 500  # compact rows, padded rows (row P = the zero row)
    inv = torch.randint(0, R, (P + 1,), generator=g)
    inv[torch.rand(P + 1, generator=g) < 0.3] = R
    inv[P] = R
    rows = max(N, 1)
    tab = torch.randint(0, P + 1, (rows, 4), generator=g)
    tab[:, 3] = torch.randint(-1000, P + 1, (rows,), generator=g)
    un = torch.rand(rows, generator=g) < 0.4
    if N > 2:
        un[0], un[1] = True, False
    # untouched: .x any negative, the rest garbage (negative or a stale row)
    tab[un] = torch.randint(-1000, P + 1, (int(un.sum()), 4), generator=g)
    tab[un, 0] = torch.randint(-1000, 0, (int(un.sum()),), generator=g)
    tw = torch.rand(rows, 4, generator=g) + 0.01
    tw[un] = torch.randn(int(un.sum()), 4, generator=g) * 1e6
    idx3 = torch.full((3 * N + 6,), -5, dtype=torch.int32, device=DEV)
    w3 = torch.full((3 * N + 6,), SENT, device=DEV)
    owned = torch.full((N + 16,), 0xAB, dtype=torch.uint8, device=DEV)
    inv_d, tab_d, tw_d = inv.int().to(DEV), tab.int().to(DEV), tw.to(DEV)
    _lib.call("mssvt_train_interp_compact", N, R, _lib.ptr(inv_d), _lib.ptr(tab_d), _lib.ptr(tw_d), _lib.ptr(idx3), _lib.ptr(w3),
              _lib.ptr(owned), _lib.stream())
    own = ~un[:N]
    want_idx = torch.where(own.unsqueeze(1), inv[tab[:N, :3].clamp(min=0)], torch.full((N, 3), R))
    want_w = torch.where(own.unsqueeze(1), tw[:N, :3], torch.zeros(N, 3))
    assert torch.equal(idx3.cpu()[:3 * N].long(), want_idx.reshape(-1))
    assert torch.equal(_bits(w3.cpu()[:3 * N]), _bits(want_w.reshape(-1)))
    assert torch.equal(owned.cpu()[:N], own.to(torch.uint8))
    assert bool((owned[N:] == 0xAB).all()) and bool((idx3[3 * N:] == -5).all()) and bool((w3[3 * N:] == SENT).all())
    if N > 2:
        assert want_idx[0].tolist() == [R, R, R] and want_w[0].tolist() == [0.0, 0.0, 0.0] and int(owned[0]) == 0
        assert bool((want_idx[own] == R).any()) and bool((want_idx[own] < R).any())  # both kinds of owned entries occur


@pytest.mark.parametrize("R", SIZES)
def test_train_query_sets(R):
    """q_rows = the int bits of row_meta[:, 3] (a row index whose float bits are a NaN pattern included), q_geo8 = [offset
    xyz, wcentre[row_src[:, 0]] xyz, 0, 0]; rows >= R of the outputs are untouched."""
    g = torch.Generator().manual_seed(R + 1)
    rows, nw = R + 5, 23
    meta = torch.randn(rows, 4, generator=g)
    vox = torch.randint(0, 1 << 20, (rows,), generator=g).int()
    if R:
        vox[R - 1] = 0x7FC00001  # a quiet NaN's bits
        vox[0] = 0x7F800001 if R > 1 else vox[0]  # a signalling NaN's
    meta.view(torch.int32)[:, 3] = vox
    row_src = torch.stack([torch.randint(0, nw, (rows,), generator=g), torch.randint(0, 1 << 20, (rows,), generator=g)], 1).int()
    wc = torch.randn(nw, 4, generator=g)
    q_rows = torch.full((rows,), -5, dtype=torch.int32, device=DEV)
    q_geo = torch.full((rows, 8), SENT, device=DEV)
    meta_d, row_src_d, wc_d = meta.to(DEV), row_src.to(DEV), wc.to(DEV)
    _lib.call("mssvt_train_query_sets", R, _lib.ptr(meta_d), _lib.ptr(row_src_d), _lib.ptr(wc_d), _lib.ptr(q_rows), _lib.ptr(q_geo),
              _lib.stream())
    want = torch.cat([meta[:R, :3], wc[row_src[:R, 0].long(), :3], torch.zeros(R, 2)], 1)
    assert torch.equal(q_rows.cpu()[:R], vox[:R])
    assert torch.equal(_bits(q_geo.cpu()[:R]), _bits(want))
    assert bool((q_rows[R:] == -5).all()) and bool((q_geo[R:] == SENT).all())


def _partial_permutation(n_src, nnz, name_row0, seed):
    """`nnz` distinct rows of n_src in random order (fewer where n_src has no more), with or without source row 0."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n_src, generator=g)
    if not name_row0:
        return perm[perm != 0][:nnz]
    perm = perm[:nnz]
    if nnz and not bool((perm == 0).any()):
        perm[int(torch.randint(0, nnz, (1,), generator=g))] = 0
    return perm


UNIQUE_CASES = [(n, int(0.6 * n), r0) for n in SIZES[1:] for r0 in (False, True)] + [(300, 0, False), (0, 0, False), (64, 64, True), (2, 1, True)]


@pytest.mark.parametrize("n_src,nnz,name_row0", UNIQUE_CASES)
def test_train_unique_inverse(n_src, nnz, name_row0):
    """bwd_end[v] - v = 1 exactly where an entry reads source row v, and there idx[bwd_idx[v]] = v -- entry 0 and source
    row 0 included ("entry 0 reads me" is not "nothing reads me"); bwd_idx stays a valid entry everywhere."""
    nnz = min(nnz, max(n_src - (0 if name_row0 else 1), 0))
    idx = _partial_permutation(n_src, nnz, name_row0, n_src + nnz)
    nnz = idx.numel()
    assert (nnz > 0 and bool((idx == 0).any())) == (name_row0 and nnz > 0)
    inv = torch.full((n_src + 3,), -7, dtype=torch.int32, device=DEV)
    bwd_idx = torch.full((n_src + 3,), -5, dtype=torch.int32, device=DEV)
    bwd_end = torch.full((n_src + 3,), -5, dtype=torch.int32, device=DEV)
    idx_d = idx.int().to(DEV)
    _lib.call("mssvt_train_unique_inverse", nnz, n_src, _lib.ptr(idx_d) if nnz else None, _lib.ptr(inv), _lib.ptr(bwd_idx),
              _lib.ptr(bwd_end), _lib.stream())
    want_inv = torch.full((n_src,), -1, dtype=torch.long)
    want_inv[idx] = torch.arange(nnz)
    read = want_inv >= 0
    got_idx, got_end = bwd_idx.cpu()[:n_src].long(), bwd_end.cpu()[:n_src].long()
    assert torch.equal(got_end - torch.arange(n_src), read.long())
    assert torch.equal(got_idx[read], want_inv[read])
    assert torch.equal(idx[got_idx[read]], torch.arange(n_src)[read])
    assert bool((got_idx >= 0).all()) and bool((got_idx < max(nnz, 1)).all())
    if nnz:  # the row entry 0 names sums entry 0 -- and is told apart from the rows nothing names, whose index is 0 too
        v0 = int(idx[0])
        assert int(got_idx[v0]) == 0 and int(got_end[v0]) == v0 + 1
        assert bool((got_end[~read] == torch.arange(n_src)[~read]).all())
    assert bool((bwd_idx[n_src:] == -5).all()) and bool((bwd_end[n_src:] == -5).all()) and bool((inv[n_src:] == -7).all())


@pytest.mark.parametrize("n_src,nnz,name_row0", [c for c in UNIQUE_CASES if c[0] > 0])
def test_gather_unique_is_the_sorted_gather(n_src, nnz, name_row0):
    """_gather_unique(idx, n) against Csr.gather(idx, n): gather_sum forward and backward bit-identical, and both equal to
    float64 index_select / index_add_ (exact: one term per row)."""
    tp = _tp()
    nnz = min(nnz, max(n_src - (0 if name_row0 else 1), 0))
    idx = _partial_permutation(n_src, nnz, name_row0, n_src + nnz)
    nnz, C = idx.numel(), 20
    g = torch.Generator().manual_seed(3)
    src0, gr = torch.randn(n_src, C, generator=g), torch.randn(nnz, C, generator=g)
    idx_d = idx.int().to(DEV)
    out = []
    for csr in (tp._gather_unique(idx_d, n_src), tp.Csr.gather(idx_d, n_src)):
        src = src0.to(DEV).requires_grad_(True)
        y = tp.gather_sum(src, csr)
        y.backward(gr.to(DEV))
        out.append((y.detach().cpu(), src.grad.cpu()))
    assert torch.equal(_bits(out[0][0]), _bits(out[1][0])) and torch.equal(_bits(out[0][1]), _bits(out[1][1]))
    assert out[0][0].shape == (nnz, C) and out[0][1].shape == (n_src, C)
    assert torch.equal(out[0][0].double(), src0.double().index_select(0, idx))
    assert torch.equal(out[0][1].double(), torch.zeros(n_src, C, dtype=torch.float64).index_add_(0, idx, gr.double()))


# ---------------------------------------------------------------------------------------------------------
# e. _BlockTail and _RepeatRows as autograd nodes
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [16, 64, 128, 256])
def test_block_tail_node_against_float64(C):
    """new = row_a x_in + row_b sum_e w_e attn[idx_e] on a hand-built 3-entries-per-voxel table with owned and untouched
    voxels and dropped rows (row_b = 0).  Forward: the residual bound.  d x_in = g row_a: one product, exact.  d attn: the
    inverted lists' sums of the rounded rows g row_b -- bound(L, mag) against float64 on those rows, bound(L, mag, 2) against
    float64 autograd (one more rounding: the product g row_b); the zero row R gets no gradient."""
    tp = _tp()
    N, R = 301, 60
    g = torch.Generator().manual_seed(C)
    un = torch.rand(N, generator=g) < 0.3
    un[0], un[1] = True, False
    idx3 = torch.randint(0, R + 1, (N, 3), generator=g)  # (an owned voxel's empty slot names the zero row R, too)
    w3 = torch.rand(N, 3, generator=g)
    idx3[un], w3[un] = R, 0.0
    row_b = torch.where(torch.rand(N, generator=g) < 0.3, torch.zeros(N), torch.full((N,), 1.0 / 0.7))
    row_b[2], row_b[3] = 0.0, 1.0 / 0.7
    row_a = torch.where(un, row_b + 1.0, torch.ones(N))
    attn0 = torch.randn(R + 1, C, generator=g) * torch.exp2(torch.randint(-4, 5, (R + 1, 1), generator=g).float())
    attn0[R] = 0.0
    x0, gr = torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)
    off3 = torch.arange(0, 3 * N + 1, 3, dtype=torch.int32)
    csr = tp.Csr(off3.to(DEV), idx3.reshape(-1).int().to(DEV), w3.reshape(-1).to(DEV), R + 1, drop_src=R, fwd_longest=3)
    runs = []
    for _ in range(2):
        attn, x = attn0.to(DEV).requires_grad_(True), x0.to(DEV).requires_grad_(True)
        new = tp._BlockTail.apply(attn, x, csr, row_a.to(DEV), row_b.to(DEV))
        new.backward(gr.to(DEV))
        runs.append((new.detach().cpu(), attn.grad.cpu(), x.grad.cpu()))
        keep = _junk()
    assert keep.numel()
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))
    new, d_attn, d_x = runs[0]
    # forward
    flat_idx, flat_w = idx3.reshape(-1), w3.reshape(-1)
    total, mag = ref.ref64(off3[:-1], off3[1:], flat_idx, flat_w, attn0)
    ra, rb = row_a.double().unsqueeze(1), row_b.double().unsqueeze(1)
    _inside(new, ra * x0.double() + rb * total, ref.bound(3, rb.abs() * mag + (ra * x0.double()).abs(), extra=3), "tail forward")
    assert torch.equal(new[un], ((row_b[un] + 1.0).unsqueeze(1) * x0[un]))  # an untouched voxel: (1 + row_b) x_in
    # backward
    assert torch.equal(d_x, gr * row_a.unsqueeze(1))
    assert torch.equal(_bits(d_attn[R]), torch.zeros(C, dtype=torch.int32))
    keep_e = torch.nonzero(flat_idx != R, as_tuple=True)[0]
    e_sorted = keep_e[torch.sort(flat_idx[keep_e], stable=True).indices]  # per compact row its entries, ascending
    t_off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(torch.bincount(flat_idx[keep_e], minlength=R), 0)])
    L = t_off[1:] - t_off[:-1]
    assert int(L.max()) > 8 and int(L.min()) < 8  # both loops of the kernel
    rows32 = gr * row_b.unsqueeze(1)  # what the node hands to the segmented sum
    total, mag = ref.ref64(t_off[:-1], t_off[1:], e_sorted // 3, flat_w[e_sorted], rows32)
    _inside(d_attn[:R], total, ref.bound(L, mag), "tail d_attn against its rounded rows")
    ad, xd = attn0.double().requires_grad_(True), x0.double().requires_grad_(True)
    gathered = (ad[idx3.reshape(-1)] * flat_w.double().unsqueeze(1)).reshape(N, 3, C).sum(1)
    (ra * xd + rb * gathered).backward(gr.double())
    assert torch.equal(d_x, xd.grad.float())  # (the float64 product of two float32 factors is exact: one rounding)
    _inside(d_attn[:R], ad.grad[:R], ref.bound(L, mag, extra=2), "tail d_attn against float64 autograd")


def test_repeat_rows_node():
    """repeat_rows = repeat_interleave (lengths with zeros and a 300-long run); its gradient a segmented sum per row,
    against float64 inside bound(L, mag) (any order of L - 1 adds obeys it); twice: the same bits."""
    tp = _tp()
    g = torch.Generator().manual_seed(21)
    lengths = torch.tensor([0, 3, 300, 0, 1, 17, 256, 2, 0])
    total, C = int(lengths.sum()), 24
    x0, gr = torch.randn(lengths.numel(), C, generator=g), torch.randn(total, C, generator=g) * 3.0
    runs = []
    for _ in range(2):
        x = x0.to(DEV).requires_grad_(True)
        y = tp.repeat_rows(x, lengths.to(DEV), total)
        y.backward(gr.to(DEV))
        runs.append((y.detach().cpu(), x.grad.cpu()))
        keep = _junk()
    assert keep.numel()
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(_bits(runs[0][1]), _bits(runs[1][1]))
    assert torch.equal(runs[0][0], torch.repeat_interleave(x0, lengths, dim=0))
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(lengths, 0)])
    want, mag = ref.ref64(off[:-1], off[1:], torch.arange(total), None, gr)
    _inside(runs[0][1], want, ref.bound(lengths, mag), "repeat_rows backward")
    assert bool((runs[0][1][lengths == 0] == 0).all())
