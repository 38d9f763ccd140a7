"""tests/segment_sum_ref.py (the references of tests/test_train_rows_gpu.py) pinned on the CPU: ref64 against index_add_,
ordered32 against a per-row loop of numpy.float32 adds, the order check shown able to fail, ordered32 inside `bound`."""
import numpy as np
import torch

from tests import segment_sum_ref as ref


def _case(seed, n_dst=23, n_src=17, C=12, longest=40):
    g = torch.Generator().manual_seed(seed)
    length = torch.randint(0, longest + 1, (n_dst,), generator=g)
    length[0], length[1] = 0, longest
    # not a prefix sum: the ranges lie in permuted order with gaps, and the last two rows overlap
    order = torch.randperm(n_dst, generator=g)
    start = torch.zeros(n_dst, dtype=torch.long)
    at = 3
    for d in order.tolist():
        start[d] = at
        at += int(length[d]) + (d % 2)
    nnz = at + longest + 5
    start[order[-1]] = start[order[-2]] + 1
    end = start + length
    idx = torch.randint(0, n_src, (nnz,), generator=g)
    w = torch.randn(nnz, generator=g)
    src = torch.randn(n_src, C, generator=g) * torch.exp2(torch.randint(-8, 9, (n_src, 1), generator=g).float())
    return start.int(), end.int(), idx.int(), w, src


def test_ref64_matches_index_add_in_float64():
    for seed in range(3):
        start, end, idx, w, src = _case(seed)
        L = ref.lengths(start, end)
        dst_of = torch.repeat_interleave(torch.arange(L.numel()), L)
        e = torch.cat([torch.arange(int(s), int(s) + int(n)) for s, n in zip(start, L)] + [torch.zeros(0, dtype=torch.long)])
        for wt in (w, None):
            rows = src.double()[idx.long()[e]]
            if wt is not None:
                rows = rows * wt.double()[e].unsqueeze(1)
            want = torch.zeros(L.numel(), src.shape[1], dtype=torch.float64).index_add_(0, dst_of, rows)
            want_mag = torch.zeros_like(want).index_add_(0, dst_of, rows.abs())
            got, mag = ref.ref64(start, end, idx, wt, src)
            assert got.dtype == torch.float64 and mag.dtype == torch.float64
            # (index_add_ adds in another order than the loop over list positions: float64 rounding of either)
            assert bool(((got - want).abs() <= 2.0 ** -50 * want_mag).all())
            assert bool(((mag - want_mag).abs() <= 2.0 ** -50 * want_mag).all())
            assert bool((got[L == 0] == 0).all()) and bool((mag[L == 0] == 0).all())


def test_ref64_takes_reversed_and_empty_ranges_as_empty():
    src = torch.arange(8.0).reshape(4, 2)
    start, end = torch.tensor([3, 2, 0, 1]), torch.tensor([1, 2, 4, 3])  # reversed, empty, all, overlapping the third
    idx = torch.tensor([0, 1, 2, 3])
    got, mag = ref.ref64(start, end, idx, torch.tensor([1.0, -1.0, 2.0, 0.5]), src)
    assert got.tolist() == [[0.0, 0.0], [0.0, 0.0], [0 - 2 + 8 + 3, 1 - 3 + 10 + 3.5], [-2 + 8, -3 + 10]]
    assert mag.tolist() == [[0.0, 0.0], [0.0, 0.0], [0 + 2 + 8 + 3, 1 + 3 + 10 + 3.5], [2 + 8, 3 + 10]]
    assert ref.ordered32(start, end, idx, src).tolist() == [[0.0, 0.0], [0.0, 0.0], [12.0, 16.0], [6.0, 8.0]]


def test_ordered32_matches_a_per_row_loop_of_float32_adds():
    for seed in range(3):
        start, end, idx, _, src = _case(10 + seed, longest=70)
        got = ref.ordered32(start, end, idx, src)
        assert got.dtype == torch.float32
        s = src.numpy().astype(np.float32)
        want = np.zeros((start.numel(), s.shape[1]), dtype=np.float32)
        for d in range(start.numel()):
            acc = np.zeros(s.shape[1], dtype=np.float32)
            for e in range(int(start[d]), int(end[d])):
                acc = np.float32(1.0) * s[int(idx[e])] + acc
                assert acc.dtype == np.float32
            want[d] = acc
        assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32))


def test_the_order_check_can_fail():
    """[1e8, -1e8, 1.0] added ascending gives 1.0; descending, the 1.0 is lost in -1e8 and the sum is 0.0.  ([1e8, 1.0, -1e8]
    would not do: it loses the 1.0 in either direction.)"""
    src = torch.tensor([[1e8], [-1e8], [1.0]])
    idx = torch.tensor([0, 1, 2])
    start, end = torch.tensor([0]), torch.tensor([3])
    asc = ref.ordered32(start, end, idx, src)
    desc = ref.ordered32(start, end, torch.flip(idx, [0]), src)
    assert asc.item() == 1.0 and desc.item() == 0.0 and not torch.equal(asc, desc)
    both = ref.ordered32(start, end, torch.tensor([0, 2, 1]), src)
    assert both.item() == 0.0
    total, mag = ref.ref64(start, end, idx, None, src)
    assert total.item() == 1.0 and mag.item() == 2e8 + 1.0
    assert abs(asc.item() - 1.0) <= ref.bound(3, mag).item() and abs(desc.item() - 1.0) <= ref.bound(3, mag).item()


def test_ordered32_stays_inside_the_bound_of_ref64():
    """Lengths 0 .. 256 (one row each), row scales 2^-8 .. 2^8, rows repeated: the float32 chain within (L + 1) 2^-24 mag
    of the float64 sum, and not by a wide margin of the bound's own (it is no loose figure)."""
    g = torch.Generator().manual_seed(7)
    length = torch.arange(0, 257)
    off = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(length, 0)])
    nnz, n_src, C = int(off[-1]), 61, 16
    idx = torch.randint(0, n_src, (nnz,), generator=g)
    src = torch.randn(n_src, C, generator=g) * torch.exp2(torch.randint(-8, 9, (n_src, 1), generator=g).float())
    start, end = off[:-1], off[1:]
    total, mag = ref.ref64(start, end, idx, None, src)
    got = ref.ordered32(start, end, idx, src)
    err = (got.double() - total).abs()
    lim = ref.bound(length, mag)
    assert lim.shape == mag.shape and bool((err <= lim).all())
    assert bool((got[0] == 0).all()) and bool((lim[0] == 0).all())
    assert torch.equal(got[1], src[idx[0]])  # one entry: no rounding at all
    assert float((err[1:] / lim[1:].clamp(min=1e-300)).max()) < 1.0


def test_bound_is_the_stated_formula():
    mag = torch.tensor([[2.0, 4.0], [1.0, 0.0]], dtype=torch.float64)
    assert ref.bound(3, mag).tolist() == [[4 * 2.0 ** -24 * 2, 4 * 2.0 ** -24 * 4], [4 * 2.0 ** -24, 0.0]]
    assert ref.bound(torch.tensor([0, 7]), mag, extra=3).tolist() == [[3 * 2.0 ** -24 * 2, 3 * 2.0 ** -24 * 4],
                                                                     [10 * 2.0 ** -24, 0.0]]
