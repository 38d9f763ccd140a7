"""k_attn_kvh (csrc/block_attn.hip) where its pass bodies and its prologue switch: windows whose live keys all sit in the
first half of the key list take another pass body than their neighbours, and the first windows of a wave are fetched
during the weight staging, as soon as the wave knows how many windows there are.

Case builder, float64 reference, device harness and the kv16 tolerance (|got - ref| <= 1e-5 max|ref| + 1e-4 |ref|) are those
of tests/test_block_attn_gpu.py; only the window structure is chosen here: N = 500 feature rows, two head groups of
Cg = 64, head_dim 16.

  1. one launch mixing the classes: the live key slots cycle through slot 0 only / 0-14 / 0-15 (exactly one tile) / 0-16
     (first key of tile 1) / 0 and K-1 only / all / tile 0 with holes (K = 64: also tiles 0 and 1 only, tiles 0 and 3 only,
     tiles 0 and 2 only, first key of tile 2), nq_valid through 0, 1, 4, 5, nq = 6 (one and two passes), four windows per
     wave of the grid: a wave steps between the bodies while the next window's tile mask is already in its registers;
  2. position independence, bit for bit: 40 windows alone and embedded at three offsets among 3200 others;
  3. prologue edges: 0, 1, exactly as many and one more active windows than the launch has waves, with the work order
     allocated at exactly its capacity.
"""
import pytest
import torch

from tests import test_block_attn_gpu as ba

pytestmark = pytest.mark.gpu

GROUPS = [(0, 64, 4), (64, 64, 4)]
NQ = 6
NQV_CYCLE = (0, 1, 4, 5, NQ)
HOLES = (0, 2, 3, 5, 8, 13)  # tile 0 with masked slots between live ones


def key_classes(K):
    r = lambda a, b: tuple(range(a, b))  # noqa: E731
    cls = [(0,), r(0, 15), r(0, 16), r(0, 17), (0, K - 1), r(0, K), HOLES]
    if K == 64:
        # tiles 0 and 1 only, tiles 0 and 3 only, first key of tile 2, tiles 0 and 2 only (11 classes: coprime with the 5 counts)
        cls += [r(0, 32), r(0, 16) + r(48, 64), r(0, 33), r(0, 16) + r(32, 48)]
    return cls


def waves(K, form):
    """Wavefronts per head group of the window launch (launch_block_attn): resident workgroups per CU x 4 waves."""
    del form  # with and without blobs: three resident workgroups per CU at K <= 32, two above
    return (ba._cus() * (2 if K > 32 else 3) // len(GROUPS)) * 4


def build_base(K, nw):
    """nw windows: key class (w + 3 g) mod #classes in group g, nq_valid = NQV_CYCLE[w mod 5] in the first slots."""
    c = ba.make_case(128, GROUPS, 16, NQ, K, nw, N=500, seed=4000 + K, keys="all", queries="all", cap=nw)
    cls = key_classes(K)
    for gi, km in enumerate(c.kmeta):
        live = torch.zeros(c.cap, K, dtype=torch.bool)
        for i, slots in enumerate(cls):
            w = torch.arange((i - 3 * gi) % len(cls), c.cap, len(cls))
            live[w[:, None], torch.tensor(slots)[None, :]] = True
        assert bool(live[:, 0].all())
        rows = km.view(torch.int32)[..., 3]
        rows[~live] = -1
    counts = torch.tensor(NQV_CYCLE, dtype=torch.int32)[torch.arange(c.cap) % len(NQV_CYCLE)]
    c.qmeta.view(torch.int32)[..., 3][torch.arange(NQ)[None, :] >= counts[:, None]] = -1
    c.nq_valid = counts
    ba.check_invariants(c)
    return c


def subcase(base, wins, cap=None):
    """The windows `wins` of `base`, in that order, as a case of their own (same rows, same weights)."""
    c = ba.Case()
    for k in ("C", "groups", "hd", "nq", "K", "N", "xhat", "Wq", "bq", "Wkv", "bkv", "Wo", "bo", "Wpos", "bpos"):
        setattr(c, k, getattr(base, k))
    c.nw = len(wins)
    c.cap = c.nw + 3 if cap is None else cap
    idx = torch.tensor(list(wins) + [wins[0]] * (c.cap - c.nw), dtype=torch.long)
    c.wcentre = base.wcentre[idx].clone()
    c.kmeta = [km[idx].clone() for km in base.kmeta]
    c.qmeta = base.qmeta[idx].clone()
    c.nq_valid = base.nq_valid[idx].clone()
    c.qmeta.view(torch.int32)[c.nw:, :, 3] = -1
    c.nq_valid[c.nw:] = 0
    ba.check_invariants(c)
    return c


_bases = {}


def base(K):
    if K not in _bases:
        _bases[K] = build_base(K, 4 * waves(K, "kv16") + 13)
    return _bases[K]


_mixed = {}


def mixed(K):
    if K not in _mixed:
        _mixed.clear()
        _mixed[K] = ba.OnGpu(base(K))
    return _mixed[K]


# ---- 1. one launch mixing the classes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,form", [(32, "kv16_blobs"), (32, "kv16"), (64, "kv16"), (64, "kv16_blobs")])
def test_one_launch_mixing_one_tile_and_two_tile_windows(K, form):
    g = mixed(K)
    c = g.case
    assert c.nw >= 4 * waves(K, form) and int(g.n_act.item()) == int((c.nq_valid > 0).sum())
    for gi in range(len(GROUPS)):  # the launch holds both kinds of window, in both kinds of pass count
        front = (ba.row_bits(c.kmeta[gi])[:, K // 2:] < 0).all(1)
        for kind in (front, ~front):
            assert bool((kind & (c.nq_valid > 4)).any()) and bool((kind & (c.nq_valid > 0) & (c.nq_valid <= 4)).any())
    ba.check_form(g, form, "tiles mixed K%d" % K)


# ---- 2. position independence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,form", [(32, "kv16_blobs"), (32, "kv16"), (64, "kv16")])
def test_a_window_computes_the_same_bits_wherever_it_stands(K, form):
    b = base(K)
    fixed, others = list(range(40)), list(range(40, 3240))
    assert set(NQV_CYCLE) == set(b.nq_valid[:40].tolist())
    st, alone = ba.OnGpu(subcase(b, fixed)).run(form)
    assert st == 0
    alone = alone[:40 * NQ]
    assert bool((alone != ba.SENTINEL).any())
    for off in (17, 1501, 3100):
        st, attn = ba.OnGpu(subcase(b, others[:off] + fixed + others[off:])).run(form)
        assert st == 0
        assert torch.equal(attn[off * NQ:(off + 40) * NQ], alone), (K, form, off)


# ---- 3. prologue edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,form", [(32, "kv16_blobs"), (32, "kv16"), (64, "kv16")])
@pytest.mark.parametrize("n_act", ["0", "1", "waves", "waves+1"])
def test_active_window_counts_around_the_grid_size(K, form, n_act):
    b = base(K)
    n = {"0": 0, "1": 1, "waves": waves(K, form), "waves+1": waves(K, form) + 1}[n_act]
    active = (b.nq_valid > 0).nonzero()[:, 0].tolist()
    wins = active[:n] if n else [int((b.nq_valid == 0).nonzero()[0, 0])]
    g = ba.OnGpu(subcase(b, wins, cap=len(wins)))  # perm: exactly `cap` entries, all of them listed (n > 0)
    assert g.perm.numel() == len(wins) and int(g.n_act.item()) == n
    ba.check_form(g, form, "prologue K%d n_act=%s" % (K, n_act))
