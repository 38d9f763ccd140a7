"""k_attn_kvh<.., 2, true> (csrc/block_attn.hip) walking step lists: two windows whose live keys all sit in key slots 0 .. 15
share a wavefront step -- window B's slots in the upper key tile, the query lists concatenated, each column masking the other
window's tile (mssvt_block_attention_kv16_steps, lists from mssvt_plan_order_steps or written by hand).

Case builder, float64 reference, device harness and the kv16 tolerance (|got - ref| <= 1e-5 max|ref| + 1e-4 |ref|) are those
of tests/test_block_attn_gpu.py, as in tests/test_attn_kvh_tiles_gpu.py: N = 500 feature rows, two head groups of Cg = 64,
head_dim 16, K = 32, nq = 6, about four steps per wave of the launch.

  1. mixed classes in one launch: the live key slots cycle through slot 0 only / 0-14 / 0-15 / tile 0 with holes (pairable) /
     0-16 / all (not pairable), shifted by three classes in the second group so that the two groups pair differently;
     nq_valid cycles 0 .. 6.  Lists from the builder (pairs of equal counts: sums 2, 4, 8, 12 ...) and by hand (sums 5, 1 + 6,
     unequal pairs): the rows are torch.equal to mssvt_block_attention_kv16's and within the tolerance of float64;
  2. partner independence, bit for bit, with hand-built lists: 40 windows as singles, paired (A, B), (B, A) and with other
     partners;
  3. edges: 0 and 1 active windows, an odd number of pairable windows, no pairable window, exactly as many steps as the launch
     has waves and one more, and the window that straddles row_capacity sitting in a pair.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import kvh_pairs_ref as pr
from tests import test_attn_kvh_tiles_gpu as kt
from tests import test_block_attn_gpu as ba

pytestmark = pytest.mark.gpu

K = 32
NQ = kt.NQ
NQV_CYCLE = tuple(range(NQ + 1))
R = lambda a, b: tuple(range(a, b))  # noqa: E731
CLASSES = [(0,), R(0, 15), R(0, 16), kt.HOLES, R(0, 17), R(0, K)]  # the first four: upper tile dead
PAIRABLE = 4


def build_base(nw):
    """nw windows: key class (w + 3 g) mod 6 in group g, nq_valid = w mod 7 in the first slots."""
    c = ba.make_case(128, kt.GROUPS, 16, NQ, K, nw, N=500, seed=5032, keys="all", queries="all", cap=nw)
    for gi, km in enumerate(c.kmeta):
        live = torch.zeros(c.cap, K, dtype=torch.bool)
        for i, slots in enumerate(CLASSES):
            w = torch.arange((i - 3 * gi) % len(CLASSES), c.cap, len(CLASSES))
            live[w[:, None], torch.tensor(slots)[None, :]] = True
        assert bool(live[:, 0].all())
        km.view(torch.int32)[..., 3][~live] = -1
    counts = torch.tensor(NQV_CYCLE, dtype=torch.int32)[torch.arange(c.cap) % len(NQV_CYCLE)]
    c.qmeta.view(torch.int32)[..., 3][torch.arange(NQ)[None, :] >= counts[:, None]] = -1
    c.nq_valid = counts
    ba.check_invariants(c)
    return c


class Paired(ba.OnGpu):
    """OnGpu with the step-list entry points."""

    def flags(self):
        return [pr.upper_live(ba.row_bits(km).cpu().numpy()) for km in self.case.kmeta]

    def built_steps(self):
        """[(steps (cap, 2), num_steps)] per group from mssvt_plan_order_steps; its perm / q_off / rows must be the plain call's."""
        from mssvt_amd import _lib
        c, lib, ng = self.case, _lib.lib(), len(self.case.groups)
        i32 = lambda n, fill: torch.full(n, fill, dtype=torch.int32, device=ba.DEV)  # noqa: E731
        pa = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
        live = [torch.from_numpy(f).to(ba.DEV) for f in self.flags()]
        steps = [i32((c.cap, 2), -7) for _ in range(ng)]
        nst = [i32((1,), -7) for _ in range(ng)]
        scratch = i32((int(lib.mssvt_plan_order_steps_scratch_ints(1, ng)),), -7)
        perm, n_act, q_off, n_rows = i32((c.cap,), -7), i32((1,), -7), i32((c.cap,), -7), i32((1,), -7)
        row_meta = torch.full((self.row_cap, 4), float("nan"), dtype=torch.float32, device=ba.DEV)
        row_src = i32((self.row_cap, 2), -7)
        st = lib.mssvt_plan_order_steps(
            1, self.num_wins.data_ptr(), pa([self.nq_valid]), (ctypes.c_int * 1)(c.nq), pa([self.qmeta]), c.cap, self.row_cap,
            pa([perm]), pa([n_act]), pa([q_off]), pa([row_meta]), pa([row_src]), pa([n_rows]), ng, pa(live), pa(steps), pa(nst),
            scratch.data_ptr(), ba._stream())
        assert st == 0
        torch.cuda.synchronize()
        assert torch.equal(q_off[:c.nw], self.q_off[:c.nw]) and torch.equal(n_act, self.n_act) and torch.equal(n_rows, self.n_rows)
        n = int(n_act.item())
        assert torch.equal(perm[:n].sort().values, self.perm[:n].sort().values)
        nr = int(n_rows.item())
        assert torch.equal(row_src[:nr], self.row_src[:nr]) and torch.equal(row_meta[:nr].view(torch.int32), self.row_meta[:nr].view(torch.int32))
        out = []
        for g in range(ng):
            ns = int(nst[g].item())
            pr.check_steps(c.nq_valid.numpy(), self.flags()[g], c.nw, steps[g].cpu().numpy(), ns)
            assert bool((steps[g][ns:] == -7).all())  # nothing written behind the count
            out.append((steps[g], ns))
        return out

    def run_steps(self, lists):
        """(status, attn) of mssvt_block_attention_kv16_steps on `lists` = per group (steps tensor or list of pairs, count)."""
        from mssvt_amd import _lib
        c, lib = self.case, _lib.lib()
        ia = lambda v: (ctypes.c_int * len(v))(*[int(x) for x in v])  # noqa: E731
        pa = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
        dev = []
        for s, n in lists:
            if not torch.is_tensor(s):  # exactly n steps allocated (one dummy for n = 0): nothing behind them may be read
                s = torch.tensor(list(s) if n else [(-9, -9)], dtype=torch.int32).reshape(-1, 2)
                assert s.shape[0] == max(n, 1)
            dev.append((s.to(ba.DEV).contiguous(), torch.tensor([n], dtype=torch.int32, device=ba.DEV)))
        attn = torch.full((c.cap * c.nq + 1, c.C), ba.SENTINEL, dtype=torch.float32, device=ba.DEV)
        qbuf = torch.full((self.row_cap, self.width), float("nan"), dtype=torch.float32, device=ba.DEV)
        st = lib.mssvt_block_attention_kv16_steps(
            c.C, len(c.groups), ia([g[0] for g in c.groups]), ia([g[1] for g in c.groups]), ia([g[2] for g in c.groups]), c.hd,
            ctypes.c_float(c.scale), c.nq, c.K, self.xhat.data_ptr(), self.n_act.data_ptr(), self.perm.data_ptr(),
            self.q_off.data_ptr(), self.nq_valid.data_ptr(), self.n_rows.data_ptr(), self.row_cap, self.row_meta.data_ptr(),
            self.row_src.data_ptr(), pa(self.kmeta), self.wcentre.data_ptr(), pa(self.Wq), pa(self.bq), pa(self.Wkv), pa(self.bkv),
            pa(self.Wo), pa(self.bo), self.Wpos.data_ptr(), self.bpos.data_ptr(), qbuf.data_ptr(), attn.data_ptr(),
            pa(self.blobs()), pa([d[0] for d in dev]), pa([d[1] for d in dev]), ba._stream())
        torch.cuda.synchronize()
        return int(st), attn


def check_rows(g, attn, what):
    """The existing entry's rows bit for bit, and the float64 reference within the kv16 tolerance."""
    st, plain = g.run("kv16_blobs")
    assert st == 0
    assert torch.equal(attn, plain), what
    ba.sentinel_kept(g, attn)
    if not bool(g.written.any()):
        return
    got, ref = attn.double()[g.written], g.ref[g.written]
    tol = 1e-5 * ref.abs().max() + 1e-4 * ref.abs()
    ratio = float(((got - ref).abs() / tol).max())
    print("RATIO %s steps err/bound=%.3f" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


def hand_steps(c, flags, wins=None, want=()):
    """Steps written on the host for one group: first one pair per (nqA, nqB) of `want`, then the remaining pairable windows
    two by two in window order (unequal counts side by side), the others alone."""
    nqv = c.nq_valid.numpy()
    wins = [w for w in (range(c.nw) if wins is None else wins) if nqv[w] > 0]
    pool = [w for w in wins if flags[w] == 0]
    steps = []
    for na, nb in want:
        a = next(w for w in pool if nqv[w] == na)
        pool.remove(a)
        b = next(w for w in pool if nqv[w] == nb)
        pool.remove(b)
        steps.append((a, b))
    steps += [(pool[i], pool[i + 1]) for i in range(0, len(pool) - 1, 2)]
    if len(pool) % 2:
        steps.append((pool[-1], -1))
    steps += [(w, -1) for w in wins if flags[w] != 0]
    return steps


_base = {}


def base():
    if not _base:
        _base["c"] = build_base(6 * kt.waves(K, "kv16_blobs") + 13)
    return _base["c"]


_mixed = {}


def mixed():
    if not _mixed:
        _mixed["g"] = Paired(base())
    return _mixed["g"]


# ---- 1. mixed classes in one launch ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["builder", "hand"])
def test_mixed_classes_in_one_launch(source):
    g = mixed()
    c, flags = g.case, g.flags()
    nqv = c.nq_valid.numpy()
    assert not np.array_equal(flags[0], flags[1])
    want = [(1, 1), (2, 2), (2, 3), (4, 4), (6, 6), (1, 6)]  # sums 2, 4, 5, 8, 12 and the most unequal pair
    if source == "builder":
        lists = g.built_steps()
    else:
        lists = []
        for f in flags:
            s = hand_steps(c, f, want=want)
            lists.append((s, len(s)))
    for (s, n), f in zip(lists, flags):
        s = (s.cpu().numpy() if torch.is_tensor(s) else np.array(s))[:n]
        pairs = s[s[:, 1] >= 0]
        sums = set((nqv[pairs[:, 0]] + nqv[pairs[:, 1]]).tolist())
        assert {2, 4, 8, 12} <= sums and n >= 3 * kt.waves(K, "kv16_blobs")
        if source == "hand":
            assert 5 in sums and bool(((nqv[pairs[:, 0]] == 1) & (nqv[pairs[:, 1]] == 6)).any())
        assert bool((s[:, 1] < 0).any()) and bool((f[s[s[:, 1] < 0][:, 0]] != 0).any())  # two-tile singles in the same launch
    st, attn = g.run_steps(lists)
    assert st == 0
    check_rows(g, attn, "pairs mixed %s" % source)


# ---- 2. partner independence ------------------------------------------------------------------------------------------------
def test_a_window_computes_the_same_bits_whoever_its_partner_is():
    b = base()
    # pairable in both groups (class index 0 or 3 in group 0), every count 1 .. 6 among them
    fixed = [w for w in range(b.nw) if w % 6 in (0, 3) and int(b.nq_valid[w]) > 0][:40]
    assert set(b.nq_valid[fixed].tolist()) == set(range(1, NQ + 1))
    g = Paired(kt.subcase(b, fixed))
    assert all(int(f[:40].sum()) == 0 for f in g.flags())
    w = list(range(40))
    arrangements = {
        "singles": [(i, -1) for i in w],
        "ab": [(w[i], w[i + 1]) for i in range(0, 40, 2)],
        "ba": [(w[i + 1], w[i]) for i in range(0, 40, 2)],
        "far": [(w[i], w[i + 20]) for i in range(20)],
        "mixed": [(w[i], w[39 - i]) for i in range(10)] + [(i, -1) for i in range(10, 30)],
    }
    st, plain = g.run("kv16_blobs")
    assert st == 0 and bool((plain[:40 * NQ] != ba.SENTINEL).any())
    for name, s in arrangements.items():
        st, attn = g.run_steps([(s, len(s))] * 2)
        assert st == 0
        assert torch.equal(attn, plain), name
    # a different list per group
    st, attn = g.run_steps([(arrangements["ab"], 20), (arrangements["far"], 20)])
    assert st == 0 and torch.equal(attn, plain)


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------
def _pick(b, pred, n):
    out = [w for w in range(b.nw) if pred(w)][:n]
    assert len(out) == n
    return out


@pytest.mark.parametrize("edge", ["0", "1", "odd", "none", "waves", "waves+1"])
def test_edges_of_the_step_list(edge):
    b = base()
    nqv = b.nq_valid
    wv = kt.waves(K, "kv16_blobs")
    both = lambda w: w % 6 in (0, 3) and int(nqv[w]) > 0  # noqa: E731  (pairable in both groups)
    if edge == "0":
        wins = [int((nqv == 0).nonzero()[0, 0])]
    elif edge == "1":
        wins = _pick(b, both, 1)
    elif edge == "odd":
        wins = _pick(b, lambda w: both(w) and int(nqv[w]) == 3, 5)
    elif edge == "none":
        wins = _pick(b, lambda w: w % 6 == 4 and int(nqv[w]) > 0, 7)  # (group 0: both tiles; group 1: slots 0 .. 14)
    else:
        wins = _pick(b, lambda w: w % 6 < PAIRABLE and int(nqv[w]) > 0, 2 * wv + (1 if edge == "waves+1" else 0))  # (group 0)
    g = Paired(kt.subcase(b, wins, cap=len(wins)))
    lists = g.built_steps()
    flags = g.flags()
    if edge == "0":
        assert [n for _, n in lists] == [0, 0]
    elif edge == "1":
        assert [n for _, n in lists] == [1, 1]
    elif edge == "odd":
        assert [n for _, n in lists] == [3, 3]
    elif edge == "none":
        assert lists[0][1] == 7 and int(flags[0].sum()) == 7  # group 0: every window alone
    st, attn = g.run_steps(lists)
    assert st == 0
    check_rows(g, attn, "pairs edge %s built" % edge)
    if edge in ("waves", "waves+1"):  # by hand in group 0: exactly `waves` pairs, then one single more
        n = len(wins)
        assert int(flags[0].sum()) == 0
        s = [(i, i + 1) for i in range(0, 2 * wv, 2)] + [(i, -1) for i in range(2 * wv, n)]
        assert len(s) == wv + (edge == "waves+1")
        st, attn = g.run_steps([(s, len(s)), lists[1]])
        assert st == 0
        check_rows(g, attn, "pairs edge %s hand" % edge)


def test_the_window_past_the_row_capacity_sits_in_a_pair():
    """row_capacity one row short of the last window's end: its rows are skipped, its partner's rows are written and equal to
    the partner's run as a single; as window A and as window B of the pair."""
    b = base()
    wins = [w for w in range(b.nw) if w % 6 in (0, 3) and int(b.nq_valid[w]) >= 2][:9]
    c = kt.subcase(b, wins, cap=len(wins))
    g = Paired(c, row_capacity=c.total_rows - 1)
    last = c.nw - 1
    assert not bool(g.written[last * NQ:(last + 1) * NQ].any()) and int(g.n_rows.item()) == c.total_rows - int(c.nq_valid[last])
    singles = [(i, -1) for i in range(c.nw)]
    st, alone = g.run_steps([(singles, len(singles))] * 2)
    assert st == 0
    check_rows(g, alone, "pairs straddle singles")
    for s in ([(2, last)] + [(i, -1) for i in range(c.nw) if i not in (2, last)],
              [(last, 2)] + [(i, -1) for i in range(c.nw) if i not in (2, last)],
              [(0, 1), (last, 3), (2, 4), (5, 6), (7, -1)]):
        st, attn = g.run_steps([(s, len(s))] * 2)
        assert st == 0
        assert torch.equal(attn, alone)
        assert bool((attn[2 * NQ:2 * NQ + int(c.nq_valid[2])] != ba.SENTINEL).all())
        assert bool((attn[last * NQ:(last + 1) * NQ] == ba.SENTINEL).all())


def test_launch_forms_that_cannot_pair_return_a_status():
    """The K = 64 launch form takes no pairs: the entry point declines (MSSVT_E_TOOLARGE = -2) before it launches anything."""
    g = mixed()
    lists = [([(0, -1)], 1)] * 2
    c = g.case
    keep = c.K
    try:
        c.K = 64
        st, attn = g.run_steps(lists)
    finally:
        c.K = keep
    assert st == -2 and bool((attn == ba.SENTINEL).all())
