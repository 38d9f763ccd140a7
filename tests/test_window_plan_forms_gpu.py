"""Every launch form of the window plan (csrc/window_plan.hip: k_window_plan, k_plan_order, k_query_rows; csrc/voxel_tables.hip:
k_voxel_tables) against the plain numpy reference of tests/window_plan_ref.py, on levels built by hand.

The levels (window_plan_ref.build_level) use the synthetic geometry (470 x 470 x 32 cells, +-75 m) and a second grid with
z_max = 72; B = 3 with an EMPTY middle sample, samples 0 and 2 hold the same cells.  Every level is placed window by window:
named windows with first- and second-scale fills 1, 2, 3, 15 / 16 / 17, 31 / 32 / 33, 63 / 64 / 65, bs - 1 / bs / bs + 1,
n - 1 / n (a completely occupied neighbourhood), 255 / 256 / 257 and 511 / 512 / 513 where the list reaches them; windows
with the centre cell occupied / empty; one pattern and its mirror images in x, y, z; windows in the grid's corners and on
its faces; voxels in the cells beyond the last full window.  tests/test_window_plan_ref_cpu.py holds every level to the
fills it claims.  The levels hold 1 152 ... 7 320 voxels; w555 (13 156) and w557 (25 084) are larger than "a few thousand"
because the fills 511 ... 513, 1023 ... 1025, n - 1 and n of a 729- / 1331-slot list cost that many cells in each of the two
samples (each of their cases still runs in < 0.3 s).  The level state comes from the set-up kernels (fused.two_scale_plan(..., all_lists=True)); the C entry points
are then launched again through p._plan_args into outputs pre-filled with sentinels (-7 / NaN; -1 for owner_*, vox_win and
tab_row, as their contract asks).  Every row below nw is compared in full, every row in [nw, cap) must still hold its
sentinel.

Kernels reached, by parametrised id (test_plan_equals_reference[<config>-<mode>]; mode: ranked / columns / probes):

  k_window_plan<4, true>          w335-ranked, w335_k128-ranked, w335_cut-ranked, w222-ranked, w335_min-ranked, w555_e63-ranked,
                                  w555_e128-ranked
  k_window_plan<4, false>         the same configurations with -columns (run-time columns branch) and -probes (hash probes), and
                                  w335_tall-probes (z_max = 72: the probes path without forcing it)
  k_window_plan<4, true, false>   test_vox_then_voxel_tables[w335-ranked], [w335_k128-ranked], [w555_e63-ranked]  (_two_vox)
  k_window_plan<8, true / false>  w555-ranked / w555-columns, w555-probes   (bs2 = 512: 9 x 9 x 9, 729 offsets -- the K3 loop
                                  runs past the six preloaded steps)
  k_window_plan<16, true / false> w557-ranked / w557-columns, w557-probes   (bs2 = 1024)
  k_voxel_tables                  test_vox_then_voxel_tables[*]
  k_plan_order<1> alone           test_plan_order[cap4095], and wherever row_capacity pulls G down to 1
  k_plan_order<0> + <1>           test_plan_order[cap4096 (G = 2), cap6144 (3), cap8192 (4), cap131072 (64), cap133120 (clamp 64)]
  k_query_rows                    every test_plan_order* case

Sampler forms (asserted per configuration from the level's own fills and block sizes, `window_plan_ref.sampler_forms`):

  fps_on_list_fast<true, 1|2|4>   fills <= 16 / <= 32 / <= 64 (and <= bs) of w335, w555, w557, w222, w555_e63, w555_e128
  fps_on_list_fast<false, 4>      w335_k128 (K = 128 > 64)
  fps_on_list_regs<1>             w335 scale 1 (bs = 32: fills 33, 44, 45), w335_cut, w335_min (bs = 1: the bs >= 2 guard)
  fps_on_list_regs<2>             w557 scale 1 (bs = 128), w555_e128
  fps_on_list_regs<4>             w335 scale 2 (bs = 256)
  fps_on_list_regs<8>             w555 scale 2 (bs = 512)
  fps_on_list_regs<16>            w557 scale 2 (bs = 1024)
  with nv > bs, nv == bs and nv == n at every scale whose list allows them.

Compared bit for bit (int32 / float32 viewed as int32): win_ind, ind_odd / even / win1, k_ind1 / 2, k_mask1 / 2, win_vstart,
owner_odd / even / win1, nq_valid, vox_win, wcentre, qmeta_*, kmeta1 / 2 and tab_row -- the 3-NN squared distances are the
same fma chain in the oracle and in the kernel, so the neighbour choice is exact.  tab_w carries the one tolerance:
|w - w64| <= 8 x 2^-23 w64 against the float64 weight (the header promises the hardware square root and reciprocal at 1 ulp
each; a weight is sqrt, rcp, two adds, rcp and a multiply on values in (0, 1]); weights the reference gives as exactly 0 or
exactly 1 must be exactly that.  Between forms: ranked = columns = probes (each equals the same reference, and tab_row /
tab_w of EVERY launch of a table group -- any mode, lists NULL or not, beside _two_vox -- are held bit for bit to the first
launch of the configuration, `OnGpu.same_tables`); num_tabs = 0 / 2 / 4 leave the other outputs unchanged; _two_vox +
mssvt_voxel_tables equal the in-launch tables byte for byte; every optional output NULL in turn leaves the others unchanged,
and all of them NULL with the tables asked for (the whole-frame form) in every mode; two runs agree, with and without
tables; num_wins = 0 writes nothing, tables asked for or not; declined calls return their code and write nothing.  ("vox_win together with num_tabs > 0" cannot be expressed through the header's entry points --
mssvt_window_plan_two takes no vox_win, mssvt_window_plan_two_vox no tables -- so there is no call to decline.)

mssvt_plan_order / mssvt_plan_order_multi run on hand-made nq_valid / qmeta (no plan kernel) against the contract statement
`window_plan_ref.check_plan_order`; rows at and beyond num_rows are only held to the guard behind the capacity.

Measured on the MI355X (all 78 cases in 6 s): every bit-exact comparison held on every configuration and mode, and
mssvt_plan_order's contract held at every size.  Worst tab_w error / bound per configuration (the same in every mode: the
three modes' tables are asserted bit-identical): w222 - (overlapping lists: no tables), w335 0.179, w335_k128 0.179, w335_cut 0.157,
w335_min 0.157, w335_tall 0.206, w555 0.205, w555_e63 0.183, w555_e128 - (no tables), w557 0.199; the float32 numpy
evaluation in the reference's order sits at 0.12 ... 0.28 of the same bound (tests/test_window_plan_ref_cpu.py).

One finding, fixed with its case kept (w555_e63: an even list of ONE slot): with a single 3-NN candidate the reference's
weight is w / w = 1 exactly, while the kernels formed rcp(d) * rcp(rcp(d) + 0 + 0), 1 - 2^-24 for some distances -- inside the
1-ulp promise but not the exact 1 this suite asks for where the reference gives exactly 1.  k_window_plan and
k_voxel_tables now store 1 for a voxel with one candidate (include/mssvt_hip.h says so); no production shape has a query
list of one slot, so no other output changed.

On scratch copies, each of these made the suite fail while test_window_plan_matches_oracle still passed: the sign of
qmeta's x component (qmeta_odd differs, every test_plan_equals_reference case), the .w row of a quirk key (kmeta1 / kmeta2
differ), the third neighbour's weight x 1.00001 (tab_w leaves the bound; _two_vox + mssvt_voxel_tables no longer equal the
in-launch tables), the `run` offset of a later workgroup in k_plan_order (perm is no longer the set of windows with a
query, every case with G > 1).
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import window_plan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

NAMES = ["x_max", "y_max", "z_max", "x_ws", "y_ws", "z_ws", "max_odd", "max_even", "max_win1", "max_win2", "hash_size",
         "batch_size", "num_odd", "num_even", "num_win1", "num_win2", "q_odd", "q_even", "q_win1", "q_win2", "K", "win_indices",
         "num_wins", "cap", "table", "v_bs_cnt", "ind_odd", "ind_even", "ind_win1", "k_ind1", "k_ind2", "k_mask1", "k_mask2",
         "win_vstart", "owner_win1", "owner_odd", "owner_even", "indices", "vs3", "min3", "ws3", "qmeta_odd", "qmeta_even",
         "qmeta_win1", "kmeta1", "kmeta2", "wcentre", "nq_valid", "occ", "fp4", "packed", "vbase", "level_status", "win_counts"]
OUTPUTS = ["ind_odd", "ind_even", "ind_win1", "k_ind1", "k_ind2", "k_mask1", "k_mask2", "win_vstart", "owner_win1", "owner_odd",
           "owner_even", "qmeta_odd", "qmeta_even", "qmeta_win1", "kmeta1", "kmeta2", "wcentre", "nq_valid"]
OPTIONAL = ["ind_odd", "ind_even", "ind_win1", "k_ind1", "k_ind2", "k_mask1", "k_mask2", "owner_win1", "owner_odd", "owner_even",
            "qmeta_odd", "qmeta_even", "qmeta_win1"]
NAN_BITS = int(np.array([np.nan], np.float32).view(np.int32)[0])
MODES = ["ranked", "columns", "probes"]
# (list: 0 odd / 1 even / 2 win1, interpolation): every list with and without interpolation over the two groups
TAB_GROUPS = {"a": [(0, 1), (1, 1), (2, 1), (0, 0)], "b": [(1, 0), (2, 0)]}
ZERO_ROW = 900000
CONFIGS = R.configs()
TPL = {"w335": 4, "w335_k128": 4, "w335_cut": 4, "w222": 4, "w555": 8, "w557": 16, "w335_min": 4, "w555_e63": 4, "w555_e128": 4,
       "w335_tall": 4}
FORMS = {"w335": {"fast<true,1>", "fast<true,2>", "fast<true,4>", "regs<1>", "regs<4>"},
         "w335_k128": {"fast<false,4>", "regs<1>", "regs<4>"},
         "w335_cut": {"fast<true,1>", "regs<1>"},
         "w222": {"fast<true,1>", "fast<true,2>", "fast<true,4>"},
         "w555": {"fast<true,1>", "fast<true,2>", "fast<true,4>", "regs<1>", "regs<8>"},
         "w557": {"fast<true,1>", "fast<true,2>", "fast<true,4>", "regs<2>", "regs<16>"},
         "w335_min": {"fast<true,1>", "regs<1>"},
         "w555_e63": {"fast<true,1>", "fast<true,2>", "fast<true,4>", "regs<1>"},
         "w555_e128": {"fast<true,1>", "fast<true,2>", "fast<true,4>", "regs<2>"},
         "w335_tall": {"fast<true,1>", "fast<true,2>", "fast<true,4>", "regs<1>", "regs<4>"}}


def _tabs_of(group):
    return [(lst, interp, ZERO_ROW + i) for i, (lst, interp) in enumerate(TAB_GROUPS[group])]


def _full(shape, value, dtype=torch.int32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


class OnGpu(object):
    """One configuration: the level, its reference (once), the level state from the set-up kernels, the expectations on the device."""

    def __init__(self, name):
        from mssvt_amd import fused
        from mssvt_amd.mssvt_backbone import MixedScaleSparseTransformerBlock
        from mssvt_amd.mssvt_utils import SparseTensor
        self.cfg = c = CONFIGS[name]
        self.L = L = R.build_level(c)
        self.tab_groups = TAB_GROUPS if c.lists_disjoint else {}
        self.ref = R.reference_of(L, tabs=[t for g in sorted(self.tab_groups) for t in _tabs_of(g)])
        self.N = N = L.vc.shape[0]
        self.blk = blk = MixedScaleSparseTransformerBlock(
            cfg=None, in_channels=32, ff_channels=64, out_channels=32, num_heads=[2, 2], drop_path=0.0, window_size=[c.win1, c.win2],
            max_num_win1=c.max1, max_num_win2=c.max2, cbs_pattern=1, key_num_sample=c.K).to(DEV).eval()
        if c.custom:
            blk.set_vox_query_table({k: torch.from_numpy(v) for k, v in c.tables.items()})
        assert all(np.array_equal(blk.vox_query_table[k].cpu().numpy().reshape(-1, 3), c.tables[k]) for k in c.tables)
        assert fused._lists_disjoint(blk) == c.lists_disjoint
        self.sp = sp = SparseTensor(features=torch.zeros(N, 32, device=DEV), indices=torch.from_numpy(L.vc).to(DEV),
                                    spatial_shape=c.grid, voxel_size=c.voxel_size, point_cloud_range=c.range, batch_size=L.B,
                                    hash_size=R.HASH_SIZE)
        with torch.no_grad():
            self.p = p = fused.two_scale_plan(blk, sp, all_lists=True)
        torch.cuda.synchronize()
        self.cap = p.cap
        self.args = dict(zip(NAMES, p._plan_args))
        assert len(p._plan_args) == len(NAMES) and self.args["cap"] == self.cap and self.args["K"] == c.K
        self.sorted = bool(sp._level.get("sorted"))
        assert self.sorted == (not c.tall) and (self.args["occ"] is None) == c.tall
        self.nw = nw = int(p.num_wins.item())
        assert nw == self.ref["nw"]
        assert np.array_equal(p.win_ind[:nw].cpu().numpy(), self.ref["win_ind"]), "win_ind"
        self.dummy = torch.zeros(4, dtype=torch.int32, device=DEV)
        self.zero = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.expect = {k: torch.from_numpy(v).to(DEV) for k, v in self._expectations().items()}
        self.first_tables = {}  # table group -> (what launched them, tab_row, tab_w) of the first launch of this configuration

    def same_tables(self, out, group, what):
        """tab_row / tab_w of every launch of a table group, in whatever mode or form, equal the first launch's bit for bit
        (the reference holds tab_w to a tolerance only, so it cannot say this)."""
        if group not in self.first_tables:
            self.first_tables[group] = (what, out["tab_row"].clone(), out["tab_w"].clone())
            return
        first, row, w = self.first_tables[group]
        assert torch.equal(out["tab_row"], row), "tab_row of group %s: %s != %s" % (group, what, first)
        assert torch.equal(out["tab_w"].view(torch.int32), w.view(torch.int32)), "tab_w of group %s: %s != %s" % (group, what, first)

    def _expectations(self):
        r, cap, nw = self.ref, self.cap, self.nw
        e = {}

        def rows(k, src, fill, dtype=np.int32):
            a = np.full((cap,) + src.shape[1:], fill, dtype)
            a[:nw] = src
            e[k] = a
        for k in ("ind_odd", "ind_even", "ind_win1", "k_ind1", "k_ind2", "win_vstart"):
            rows(k, r[k], -7)
        for k in ("k_mask1", "k_mask2"):
            rows(k, r[k], 0xF9, np.uint8)
        for k in ("qmeta_odd", "qmeta_even", "qmeta_win1", "kmeta1", "kmeta2", "wcentre"):
            rows(k, r[k + "_bits"], NAN_BITS)
        nqv = np.full((3, cap), -7, np.int32)
        nqv[:, :nw] = r["nq_valid"]
        e["nq_valid"] = nqv
        for k in ("odd", "even", "win1"):
            e["owner_" + k] = r["owner_" + k]
        if r["vox_win"] is not None:
            e["vox_win"] = r["vox_win"]
        return e

    def mode_args(self, mode):
        a = dict(self.args)
        if self.cfg.tall:
            assert mode == "probes"
            return a
        if mode == "ranked":
            a["table"] = None  # the ranked instantiation holds no hash probe: xyz_to_vidx may be NULL
        else:
            a["table"] = self.sp.map_table.data_ptr()
            a["vbase"] = a["level_status"] = None
            if mode == "probes":
                a["occ"] = None
                for k in ("q_odd", "q_even", "q_win1", "q_win2"):
                    a[k] = a[k] or self.dummy.data_ptr()  # (an empty table: any pointer but NULL)
        return a

    def buffers(self, K=None):
        c, cap, N = self.cfg, self.cap, self.N
        K = K or c.K
        n_o, n_e = c.tables["odd"].shape[0], c.tables["even"].shape[0]
        f4 = lambda n: _full((cap, n, 4), float("nan"), torch.float32)  # noqa: E731
        return dict(ind_odd=_full((cap, n_o), -7), ind_even=_full((cap, n_e), -7), ind_win1=_full((cap, c.max1), -7),
                    k_ind1=_full((cap, K), -7), k_ind2=_full((cap, K), -7), k_mask1=_full((cap, K), 0xF9, torch.uint8),
                    k_mask2=_full((cap, K), 0xF9, torch.uint8), win_vstart=_full((cap,), -7), owner_win1=_full((N,), -1),
                    owner_odd=_full((N,), -1), owner_even=_full((N,), -1), qmeta_odd=f4(n_o), qmeta_even=f4(n_e),
                    qmeta_win1=f4(c.max1), kmeta1=f4(K), kmeta2=f4(K), wcentre=_full((cap, 4), float("nan"), torch.float32),
                    nq_valid=_full((3, cap), -7))

    def launch(self, mode, tabs=None, vox=False, null=(), override=None, num_tabs=None):
        """(status, outputs): mssvt_window_plan_two (tabs: list of (list, interp, zero_row)) or _two_vox into fresh sentinels."""
        from mssvt_amd import _lib
        a = self.mode_args(mode)
        out = self.buffers((override or {}).get("K"))
        for k in OUTPUTS:
            a[k] = None if k in null else out[k].data_ptr()
        a.update(override or {})
        head = [a[k] for k in NAMES]
        lib = _lib.lib()
        if vox:
            out["vox_win"] = _full((self.N,), -1)
            st = lib.mssvt_window_plan_two_vox(*head, out["vox_win"].data_ptr(), _lib.stream())
        else:
            tabs = tabs or []
            n = len(tabs) if num_tabs is None else num_tabs
            m = max(n, 1)
            out["tab_row"], out["tab_w"] = _full((m, self.N, 4), -1), _full((m, self.N, 4), float("nan"), torch.float32)
            col = lambda j: (ctypes.c_int * m)(*[int(tabs[i][j]) if i < len(tabs) else 0 for i in range(m)])  # noqa: E731
            pa = lambda t: (ctypes.c_void_p * m)(*[t[i].data_ptr() for i in range(m)])  # noqa: E731
            st = lib.mssvt_window_plan_two(*head, n, col(0), col(1), col(2), pa(out["tab_row"]), pa(out["tab_w"]), _lib.stream())
        torch.cuda.synchronize()
        for k in null:
            del out[k]
        return int(st), out

    def untouched(self, out):
        """Nothing was written: every output still holds its sentinel."""
        for k, t in out.items():
            fresh = -1 if k.startswith("owner") or k in ("vox_win", "tab_row") else 0xF9 if t.dtype == torch.uint8 else -7
            if t.dtype == torch.float32:
                assert bool((t.view(torch.int32) == NAN_BITS).all()), k
            else:
                assert bool((t == fresh).all()), k

    def check(self, out, what=""):
        """Every non-table output against the reference: rows below nw in full, the rest still the sentinel; bit for bit."""
        for k, t in out.items():
            if k in ("tab_row", "tab_w"):
                continue
            want = self.expect[k]
            got = t.view(torch.int32) if t.dtype == torch.float32 else t
            if not torch.equal(got, want):
                bad = (got != want).nonzero()
                first = tuple(int(v) for v in bad[0])
                raise AssertionError("%s %s: %d entries differ, first at %s: got %d, want %d (nw = %d, cap = %d)" % (
                    what, k, bad.shape[0], first, int(got[first]), int(want[first]), self.nw, self.cap))

    def check_tables(self, out, group):
        """tab_row bit for bit; tab_w inside the bound where updated, untouched elsewhere.  Returns the worst error / bound."""
        names = sorted(self.tab_groups)
        base = sum(len(TAB_GROUPS[g]) for g in names[:names.index(group)])
        rows, ws = out["tab_row"].cpu().numpy(), out["tab_w"].cpu().numpy()
        worst = 0.0
        for i, (lst, interp) in enumerate(TAB_GROUPS[group]):
            tab = self.ref["tabs"][base + i]
            upd = tab["updated"]
            assert np.array_equal(rows[i], tab["row"]), "tab_row of table %d (list %d, interp %d)" % (i, lst, interp)
            assert upd.sum() == (self.ref["nq_valid"][2].sum() if interp else self.ref["nq_valid"][lst].sum())
            assert (ws[i][~upd].view(np.int32) == NAN_BITS).all(), "tab_w written for a voxel that is not updated"
            got, want = ws[i][upd].astype(np.float64), tab["w"][upd]
            exact = (want == 0) | (want == 1)
            bad = np.nonzero(exact & (got != want))
            assert bad[0].shape[0] == 0, "table %d (list %d): %d weights the reference gives as exactly 0 or 1 differ, first %r != %r" % (
                i, lst, bad[0].shape[0], got[bad][0], want[bad][0])
            if (~exact).any():
                worst = max(worst, float((np.abs(got - want)[~exact] / want[~exact]).max()) / R.W_BOUND)
        return worst


_cache = {}


def on_gpu(name):
    """The tests of one configuration follow each other, so one is kept."""
    if name not in _cache:
        _cache.clear()
        _cache[name] = OnGpu(name)
    return _cache[name]


def _same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = (t.view(torch.int32) if t.dtype == torch.float32 else t for t in (a[k], b[k]))
        assert torch.equal(x, y), "%s: %s differs" % (what, k)


def _cases():
    out = []
    for name in sorted(CONFIGS):
        for mode in (["probes"] if CONFIGS[name].tall else MODES):
            out.append(pytest.param(name, mode, id="%s-%s" % (name, mode)))
    return out


@pytest.mark.parametrize("name,mode", _cases())
def test_plan_equals_reference(name, mode):
    g = on_gpu(name)
    c, r = g.cfg, g.ref
    # the forms this case reaches, from its own fills and block sizes
    assert (16 if max(c.bs1, c.bs2) > 512 else 8 if max(c.bs1, c.bs2) > 256 else 4) == TPL[name]
    nv1, nv2 = r["nq_valid"][2], r["nv2"]
    assert R.sampler_forms(c, nv1, nv2) == FORMS[name]
    for n, bs, nv in ((c.max1, c.bs1, nv1), (c.max2, c.bs2, nv2)):
        for f in R.fill_targets(n, bs):
            assert (nv == f).any(), (n, bs, f)
    assert (c.e[3] > 6 * 64) == (name in ("w555", "w557", "w555_e63", "w555_e128"))  # the K3 loop past the preloaded steps
    assert (nv2 < c.K).any() and r["quirk2"].any() and (name == "w335_min" or r["quirk1"].any())
    st, plain = g.launch(mode)
    assert st == 0
    g.check(plain, "num_tabs = 0")
    st, again = g.launch(mode)
    assert st == 0
    _same_bits(plain, again, "two runs, num_tabs = 0")
    worst = 0.0
    for group in sorted(g.tab_groups):
        st, out = g.launch(mode, tabs=_tabs_of(group))
        assert st == 0
        g.check(out, "num_tabs = %d" % len(TAB_GROUPS[group]))
        worst = max(worst, g.check_tables(out, group))
        st, again = g.launch(mode, tabs=_tabs_of(group))
        assert st == 0
        _same_bits(out, again, "two runs, table group " + group)  # (tables included)
        g.same_tables(out, group, mode)  # ranked = columns = probes on tab_w too, which the reference holds to a tolerance only
    print("\n%s-%s: N = %d, nw = %d, worst tab_w error / bound = %.3f" % (name, mode, g.N, g.nw, worst))
    assert worst <= 1.0, "the kernel's weights leave the header's promise (1 ulp per square root / reciprocal)"


def _vox_cases():
    return [pytest.param(n, m, id="%s-%s" % (n, m)) for n in sorted(CONFIGS) if CONFIGS[n].vox_ok
            for m in (["probes"] if CONFIGS[n].tall else ["ranked", "columns"])]


@pytest.mark.parametrize("name,mode", _vox_cases())
def test_vox_then_voxel_tables(name, mode):
    """mssvt_window_plan_two_vox (ranked, 4-slot sampler: k_window_plan<4, true, false>) leaves every output of the plan and
    vox_win as the reference states them; mssvt_voxel_tables then builds the in-launch tables byte for byte."""
    from mssvt_amd import _lib
    g = on_gpu(name)
    c = g.cfg
    # k_window_plan<4, true, false>: vox_win, column bases, lists below 512 slots (plan_two_launch)
    assert (mode == "ranked" and max(c.bs1, c.bs2) <= 256) == (mode == "ranked" and name in ("w335", "w335_k128", "w555_e63"))
    st, out = g.launch(mode, vox=True)
    assert st == 0
    g.check(out, "_two_vox")
    assert "vox_win" in g.expect
    for group in sorted(g.tab_groups):
        tabs = _tabs_of(group)
        st, want = g.launch(mode, tabs=tabs)
        assert st == 0
        n = len(tabs)
        got_row, got_w = _full((n, g.N, 4), 7), _full((n, g.N, 4), float("nan"), torch.float32)
        ia = lambda j: (ctypes.c_int * n)(*[int(t[j]) for t in tabs])  # noqa: E731
        pa = lambda t: (ctypes.c_void_p * n)(*[t[i].data_ptr() for i in range(n)])  # noqa: E731
        st = _lib.lib().mssvt_voxel_tables(
            g.N, g.sp.indices.data_ptr(), out["vox_win"].data_ptr(), out["nq_valid"].data_ptr(), g.cap, out["qmeta_odd"].data_ptr(),
            out["qmeta_even"].data_ptr(), out["qmeta_win1"].data_ptr(), c.tables["odd"].shape[0], c.tables["even"].shape[0], c.max1,
            _lib.f3(c.voxel_size), _lib.f3(c.range[0:3]), n, ia(0), ia(1), ia(2), pa(got_row), pa(got_w), 0, None, None, None,
            _lib.stream())
        torch.cuda.synchronize()
        assert st == 0
        assert torch.equal(got_row, want["tab_row"]), "tab_row (written for every voxel)"
        assert torch.equal(got_w.view(torch.int32), want["tab_w"].view(torch.int32)), "tab_w"
        assert g.check_tables(dict(tab_row=got_row, tab_w=got_w), group) <= 1.0
        g.same_tables(want, group, "in-launch tables beside _two_vox, " + mode)


@pytest.mark.parametrize("name", ["w335_cut", "w222"])
def test_every_optional_output_null_in_turn(name):
    """The whole-frame call's form: with the metadata asked for, each list / key / owner / qmeta output may be NULL."""
    g = on_gpu(name)
    for k in OPTIONAL:
        st, out = g.launch("ranked", null=(k,))
        assert st == 0, k
        g.check(out, "%s = NULL" % k)
    for mode in MODES:
        st, out = g.launch(mode, null=tuple(OPTIONAL))  # what mssvt_frame_forward passes
        assert st == 0
        g.check(out, "all optional outputs NULL, " + mode)
        # ... with the tables asked for in the same launch: the other outputs and the tables stay what they were
        for group in sorted(g.tab_groups):
            st, out = g.launch(mode, tabs=_tabs_of(group), null=tuple(OPTIONAL))
            assert st == 0
            g.check(out, "all optional outputs NULL, table group %s, %s" % (group, mode))
            assert g.check_tables(out, group) <= 1.0
            g.same_tables(out, group, "lists NULL, " + mode)
    assert bool(g.tab_groups) == (name == "w335_cut")


@pytest.mark.parametrize("mode", MODES)
def test_no_window_nothing_written(mode):
    g = on_gpu("w335")
    assert g.cfg.vox_ok and g.tab_groups
    st, out = g.launch(mode, override=dict(num_wins=g.zero.data_ptr()))
    assert st == 0
    g.untouched(out)
    st, out = g.launch(mode, tabs=_tabs_of("a"), override=dict(num_wins=g.zero.data_ptr()))  # tables asked for: not touched either
    assert st == 0 and out["tab_row"].shape[0] == 4
    g.untouched(out)
    st, out = g.launch(mode, vox=True, override=dict(num_wins=g.zero.data_ptr()))
    assert st == 0
    g.untouched(out)


BADARG, TOOLARGE = -1, -2


def test_declined_calls_return_their_code_and_write_nothing():
    g = on_gpu("w335_cut")  # (odd table of 20 offsets > max_num_win1 = 6: _two_vox declines it as it stands)
    tabs = _tabs_of("a")
    cases = [("x_ws > 60", TOOLARGE, dict(override=dict(x_ws=61))),
             ("key_num_sample > 1024", TOOLARGE, dict(override=dict(K=1025))),
             ("max_num_win2 >= 2048", TOOLARGE, dict(override=dict(max_win2=2048))),
             ("max_num_win1 >= 2048", TOOLARGE, dict(override=dict(max_win1=2048))),
             ("num_tabs = 5", TOOLARGE, dict(tabs=tabs, num_tabs=5)),
             ("_two_vox, max_num_odd > max_num_win1", TOOLARGE, dict(vox=True)),
             ("_two_vox, num_odd + max_num_even > max_num_win1", TOOLARGE, dict(vox=True, override=dict(max_win1=22))),
             ("kmeta1 without nq_valid", BADARG, dict(null=("nq_valid",))),
             ("column_vbase without level_status_dev", BADARG, dict(override=dict(level_status=None)))]
    for what, code, kw in cases:
        st, out = g.launch("ranked", **kw)
        assert st == code, (what, st)
        g.untouched(out)


# ---------------------------------------------------------------------------------------------------------------------
# mssvt_plan_order / mssvt_plan_order_multi on hand-made nq_valid / qmeta
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _groups(cap, row_cap):
    """Workgroups per list: a RESTATEMENT of mssvt_plan_order_multi_vt's launch code in csrc/window_plan.hip (`int G =
    win_capacity / 2048; if (G > 64) G = 64; while (G > 1 && G * (PO_KEYS + 1) > 2 * row_capacity) --G;`; a workgroup's run is
    per_wg = ceil(nw / G) windows, k_plan_order).  The cases claim their G through this copy: change both together."""
    G = min(cap // 2048, 64)
    while G > 1 and G * 258 > 2 * row_cap:
        G -= 1
    return max(G, 1)


def _make_set(pattern, cap, nq, seed):
    """(nq_valid (cap), qmeta bits (cap, nq, 4)): nq_valid[w] valid slots at random places of window w's row."""
    rng = np.random.default_rng(seed)
    if pattern == "zero":
        nqv = np.zeros(cap, np.int64)
    elif pattern == "equal":
        nqv = np.full(cap, min(nq, 3), np.int64)
    elif pattern == "heavy_last":
        nqv = np.ones(cap, np.int64)  # (the last window of every prefix tested below is made heavy by the caller)
    elif pattern == "above256":
        nqv = rng.integers(0, nq + 1, cap)
        nqv[rng.random(cap) < 0.3] = nq
    else:
        nqv = rng.integers(0, nq + 1, cap)
    order = np.argsort(np.argsort(rng.random((cap, nq)), axis=1), axis=1)
    return nqv.astype(np.int32), order


def _qmeta(nqv, order, seed):
    cap, nq = order.shape
    valid = order < nqv[:, None]
    rng = np.random.default_rng(seed + 1)
    q = rng.standard_normal((cap, nq, 4)).astype(np.float32).view(np.int32)
    q[..., 3] = np.where(valid, rng.integers(0, 1 << 20, (cap, nq)), -1)
    q[..., :3][~valid] = 0
    return q


class OrderRun(object):
    def __init__(self, sets, cap, row_cap):
        """sets: list of (nq_valid np, qmeta bits np, nq)"""
        self.sets, self.cap, self.rc = sets, cap, row_cap
        self.dev = [(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)) for a, b, _ in sets]
        self.num_wins = _full((1,), 0)

    def run(self, nw, single=False):
        from mssvt_amd import _lib
        n, cap, rc = len(self.sets), self.cap, self.rc
        self.num_wins.fill_(nw)
        o = [dict(perm=_full((cap + GUARD,), -7), n_act=_full((1 + GUARD,), -7), q_off=_full((cap + GUARD,), -7),
                  meta=_full((rc + GUARD, 4), float("nan"), torch.float32), src=_full((rc + GUARD, 2), -7),
                  n_rows=_full((1 + GUARD,), -7)) for _ in range(n)]
        lib = _lib.lib()
        if single:
            st = lib.mssvt_plan_order(self.num_wins.data_ptr(), self.dev[0][0].data_ptr(), self.sets[0][2], self.dev[0][1].data_ptr(),
                                      cap, rc, o[0]["perm"].data_ptr(), o[0]["n_act"].data_ptr(), o[0]["q_off"].data_ptr(),
                                      o[0]["meta"].data_ptr(), o[0]["src"].data_ptr(), o[0]["n_rows"].data_ptr(), _lib.stream())
        else:
            pa = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])  # noqa: E731
            st = lib.mssvt_plan_order_multi(n, self.num_wins.data_ptr(), pa([d[0] for d in self.dev]),
                                            (ctypes.c_int * n)(*[s[2] for s in self.sets]), pa([d[1] for d in self.dev]), cap, rc,
                                            pa([x["perm"] for x in o]), pa([x["n_act"] for x in o]), pa([x["q_off"] for x in o]),
                                            pa([x["meta"] for x in o]), pa([x["src"] for x in o]), pa([x["n_rows"] for x in o]),
                                            _lib.stream())
        torch.cuda.synchronize()
        assert st == 0
        return [{k: v.cpu().numpy() for k, v in x.items()} for x in o]

    def check(self, nw, outs, which=None):
        for i, x in enumerate(outs):
            nqv, qm, nq = self.sets[i if which is None else which]
            cap, rc = self.cap, self.rc
            # nothing behind the capacities
            assert (x["perm"][cap:] == -7).all() and (x["q_off"][cap:] == -7).all() and (x["src"][rc:] == -7).all()
            assert (x["meta"][rc:].view(np.int32) == NAN_BITS).all() and (x["n_act"][1:] == -7).all() and (x["n_rows"][1:] == -7).all()
            R.check_plan_order(nqv, nw, nq, qm, rc, x["perm"], x["n_act"][0], x["q_off"], x["n_rows"][0], x["src"],
                               x["meta"].view(np.int32))


CAPS = [4095, 4096, 6144, 8192, 131072, 133120]
G_OF = {4095: 1, 4096: 2, 6144: 3, 8192: 4, 131072: 64, 133120: 64}


def _nws(cap):
    return [0, 1, 63, 64, 65, cap // 2 + 1, cap]


@pytest.mark.parametrize("cap", CAPS, ids=["cap%d" % c for c in CAPS])
def test_plan_order(cap):
    """Every row fits: G workgroups per list as the capacity asks (the row capacity is kept large enough for their histograms)."""
    nq = 4
    for pattern in ("zero", "equal", "heavy_last", "random"):
        nqv, order = _make_set(pattern, cap, nq, cap + len(pattern))
        for nw in _nws(cap):
            v = nqv.copy()
            if pattern == "heavy_last" and nw:
                v[nw - 1] = nq
            v[nw:] = 2  # rows of the capacity beyond nw: never looked at
            qm = _qmeta(v, order, nw)
            rc = max(int(v[:nw].sum()), 64 * 129)
            assert _groups(cap, rc) == G_OF[cap]
            run = OrderRun([(v, qm, nq)], cap, rc)
            run.check(nw, run.run(nw))


@pytest.mark.parametrize("cap", [4095, 4096, 8192], ids=["cap4095", "cap4096", "cap8192"])
def test_plan_order_above_256_queries(cap):
    """nq = 300: the max_key clamp -- every window with >= 256 queries shares the first bucket."""
    nq = 300
    nqv, order = _make_set("above256", cap, nq, cap)
    qm = _qmeta(nqv, order, 5)
    assert (nqv > 256).sum() > cap // 8 and ((nqv > 0) & (nqv < 256)).sum() > cap // 8
    rc = int(nqv.astype(np.int64).sum())
    run = OrderRun([(nqv, qm, nq)], cap, rc)
    for nw in (65, cap // 2 + 1, cap):
        assert _groups(cap, rc) == G_OF[cap]
        run.check(nw, run.run(nw))


@pytest.mark.parametrize("cap", [4096, 6144, 8192, 131072], ids=["cap4096", "cap6144", "cap8192", "cap131072"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_plan_order_straddling_window(cap, where):
    """The window whose rows end beyond row_capacity lies in the first / a middle / the last workgroup's run: it is dropped whole,
    with every window behind it."""
    nq = 8
    nqv, order = _make_set("random", cap, nq, cap + 1)
    nqv = np.maximum(nqv, 4).astype(np.int32)  # (every window can straddle; the rows of ONE run hold the G histograms)
    qm = _qmeta(nqv, order, 9)
    nw = cap - 3
    G = G_OF[cap]
    per_wg = -(-nw // G)
    g = {"first": 0, "middle": G // 2, "last": G - 1}[where]
    w = min(g * per_wg + per_wg - 2, nw - 2)  # late in its workgroup's run
    q_off = np.cumsum(nqv.astype(np.int64)) - nqv
    rc = int(q_off[w]) + 1
    assert _groups(cap, rc) == G and w // per_wg == g and q_off[w] < rc < q_off[w] + nqv[w]
    run = OrderRun([(nqv, qm, nq)], cap, rc)
    outs = run.run(nw)
    assert outs[0]["n_rows"][0] == q_off[w]
    run.check(nw, outs)


@pytest.mark.parametrize("rc,G", [(300, 2), (200, 1), (1, 1)], ids=["G2", "G1", "one_row"])
def test_plan_order_small_row_capacity_reduces_the_workgroups(rc, G):
    cap, nq = 8192, 4
    assert _groups(cap, rc) == G and _groups(cap, 64 * 129) == 4
    nqv, order = _make_set("random", cap, nq, 77)
    qm = _qmeta(nqv, order, 3)
    run = OrderRun([(nqv, qm, nq)], cap, rc)
    for nw in (0, 65, cap // 2 + 1, cap):
        run.check(nw, run.run(nw))


@pytest.mark.parametrize("cap", [4095, 8192], ids=["cap4095", "cap8192"])
@pytest.mark.parametrize("num_sets", [1, 2, 3, 4])
def test_plan_order_multi(cap, num_sets):
    """Lists of different nq in one launch pair; mssvt_plan_order is set 0 of the multi call."""
    nqs = [5, 20, 64, 300][:num_sets]
    sets = []
    for i, nq in enumerate(nqs):
        nqv, order = _make_set("random" if nq < 300 else "above256", cap, nq, 100 * cap + i)
        if i == 1:
            nqv[::3] = 0
        sets.append((nqv, _qmeta(nqv, order, i), nq))
    rc = max(max(int(s[0].astype(np.int64).sum()) for s in sets), 64 * 129)
    run = OrderRun(sets, cap, rc)
    for nw in (1, 65, cap):
        outs = run.run(nw)
        run.check(nw, outs)
        one = run.run(nw, single=True)[:1]
        run.check(nw, one, which=0)
        n = int(one[0]["n_rows"][0])
        assert n == outs[0]["n_rows"][0] and one[0]["n_act"][0] == outs[0]["n_act"][0]
        for k in ("q_off", "src", "meta"):
            m = nw if k == "q_off" else n
            assert np.array_equal(one[0][k][:m].view(np.int32), outs[0][k][:m].view(np.int32)), k


def test_plan_order_declines_zero_and_five_sets():
    from mssvt_amd import _lib
    d = _full((8,), 0)
    for n, code in ((0, BADARG), (5, TOOLARGE)):
        m = max(n, 1)
        pa = (ctypes.c_void_p * m)(*[d.data_ptr()] * m)
        ia = (ctypes.c_int * m)(*[1] * m)
        st = _lib.lib().mssvt_plan_order_multi(n, d.data_ptr(), pa, ia, pa, 8, 8, pa, pa, pa, pa, pa, pa, _lib.stream())
        torch.cuda.synchronize()
        assert st == code and bool((d == 0).all())
