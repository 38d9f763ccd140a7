"""Reference of everything the window plan writes (csrc/window_plan.hip, csrc/voxel_tables.hip), in plain numpy, plus the
hand-built levels the forms suite plans and the statement of mssvt_plan_order's contract.

`plan_reference` takes what mssvt_window_plan_two / _two_vox take -- voxel coordinates sorted by (b, x, y, z), batch size,
grid, voxel size, range, the four query tables, max_num_win1 / max_num_win2, K and the (list, interp, zero_row) table
variants -- and returns every output of the call.  The three index primitives are the project's oracle (oracle/cref.py,
held to the reference run in tests/test_oracle_golden.py): get_non_empty_window_center, gather_two_window_voxels,
farthest_point_sample on the padded offset lists (block size cref.opt_n_threads(n), inside the oracle) and three_nn.
Everything on top of them is written out here:

  nq_valid, win_vstart   counts of the -1 padded lists; first feature row of the window's sample
  owner_*                the highest flat slot w * maxn + s that holds the voxel, -1 if none does
  vox_win                the window whose win1 list holds the voxel (lists that cannot overlap), -1 if none does
  k_ind, k_mask          the picked list entry round-tripped through fp32 and `(x + 0.1).int()` (oracle/block_ref.py:202-219):
                         a picked EMPTY slot (-1) becomes voxel 0 of the sample; masked = a repeated pick of slot 0 | index < 0
  wcentre, qmeta, kmeta  float32, one rounding per operation as block_ref.with_coords: (idx + 0.5) * cell + lo, minus the window
                         centre; .w = bits of the global feature row; an empty / masked slot is (0, 0, 0, bits(-1)); a picked empty
                         slot that became voxel 0 of the sample takes that voxel's coordinates
  tables, no interp      (w * maxn + slot, zero, zero, 0) / (1, 0, 0, 0) for the voxels of the query list only
  tables, interp         known points = all maxn query slots, empty slots at the world origin (block_ref.py:248-258); indices
                         from cref's three_nn; weights 1 / max(dist, 1e-10), normalised, in float64 from the float32 squared
                         distances; a neighbour that is an empty slot (or a missing third candidate) gets weight 0 and the
                         zero row, and still takes part in the normalisation

Float arrays with a bit-exact contract are returned as int32 views (`*_bits`); tab_w is float64.
"""
import numpy as np

from oracle import cref

F32 = np.float32
HASH_SIZE = 200003
MAX_NUM_WINS = 90000
# tab_w: the header promises the hardware square root and reciprocal at 1 ulp each; a weight is sqrt, rcp, two adds, rcp and a
# multiply on values in (0, 1] -- six operations of <= 2^-23 relative error each, the sum's error shared by three addends whose
# own sqrt and rcp errors enter it again: 8 x 2^-23 relative to the float64 weight, from that operation count
W_BOUND = 8.0 * 2.0 ** -23


def centres(idx_xyz, cell, lo):
    """float32 (idx + 0.5) * cell + lo, one rounding per operation (ref mssvt_backbone.py:132-137)."""
    return (idx_xyz.astype(F32) + F32(0.5)) * np.asarray(cell, F32)[None] + np.asarray(lo, F32)[None]


def weights_f64(d2):
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 1.0 / np.maximum(np.sqrt(d2.astype(np.float64)), 1e-10)
        return w / w.sum(-1, keepdims=True)


def weights_f32(d2):
    """The reference's own evaluation order in float32 (block_ref.py:251-254)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (F32(1.0) / np.maximum(np.sqrt(d2.astype(F32)), F32(1e-10))).astype(F32)
        return (w / w.sum(-1, keepdims=True, dtype=F32)).astype(F32)


def owner_of(ind, wv, num_voxels):
    own = np.full(num_voxels, -1, np.int64)
    rows = (ind.astype(np.int64) + wv[:, None]).reshape(-1)
    ok = ind.reshape(-1) >= 0
    np.maximum.at(own, rows[ok], np.arange(rows.shape[0])[ok])
    return own.astype(np.int32)


def plan_reference(vc, B, grid, voxel_size, pc_range, win1, tables, max1, max2, K, tabs=(), hash_size=HASH_SIZE):
    vc = np.ascontiguousarray(vc, np.int32)
    N = vc.shape[0]
    t = {k: np.ascontiguousarray(np.asarray(tables[k]).reshape(-1, 3), np.int32) for k in ("odd", "even", "win1", "win2")}
    n_o, n_e = t["odd"].shape[0], t["even"].shape[0]
    cnt = cref.bs_cnt(vc, B)
    table = cref.build_hash_table(B, hash_size, grid, vc, cnt)
    wgrid = [grid[i] // win1[i] for i in range(3)]
    win, _ = cref.get_non_empty_window_center(win1, MAX_NUM_WINS, B, hash_size, wgrid, vc)
    o = cref.gather_two_window_voxels(grid, win1, n_o, n_e, max1, max2, t["odd"], t["even"], t["win1"], t["win2"], win, table)
    ind = dict(odd=o[0], even=o[1], win1=o[2], win2=o[3])
    nw = win.shape[0]
    vstart = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    wv = vstart[win[:, 0]]
    r = dict(nw=nw, win_ind=win, ind_odd=o[0], ind_even=o[1], ind_win1=o[2], ind_win2=o[3], win_vstart=wv.astype(np.int32))
    r["nq_valid"] = np.stack([(ind[k] >= 0).sum(1) for k in ("odd", "even", "win1")]).astype(np.int32)
    r["nv2"] = (o[3] >= 0).sum(1).astype(np.int32)
    for k in ("odd", "even", "win1"):
        r["owner_" + k] = owner_of(ind[k], wv, N)
    # vox_win: defined when no voxel sits in two win1 lists
    rows1 = (o[2].astype(np.int64) + wv[:, None])[o[2] >= 0]
    r["disjoint"] = np.unique(rows1).shape[0] == rows1.shape[0]
    vox_win = np.full(N, -1, np.int32)
    vox_win[rows1] = np.nonzero(o[2] >= 0)[0]
    r["vox_win"] = vox_win if r["disjoint"] else None

    vcoord = centres(vc[:, [3, 2, 1]], voxel_size, pc_range[0:3])
    win_size_m = [voxel_size[i] * win1[i] for i in range(3)]
    wc = centres(win[:, [3, 2, 1]], win_size_m, pc_range[0:3])
    r["wcentre_bits"] = np.concatenate([wc, np.zeros((nw, 1), F32)], 1).view(np.int32)

    def meta(local, keep):
        rows = np.where(keep, local.astype(np.int64) + wv[:, None], -1)
        out = np.zeros(local.shape + (4,), F32)
        if N:
            rel = vcoord[np.maximum(rows, 0)] - wc[:, None, :]
            out[..., :3] = np.where(keep[..., None], rel, F32(0))
        bits = out.view(np.int32)
        bits[..., 3] = rows
        return bits

    for k in ("odd", "even", "win1"):
        r["qmeta_%s_bits" % k] = meta(ind[k], ind[k] >= 0)
    for g, (lst, coord) in enumerate(((o[2], o[6]), (o[3], o[7]))):
        fps = cref.farthest_point_sample(coord.astype(F32), K)
        picked = np.take_along_axis(lst, fps.astype(np.int64), 1)
        k_ind = (picked.astype(F32) + F32(0.1)).astype(np.int32)  # C truncation: -0.9 -> 0
        mask = fps == 0
        mask[:, 0] = False
        mask |= k_ind < 0
        r["fps%d" % (g + 1)] = fps
        r["quirk%d" % (g + 1)] = (picked < 0) & ~mask  # a picked empty slot that is voxel 0 of the sample now
        r["k_ind%d" % (g + 1)] = k_ind
        r["k_mask%d" % (g + 1)] = mask.astype(np.uint8)
        r["kmeta%d_bits" % (g + 1)] = meta(k_ind, ~mask)

    r["tabs"] = []
    for lst, interp, zero_row in tabs:
        q = ind[("odd", "even", "win1")[lst]]
        maxn = q.shape[1]
        row = np.full((N, 4), -1, np.int32)
        wgt = np.full((N, 4), np.nan, np.float64)
        extra = {}
        qv = q >= 0
        if not interp:
            w_i, s_i = np.nonzero(qv)
            g = q[qv].astype(np.int64) + wv[w_i]
            row[g] = np.stack([w_i * maxn + s_i, np.full_like(w_i, zero_row), np.full_like(w_i, zero_row), 0 * w_i], 1)
            wgt[g] = np.array([1.0, 0.0, 0.0, 0.0])
        else:
            def coords(l):
                rows = np.where(l >= 0, l.astype(np.int64) + wv[:, None], 0)
                return np.where((l >= 0)[..., None], vcoord[rows], F32(0)).astype(F32)
            d2, idx = cref.three_nn_sq(coords(o[2]), coords(q))
            w = weights_f64(d2)
            nb_valid = np.take_along_axis(qv, idx.reshape(nw, -1).astype(np.int64), 1).reshape(idx.shape) & np.isfinite(d2)
            w = np.where(nb_valid, w, 0.0)
            slot = np.where(nb_valid, np.arange(nw)[:, None, None] * maxn + idx, zero_row)
            v1 = o[2] >= 0
            g = o[2][v1].astype(np.int64) + wv[np.nonzero(v1)[0]]
            row[g] = np.concatenate([slot[v1], np.zeros((g.shape[0], 1), np.int64)], 1)
            wgt[g] = np.concatenate([w[v1], np.zeros((g.shape[0], 1))], 1)
            extra = dict(nn_idx=idx, nn_d2=d2)
        r["tabs"].append(dict(row=row, w=wgt, updated=row[:, 0] >= 0, **extra))
    return r


# ---------------------------------------------------------------------------------------------------------------------
# mssvt_plan_order / mssvt_plan_order_multi: the contract of include/mssvt_hip.h, on numpy arrays
# ---------------------------------------------------------------------------------------------------------------------
def check_plan_order(nq_valid, nw, nq, qmeta_bits, row_cap, perm, n_act, q_off, n_rows, row_src, row_meta_bits):
    """nq_valid (>= nw) ints, qmeta_bits (>= nw, nq, 4) int32 views whose valid slots (.w >= 0) number nq_valid[w] per window;
    the rest: what the call left.  Order is by min(nq_valid, 256) descending, order inside a bucket is free.  Rows at and
    beyond num_rows are not looked at: the header promises nothing about them."""
    nqv = np.asarray(nq_valid[:nw]).astype(np.int64)
    total = int(nqv.sum())
    csum = np.cumsum(nqv)
    assert np.array_equal(np.asarray(q_off[:nw]).astype(np.int64), csum - nqv), "q_off"
    fits = csum <= row_cap
    kept = int(nqv[fits].sum())  # rows of the windows that fit the capacity
    assert int(n_rows) == (total if total <= row_cap else kept), ("num_rows", int(n_rows), total, kept)
    n_act = int(n_act)
    assert n_act == int((nqv > 0).sum()), "num_active"
    perm = np.asarray(perm[:n_act]).astype(np.int64)
    assert np.array_equal(np.sort(perm), np.nonzero(nqv > 0)[0]), "perm is not the set of windows with a query"
    key = np.minimum(nqv, 256)[perm]
    assert bool((key[1:] <= key[:-1]).all()), "perm is not in descending order of min(nq_valid, 256)"
    w, s = np.nonzero(np.asarray(qmeta_bits[:nw])[..., 3] >= 0)  # window order, then slot order
    n = min(total, kept)
    assert np.array_equal(np.asarray(row_src[:n]).astype(np.int64), np.stack([w, w * nq + s], 1)[:n]), "qrow_src"
    assert np.array_equal(np.asarray(row_meta_bits[:n]), np.asarray(qmeta_bits)[w[:n], s[:n]]), "qrow_meta"


# ---------------------------------------------------------------------------------------------------------------------
# hand-built levels
# ---------------------------------------------------------------------------------------------------------------------
GRID = [470, 470, 32]
VOXEL_SIZE = [0.32, 0.32, 0.1875]
RANGE = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.0]
# the natural probes path: z_max > 64 (the same metric extent in x, y; thinner cells in z)
GRID_TALL = [470, 470, 72]
VOXEL_SIZE_TALL = [0.32, 0.32, 0.09375]
RANGE_TALL = [-75.2, -75.2, -2.0, 75.2, 75.2, 4.75]


def standard_tables(win1, win2):
    from oracle import block_ref
    return block_ref.vox_query_table(win1, win2)[0]


def custom_tables(ends):
    """The 9 x 9 x 9 offsets in the standard order, cut anew: odd | even | win1 end at offsets `ends` of the concatenated order
    (the first 125 are the cells of the 5 x 5 x 5 window itself: up to there the lists of different windows cannot overlap),
    win2 = the rest."""
    t = standard_tables([5, 5, 5], [9, 9, 9])
    allo = np.concatenate([t["odd"], t["even"], t["win1"], t["win2"]], 0)
    assert allo.shape[0] == 729 and ends[0] <= ends[1] <= ends[2]
    return {"odd": allo[:ends[0]], "even": allo[ends[0]:ends[1]], "win1": allo[ends[1]:ends[2]], "win2": allo[ends[2]:]}


class Config(object):
    def __init__(self, name, win1, win2, max1, max2, K, tables=None, tall=False):
        self.name, self.win1, self.win2, self.max1, self.max2, self.K, self.tall = name, win1, win2, max1, max2, K, tall
        self.tables = {k: np.ascontiguousarray(v, np.int32) for k, v in (tables or standard_tables(win1, win2)).items()}
        self.custom = tables is not None
        self.grid, self.voxel_size, self.range = (GRID_TALL, VOXEL_SIZE_TALL, RANGE_TALL) if tall else (GRID, VOXEL_SIZE, RANGE)
        self.bs1, self.bs2 = cref.opt_n_threads(max1), cref.opt_n_threads(max2)  # the block size of the reference's sampler
        self.e = np.cumsum([self.tables[k].shape[0] for k in ("odd", "even", "win1", "win2")]).tolist()  # table ends
        lo, hi = [-(w // 2) for w in win1], [w - w // 2 - 1 for w in win1]
        inner = np.concatenate([self.tables[k] for k in ("odd", "even", "win1")], 0)
        self.lists_disjoint = bool(((inner >= lo) & (inner <= hi)).all())  # fused._lists_disjoint
        self.vox_ok = self.lists_disjoint and self.tables["odd"].shape[0] <= max1 and self.e[0] + self.tables["even"].shape[0] <= max1


def configs():
    c = [Config("w335", [3, 3, 5], [7, 7, 7], 45, 343, 32),
         Config("w335_k128", [3, 3, 5], [7, 7, 7], 45, 343, 128),
         Config("w335_cut", [3, 3, 5], [7, 7, 7], 6, 20, 8),
         Config("w222", [2, 2, 2], [4, 4, 4], 8, 64, 64),
         Config("w555", [5, 5, 5], [9, 9, 9], 125, 729, 32),
         Config("w557", [5, 5, 7], [11, 11, 11], 175, 1331, 32),
         Config("w335_min", [3, 3, 5], [7, 7, 7], 1, 3, 8),
         # custom tables: the odd / even / win1 segments end at offsets 63, 64, 65 / 64, 128, 128 (an empty win1 table) of the
         # concatenated order -- the boundaries of the (e - bq) & 63 count logic; short second-scale lists keep the levels small
         Config("w555_e63", [5, 5, 5], [9, 9, 9], 65, 100, 32, tables=custom_tables((63, 64, 65))),
         Config("w555_e128", [5, 5, 5], [9, 9, 9], 128, 150, 8, tables=custom_tables((64, 128, 128))),
         Config("w335_tall", [3, 3, 5], [7, 7, 7], 45, 343, 32, tall=True)]
    return {x.name: x for x in c}


FILLS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513)


def fill_targets(n, bs):
    """The list fills every level holds at a scale whose list has n slots and block size bs."""
    return sorted({f for f in FILLS + (bs - 1, bs, bs + 1, n - 1, n) if 1 <= f <= n})


class Level(object):
    pass


def build_level(cfg, seed=0):
    """B = 3 with an empty middle sample; samples 0 and 2 hold the same cells.  Every named window is placed alone: the second-
    scale neighbourhoods of two named windows never meet, so its fills are the cells placed for it (the windows that its
    second-scale cells open beside it are compared like every other window).  Returns the level with `named`: per window
    its name, (wx, wy, wz) and the hits h1 (first three tables) / h2 (win2 table) placed for it.
    Sizes: 1 152 ... 7 320 voxels, except w555 (13 156) and w557 (25 084): their second-scale fills 511 ... 513, n - 1, n
    (and 1023 ... 1025) cost that many cells, twice for the two samples; each of their cases still takes < 0.3 s on the GPU."""
    rng = np.random.default_rng(seed)
    X, Y, Z = cfg.grid
    ws = cfg.win1
    wg = [cfg.grid[i] // ws[i] for i in range(3)]
    off1 = np.concatenate([cfg.tables[k] for k in ("odd", "even", "win1")], 0).astype(np.int64)
    off2 = cfg.tables["win2"].astype(np.int64)
    tot1, tot2 = off1.shape[0], off2.shape[0]
    lo, hi = np.array([-(w // 2) for w in ws]), np.array([w - w // 2 - 1 for w in ws])
    cells, named = set(), []

    def place(name, w, h1, h2, centre=None, offsets=None):
        c = np.array([w[i] * ws[i] + ws[i] // 2 for i in range(3)])
        in_grid = lambda o: ((c + o >= 0) & (c + o < np.array(cfg.grid))).all(1)  # noqa: E731
        if offsets is None:
            a = off1[in_grid(off1)]
            is_c = (a == 0).all(1)
            own = ((a >= lo) & (a <= hi)).all(1) & ~is_c
            first = a[is_c][:1] if centre else a[own][:1]  # the cell that opens the window
            rest = a[~is_c & ~(a == first[0]).all(1)] if first.shape[0] else a[~is_c]
            if centre is None and h1 > rest.shape[0] + first.shape[0]:
                rest = np.concatenate([rest, a[is_c]], 0)  # a complete neighbourhood holds its centre
            rest = rest[rng.permutation(rest.shape[0])][:max(h1 - first.shape[0], 0)]
            s1 = np.concatenate([first, rest], 0)[:max(h1, 0)]
            b = off2[in_grid(off2)]
            s2 = b[rng.permutation(b.shape[0])][:h2]
        else:
            offsets = np.asarray(offsets, np.int64).reshape(-1, 3)
            offsets = offsets[in_grid(offsets)]
            k1 = (offsets[:, None, :] == off1[None]).all(2).any(1)
            k2 = (offsets[:, None, :] == off2[None]).all(2).any(1)
            s1, s2 = offsets[k1], offsets[k2 & ~k1]
        assert s1.shape[0] and ((s1 >= lo) & (s1 <= hi)).all(1).any(), "no cell of the window itself: %s" % name
        for o in np.concatenate([s1, s2], 0):
            cells.add(tuple(int(v) for v in c + o))
        named.append(dict(name=name, w=tuple(int(v) for v in w), h1=int(s1.shape[0]), h2=int(s2.shape[0]),
                          centre=bool((s1 == 0).all(1).any()), nv1=min(int(s1.shape[0]), cfg.max1),
                          nv2=min(int(s1.shape[0] + s2.shape[0]), cfg.max2)))

    # lattice of sites whose second-scale neighbourhoods are disjoint, clear of the grid's faces
    step = [-(-cfg.win2[i] // ws[i]) + 1 for i in range(3)]
    wz_mid = wg[2] // 2
    sites = [(x, y, wz_mid) for y in range(8, wg[1] // 2, step[1]) for x in range(8, wg[0] - 8, step[0])]
    it = iter(sites)

    # fills of the first scale (few second-scale hits) and of the second scale (few first-scale hits)
    for f in fill_targets(cfg.max1, cfg.bs1):
        place("nv1=%d" % f, next(it), f, 2)
    if tot1 > cfg.max1:  # a cut list: one hit more than it holds, and every cell
        place("h1=%d" % (cfg.max1 + 1), next(it), cfg.max1 + 1, 0)
    place("h1=all", next(it), tot1, 0)  # lives only through its first-scale list
    for f in fill_targets(cfg.max2, cfg.bs2):
        h1 = min(2, f) if f - min(2, f) <= tot2 else f - tot2
        place("nv2=%d" % f, next(it), h1, f - h1)
    if tot1 + tot2 > cfg.max2:
        place("h=%d" % (cfg.max2 + 1), next(it), 2, cfg.max2 - 1)
    place("h=all", next(it), tot1, tot2)  # a completely occupied neighbourhood: the maximal tie case
    # few entries, the centre cell occupied / empty (a hit at offset (0,0,0) ties with every padding slot)
    place("centre", next(it), 3, 2, centre=True)
    place("centre_only", next(it), 1, 0, centre=True)
    place("no_centre", next(it), 3, 2, centre=False)
    # one pattern and its mirror images in x, y, z
    allo = np.concatenate([off1, off2], 0)
    pat = allo[rng.permutation(allo.shape[0])][:9]
    own = off1[((off1 >= lo) & (off1 <= hi)).all(1) & ~(off1 == 0).all(1)][:1]
    pat = np.concatenate([own, pat], 0)
    for nm, sgn in (("pattern", (1, 1, 1)), ("mirror_x", (-1, 1, 1)), ("mirror_y", (1, -1, 1)), ("mirror_z", (1, 1, -1))):
        m = pat * np.array(sgn)
        if not (((m >= lo) & (m <= hi)).all(1) & (m[:, None, :] == off1[None]).all(2).any(1)).any():
            m = np.concatenate([own, m], 0)  # (an even-sized window's mirror image may hold no cell of the window itself)
        place(nm, next(it), 0, 0, offsets=np.unique(m, axis=0))
    # the grid's corners and faces: the second-scale neighbourhood leaves the grid on three, two and one sides
    far = wg[1] - 2 - step[1]
    place("corner_000", (0, 0, 0), tot1, tot2)
    place("edge_00", (0, 0, wz_mid), 5, 9)
    place("face_x0", (0, far, wz_mid), tot1, 7)
    place("corner_last", (wg[0] - 1, wg[1] - 1, wg[2] - 1), tot1, tot2)
    place("face_top", (40, wg[1] - 1, wg[2] - 1), 4, 6)
    place("face_bottom", (60, far, 0), 4, 6)
    # voxels in the cells beyond the last full window, far from every window: in no list
    stray = []
    for ax in range(3):
        if cfg.grid[ax] % ws[ax]:
            p = [300, 400, 3]
            p[ax] = cfg.grid[ax] - 1
            if ax == 2:
                p[0] = 330
            stray.append(tuple(p))
    for p in stray:
        assert all(max(abs(p[i] - q[i]) for i in range(3)) > max(cfg.win2) + max(ws) for q in cells), p
        cells.add(p)
    xyz = np.array(sorted(cells), np.int64)  # sorted by (x, y, z)
    one = lambda b: np.stack([np.full(xyz.shape[0], b), xyz[:, 2], xyz[:, 1], xyz[:, 0]], 1)  # noqa: E731
    L = Level()
    L.cfg, L.B, L.named, L.stray = cfg, 3, named, stray
    L.per_sample = xyz.shape[0]
    L.vc = np.ascontiguousarray(np.concatenate([one(0), one(2)], 0), np.int32)
    L.fills1, L.fills2 = fill_targets(cfg.max1, cfg.bs1), fill_targets(cfg.max2, cfg.bs2)
    have1, have2 = {n["nv1"] for n in named}, {n["nv2"] for n in named}
    assert set(L.fills1) <= have1 and set(L.fills2) <= have2, (cfg.name, set(L.fills1) - have1, set(L.fills2) - have2)
    return L


def window_of(r, b, w):
    """Index of window (wx, wy, wz) of sample b in the reference's window order."""
    hit = np.nonzero((r["win_ind"] == np.array([b, w[2], w[1], w[0]])).all(1))[0]
    assert hit.shape[0] == 1, (b, w)
    return int(hit[0])


def reference_of(L, tabs=()):
    c = L.cfg
    return plan_reference(L.vc, L.B, c.grid, c.voxel_size, c.range, c.win1, c.tables, c.max1, c.max2, c.K, tabs)


def sampler_forms(cfg, nv1, nv2):
    """The sampler forms of csrc/window_plan.hip a level reaches, from its windows' fills and the block sizes alone.
    A RESTATEMENT of the dispatch at the head of the "K7 + K8 + masks" loop of k_window_plan (`if (nv <= MSSVT_WAVE && nv <=
    bs && bs >= 2) ... else if (bs <= 64) ...`): the assertions that a form is reached are as good as this copy -- change
    both together."""
    forms = set()
    for n, bs, nvs in ((cfg.max1, cfg.bs1, nv1), (cfg.max2, cfg.bs2, nv2)):
        for nv in set(int(v) for v in nvs):
            if nv <= 64 and nv <= bs and bs >= 2:
                forms.add("fast<false,4>" if cfg.K > 64 else "fast<true,1>" if nv <= 16 else "fast<true,2>" if nv <= 32 else "fast<true,4>")
            else:
                forms.add("regs<%d>" % max(1, bs // 64))
    return forms
