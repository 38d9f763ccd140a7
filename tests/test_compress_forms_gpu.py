"""Every launch form of the CompressBlock attention (csrc/compress_ws.hip, csrc/compress_fused.hip) against a float64
restatement of the formula of include/mssvt_hip.h (mssvt_compress_fused: out = projs(softmax_v(scale (Wq max_v xhat_v + bq) .
(Wk k_v + bk)) (Wv k_v + bv)), k_v = xhat_v + pos_proj([centre_v - centre_w ; centre_w]); ref mssvt_backbone.py:351-383,
mssvt_utils.py:112-150 with nq = 1).

The C entry points are driven directly (mssvt_compress_ws, mssvt_compress_ws_chunked, mssvt_compress_ws_pack,
mssvt_compress_fused) on levels built BY HAND in numpy -- never by the plan kernels: a case gives, per column (b, x, y), the
occupied z cells, z_ws, ns and z_listed (cells z >= z_listed are in no window); the builder derives indices sorted by
(b, x, y, z), pair_win, win_cnt, win_ind, win_vstart, k_ind.  The geometry is synthetic.py's (columns at both ends of the
x / y range: positional inputs of +-75 m).  xhat and indices carry 32 rows behind n (xhat: NaN), `out` a sentinel.

Kernels reached, by parametrised id:
  test_ws_structural_*[<case>]               k_cmp_ws<128>: search form at 1, 2, 3 workgroups and at the natural grid;
                                             handed-in ends of mssvt_voxel_tables and hand-made ends (`all0`, `each`,
                                             `sizes`, `repeat`); k_cmp_ws_pack<128>.  <case> = ones, full32, never_full,
                                             mixed8 / 16 / 32, odd3 / 5 / 12 (ns = z_ws), odd3 / 5 / 12_ns32, unlisted,
                                             nw1 / 15 / 16 / 17 / 31 / 33, n1, two_samples
  test_ws_grid_equals_the_cu_count           k_cmp_ws<128>, one workgroup per CU, search = every handed-in cut
  test_ws_input_classes[<level>-<class>]     k_cmp_ws<128> search form (edge100: all work in chunk 0)
  test_ws_pack_* / test_ws_declined_*        k_cmp_ws_pack<128> / no launch
  test_fused_*[<C>x<hd>-f32-*]               k_cmp_query_keys<C, false>, k_cmp_kv<C, hd, false>, k_cmp_out<C, hd, false>
  test_fused_*[<C>x<hd>-split-*]             k_cmp_query_keys<C, true>, k_cmp_kv<C, hd, true>, k_cmp_out<C, hd, true>
      (C, hd) in 128x16, 128x32, 64x8, 64x16, 64x32, 32x8, 32x16, 32x32: the 16 forms
  test_fused_agrees_with_ws[<case>]          both files on the same level (128x16, split)

Tolerances, per WINDOW row: s_w = max(1, max_c |want[w, c]|), e = |got - want| / s_w, e32 the same for a float32 torch
evaluation of the same formulas in the reference's operation order.
  ln, scaled, negative (and every structural case)   max e <= 4 max e32 + 1e-6, mean e <= 4 mean e32; the split-fp16 forms
                                                      (k_cmp_ws, split_f16 = 1): + max e16 and + mean e16, see below
  far, edge100, top_xhat / hidden / ktok / v          max e <= 8 max e32, mean e <= 8 mean e32
  and the cap of tests/test_compress_ws_gpu.py on top: max|got - want| <= 2e-5 max(1, max|want|); far / edge100: 2e-3 max,
  2e-5 mean (same global scale).
e16: the first run on the MI355X put the MEAN error of the split-fp16 forms at 4.1 ... 6.9 x mean e32 (max: 1.2 ... 2.7 x max
e32) on `ln` / `negative`, the fp32-instruction forms at <= 2.4 x.  The operation that accounts for it is the split itself:
v_cvt_pkrtz_f16_f32 cuts every operand of the four chained C x C products to 22 of fp32's 24 mantissa bits TOWARD ZERO (a
one-sided error of mean 2^-23 per operand against fp32's centred 2^-25), and lo x lo is dropped.  It is bounded separately,
not by a larger factor: e16 = |float64 formula with exactly those operands cut (`split22`) - float64| / s_w, a figure of
the number format computed by the reference alone, is added to the bound of the split forms in the classes held to the
factor 4.  The classes held to 8 x e32 take no such term.
Input classes: `ln` rows as a LayerNorm leaves them; `scaled` rows x 10^U(-2, 2); `negative` xhat = -|randn| on half of the
channels (the zero padding decides the query token of every partial window); `far` Wq, bq x 60; `edge100` Wq, bq x a factor
computed from the float64 scores so that about half of the 16-row pieces pass |score log2 e| = 100 (the builder asserts
the plain -> merge and merge -> plain windows; on `unlisted` the rows in no window carry scores the builder cannot know, so
there the fraction is that of the listed rows); `top_*` one operand (max|xhat|, the positional hidden layer, the key token,
the V row) at 0.6 x 65504 in ONE channel j, by scaling column j of xhat or row j of pos_proj.0, pos_proj.2 or Wv; column j of
the matrices that read the operand is damped by 1 / 64 (entries stay fp16 normals) and `scale` (a plain fp32 factor) lowered
until max|score| <= 20, so that nothing else moves and the softmax stays sensitive (scaling a whole matrix makes every key
token of a window the same positional term, and no test could see a wrong score).  top_xhat: the key token = xhat +
positional term sits at the top with it.
Tolerance-free: every cut of one level gives the same bits; two runs agree; stale NaN = stale sentinel; rows [nw, capacity)
keep the sentinel; num_wins = 0 writes nothing; declined calls write nothing; an empty list gives bo bit for bit.
win_capacity only sizes the grid of mssvt_compress_ws (min(ceil(capacity / 16), CUs); the kernel takes nw from the device), so
capacities 16 / 32 / 48 put 1 / 2 / 3 workgroups over any level; `out` always holds max(nw, capacity) + 32 rows.
tests/test_compress_ref_cpu.py checks the reference itself without a GPU.

Measured on the MI355X (256 CUs), worst over all cases of a class (every test prints its own RATIO line), as
max / bound, mean / bound, cap -- and the same errors as multiples of max e32, mean e32:
  k_cmp_ws      ln 0.32 0.49 0.06 (3.4 x, 4.4 x)      scaled 0.33 0.36 0.83 (2.1 x, 2.3 x)   negative 0.27 0.48 0.05 (1.9 x, 4.2 x)
                far 0.15 0.29 0.02 (1.2 x, 2.3 x)     edge100 0.29 0.33 0.01 (2.3 x, 2.6 x)
                top_xhat 0.29 0.43 0.04 (2.3 x, 3.4 x)   top_hidden 0.25 0.55 0.07 (2.0 x, 4.4 x)
                top_ktok 0.37 0.54 0.07 (2.9 x, 4.3 x)   top_v 0.48 0.66 0.08 (3.8 x, 5.3 x)
  fused, split  ln 0.42 0.73 0.09 (5.9 x, 6.9 x)      scaled 0.24 0.29 0.05 (1.2 x, 1.6 x)   negative 0.35 0.42 0.05 (3.5 x, 3.1 x)
                far 0.18 0.19 0.02 (1.4 x, 1.6 x)     top_xhat 0.35 0.42 0.05   top_hidden 0.28 0.42 0.05
                top_ktok 0.31 0.42 0.06               top_v 0.22 0.39 0.06      (top_*: at most 2.8 x, 3.4 x)
  fused, fp32   ln 0.27 0.37 0.05 (1.6 x, 1.5 x)      scaled 0.21 0.25 0.04 (0.9 x, 1.0 x)   negative 0.19 0.25 0.02 (1.1 x, 1.0 x)
                far 0.19 0.12 0.01 (1.5 x, 1.0 x)
  k_cmp_ws against the split three-launch form on the 21 structural levels: at most 0.08 of the sum of their bounds.
(ln: every structural case and the LDS-limit lists included; the worst mean, 6.9 x mean e32, is 32x16 on one window.)
Every cut of every structural level, the level of one workgroup per CU included, gave the same bits; every other
tolerance-free property held; nothing in compress_ws.hip or compress_fused.hip had to change.
"""
import math

import numpy as np
import pytest
import torch

from mssvt_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"

F16_MAX = 65504.0
E_BADARG, E_TOOLARGE = -1, -2
SENTINEL = -12345.678
TOP_TARGET = 0.6
LOOSE_RATIO, TIGHT_RATIO = 8.0, 4.0
TOP_CLASSES = ("top_xhat", "top_hidden", "top_ktok", "top_v")
LOOSE = ("far", "edge100") + TOP_CLASSES
CLASSES = ("ln", "scaled", "negative") + LOOSE
FUSED_SHAPES = [(128, 16), (128, 32), (64, 8), (64, 16), (64, 32), (32, 8), (32, 16), (32, 32)]
MUTATIONS = ("pad_never", "pad_always", "centre_voxel_z", "mask_rel", "mask_rel_inverted", "no_scale", "pow2", "swap_heads", "no_bv", "no_relu2",
             "drop_cross16_last", "group_first_pred_query")
X_MAX, Y_MAX = synthetic.GRID_SIZE[0], synthetic.GRID_SIZE[1]
VS = [float(v) for v in synthetic.VOXEL_SIZE]
MN = [float(v) for v in synthetic.POINT_CLOUD_RANGE[:3]]
LDS_BYTES = 160 * 1024


# ---------------------------------------------------------------------------------------------------------------------
# 1. levels (numpy, by hand)
# ---------------------------------------------------------------------------------------------------------------------
class Level(object):
    """n rows, nw windows; indices (n + 32, 4) [b, z, y, x] sorted by (b, x, y, z); pair_win (n + 32), -1: in no window;
    win_cnt (nw), win_ind (nw, 4) [b, z / z_ws, y, x], win_vstart (nw), k_ind (nw, ns) offsets from win_vstart, -1 padded;
    z_ws, ns, win_size (metres); runs: every window is a run of rows, numbered in row order (what compress_ws.hip takes)."""

    pass


def z_magic_holds(z_ws):
    """(z * (65536 / z_ws + 1)) >> 16 == z / z_ws for every cell z < 64 (CwArgs::z_magic)."""
    return all((z * (65536 // z_ws + 1)) >> 16 == z // z_ws for z in range(64))


def level_from_columns(cols, z_ws, ns, z_listed=64):
    """cols: (b, x, y, [z cells]) in any order."""
    assert 1 <= z_ws <= ns and z_magic_holds(z_ws)
    cols = sorted((int(b), int(x), int(y), sorted(set(int(z) for z in zs))) for b, x, y, zs in cols)
    assert len(set(c[:3] for c in cols)) == len(cols)
    idx, pw, cnt, wind, vstart = [], [], [], [], []
    for b, x, y, zs in cols:
        assert 0 <= x < X_MAX and 0 <= y < Y_MAX and all(0 <= z < 64 for z in zs)
        last = None
        for z in zs:
            if z < z_listed:
                if last != z // z_ws:
                    last = z // z_ws
                    cnt.append(0)
                    wind.append((b, last, y, x))
                    vstart.append(len(idx))
                cnt[-1] += 1
                pw.append(len(cnt) - 1)
            else:
                pw.append(-1)
            idx.append((b, z, y, x))
    L = Level()
    L.n, L.nw, L.z_ws, L.ns, L.runs = len(idx), len(cnt), z_ws, ns, True
    L.win_size = [VS[0], VS[1], z_ws * VS[2]]
    ind = np.asarray(idx, dtype=np.int32).reshape(-1, 4)
    L.indices = np.concatenate([ind, np.repeat(ind[-1:], 32, 0)], 0)
    L.pair_win = np.concatenate([np.asarray(pw, dtype=np.int32), np.full(32, -1, np.int32)])
    L.win_cnt = np.asarray(cnt, dtype=np.int32)
    L.win_ind = np.asarray(wind, dtype=np.int32).reshape(-1, 4)
    L.win_vstart = np.asarray(vstart, dtype=np.int32)
    k = np.arange(ns, dtype=np.int32)[None, :].repeat(L.nw, 0)
    L.k_ind = np.where(k < L.win_cnt[:, None], k, -1).astype(np.int32)
    check_level(L)
    return L


def check_level(L):
    assert L.indices.shape == (L.n + 32, 4) and L.pair_win.shape == (L.n + 32,) and L.k_ind.shape == (L.nw, L.ns)
    assert (L.win_cnt >= 0).all() and (L.win_cnt <= L.ns).all()
    slot = np.arange(L.ns)[None, :]
    assert ((L.k_ind >= 0) == (slot < L.win_cnt[:, None])).all()
    rows = L.win_vstart[:, None] + L.k_ind
    listed = rows[L.k_ind >= 0]
    assert (listed >= 0).all() and (listed < L.n).all() and np.unique(listed).size == listed.size  # disjoint lists
    assert ((L.win_vstart >= 0) & (L.win_vstart < max(L.n, 1))).all()
    owner = np.full(L.n, -1, np.int64)
    owner[listed] = np.nonzero(L.k_ind >= 0)[0]
    assert (owner == L.pair_win[:L.n]).all() and (L.pair_win[L.n:] == -1).all()
    if L.runs:
        assert (L.win_cnt >= 1).all() and (np.diff(L.pair_win[:L.n][L.pair_win[:L.n] >= 0]) >= 0).all()
        key = ((L.indices[:L.n, 0].astype(np.int64) * X_MAX + L.indices[:L.n, 3]) * Y_MAX + L.indices[:L.n, 2]) * 64 + L.indices[:L.n, 1]
        assert (np.diff(key) > 0).all()


def _column_sites(rng, k, B=1):
    """k columns per sample at both ends of the x / y range, (0, 0) and (X - 1, Y - 1) among them."""
    xs = list(range(8)) + list(range(X_MAX - 8, X_MAX))
    sites = [(x, y) for x in xs for y in range(Y_MAX)]
    corners = [(0, 0), (X_MAX - 1, Y_MAX - 1)] if k >= 2 else []
    sites = [p for p in sites if p not in corners]
    out = []
    for b in range(B):
        pick = corners + [sites[i] for i in rng.permutation(len(sites))[:k - len(corners)]]
        out += [(b,) + p for p in sorted(pick)]
    return out


def _slab_cells(rng, z_ws, counts, z_top=32):
    """Cells of one column: slab s gets counts[s] cells (0: none)."""
    zs = []
    for s, c in enumerate(counts):
        lo, hi = s * z_ws, min((s + 1) * z_ws, z_top)
        if c and hi > lo:
            zs += [lo + int(v) for v in rng.permutation(hi - lo)[:min(c, hi - lo)]]
    return zs


def mixed_level(z_ws, ns, columns, seed, z_top=32, B=1):
    rng = np.random.RandomState(seed)
    slabs = (z_top + z_ws - 1) // z_ws
    cols = []
    for b, x, y in _column_sites(rng, columns, B):
        counts = [int(rng.randint(1, z_ws + 1)) if rng.rand() < 0.8 else 0 for _ in range(slabs)]
        if not any(counts):
            counts[0] = 1
        cols.append((b, x, y, _slab_cells(rng, z_ws, counts, z_top)))
    return level_from_columns(cols, z_ws, ns)


def exact_windows_level(nw, seed):
    """Exactly nw windows of 1 ... 32 rows (z_ws = ns = 32: one window per column)."""
    rng = np.random.RandomState(seed)
    cols = [(b, x, y, _slab_cells(rng, 32, [int(rng.randint(1, 33))])) for b, x, y in _column_sites(rng, nw)]
    assert len(cols) == nw
    return level_from_columns(cols, 32, 32)


def structural_level(name, small=False):
    """The structural cases of compress_ws.hip; small: a few windows of the same kind (the CPU restatement)."""
    rng = np.random.RandomState(1000 + sum(ord(ch) for ch in name))
    if name == "ones":  # every window one row: every 16-row piece is a whole group
        L = level_from_columns([(b, x, y, [int(rng.randint(0, 32))]) for b, x, y in _column_sites(rng, 5 if small else 48)], 32, 32)
        assert small or L.nw == 48
        assert (L.win_cnt == 1).all()
    elif name == "full32":  # 15 rows, then full windows: each spans three pieces, carried twice; full lists start from -inf
        sites = _column_sites(rng, 3 if small else 21)
        L = level_from_columns([(b, x, y, range(15) if i == 0 else range(32)) for i, (b, x, y) in enumerate(sites)], 32, 32)
        assert L.win_cnt[0] == 15 and (L.win_cnt[1:] == 32).all()
        assert all(s // 16 + 2 == (s + 31) // 16 for s in L.win_vstart[1:])
    elif name == "never_full":
        L = mixed_level(8, 32, 4 if small else 150, 11)
        assert (L.win_cnt < L.ns).all()
    elif name.startswith("mixed"):
        z = int(name[5:])
        L = mixed_level(z, z, 3 if small else {8: 120, 16: 120, 32: 150}[z], 12 + z)
        assert (L.win_cnt == L.ns).any() or small
    elif name.startswith("odd"):  # z / z_ws by z_magic, cells up to z = 63
        z = int(name[3:].split("_")[0])
        L = mixed_level(z, 32 if name.endswith("_ns32") else z, 3 if small else 40, 13 + z, z_top=64)
        assert L.indices[:, 1].max() == 63 or small
    elif name == "unlisted":
        # z_listed = 24 below the grid top: the level begins and ends with a column of unlisted rows only, and two neighbouring
        # columns in the middle hold cells above z_listed only (>= 64 consecutive rows in no window between two windows)
        sites = _column_sites(rng, 6 if small else 40)
        mid = len(sites) // 2
        cols = []
        for i, (b, x, y) in enumerate(sites):
            if i in (0, len(sites) - 1):
                zs = [24 + int(v) for v in rng.permutation(40)[:5]]
            elif i in (mid, mid + 1):
                zs = list(range(24, 30 if small else 64))
            else:
                zs = [int(v) for v in rng.permutation(64)[:int(rng.randint(1, 40))]]
                zs.append(int(rng.randint(0, 24)))
            cols.append((b, x, y, zs))
        L = level_from_columns(cols, 12, 12, z_listed=24)
        pw = L.pair_win[:L.n]
        assert pw[0] < 0 and pw[-1] < 0 and (pw >= 0).any()
        gaps = np.diff(np.nonzero(pw >= 0)[0]) - 1
        assert small or gaps.max() >= 64
    elif name.startswith("nw"):
        L = exact_windows_level(int(name[2:]), 14)
    elif name == "n1":
        L = level_from_columns([(0, X_MAX - 1, 0, [7])], 32, 32)
    elif name == "two_samples":  # the sample boundary inside a 16-row piece and inside a group of 16 windows
        L = mixed_level(16, 16, 3 if small else 21, 15, B=2)
        first = int(np.nonzero(L.indices[:L.n, 0] == 1)[0][0])
        assert small or (first % 16 != 0 and L.pair_win[first] % 16 != 0)
    else:
        raise KeyError(name)
    return L


STRUCTURAL = ("ones", "full32", "never_full", "mixed8", "mixed16", "mixed32", "odd3", "odd5", "odd12", "odd3_ns32", "odd5_ns32",
              "odd12_ns32", "unlisted", "nw1", "nw15", "nw16", "nw17", "nw31", "nw33", "n1", "two_samples")
# levels of the input classes; odd3 beside the three of the structural list because its full lists hold three rows: a channel
# whose maximum over a FULL list is negative (where the initial key of the max must be -inf and not 0) has probability 2^-3
# there against 2^-8 on mixed8 and 2^-32 on full32
CLASS_LEVELS = ("mixed8", "full32", "unlisted", "odd3")


def fused_level(nw, ns, seed, long_list=0):
    """Lists that are NOT runs: the rows of two neighbouring windows are interleaved, the slot order of every list is
    shuffled, rows in no list lie between them, window 2 (nw >= 15) is EMPTY (win_cnt = 0, slot 0 = -1), n is no multiple of
    16.  long_list: window 0 lists that many rows."""
    rng = np.random.RandomState(seed)
    cnt = rng.randint(1, min(ns, 12) + 1, size=nw)
    if long_list:
        cnt[0] = long_list
    if nw >= 15:
        cnt[2] = 0
    rows_of, pw = [[] for _ in range(nw)], []
    for w0 in range(0, nw, 2):
        labels = [w0] * int(cnt[w0]) + ([w0 + 1] * int(cnt[w0 + 1]) if w0 + 1 < nw else [])
        for w in [labels[i] for i in rng.permutation(len(labels))]:
            rows_of[w].append(len(pw))
            pw.append(w)
        pw += [-1] * int(rng.randint(0, 3))
    while len(pw) % 16 == 0 or len(pw) < 3:
        pw.append(-1)
    n = len(pw)
    ends = np.asarray(list(range(4)) + list(range(X_MAX - 4, X_MAX)))
    L = Level()
    L.n, L.nw, L.z_ws, L.ns, L.runs = n, nw, 8, ns, False
    L.win_size = [VS[0], VS[1], 8 * VS[2]]
    ind = np.stack([np.zeros(n, np.int64), rng.randint(0, 32, n), ends[rng.randint(0, 8, n)], ends[rng.randint(0, 8, n)]], 1).astype(np.int32)
    L.indices = np.concatenate([ind, np.repeat(ind[-1:], 32, 0)], 0)
    L.pair_win = np.concatenate([np.asarray(pw, dtype=np.int32), np.full(32, -1, np.int32)])
    L.win_cnt = cnt.astype(np.int32)
    L.win_vstart = np.asarray([min(r) if r else 0 for r in rows_of], dtype=np.int32)
    L.k_ind = np.full((nw, ns), -1, np.int32)
    for w, r in enumerate(rows_of):
        r = np.asarray(r, dtype=np.int32)
        L.k_ind[w, :r.size] = r[rng.permutation(r.size)] - L.win_vstart[w]
    first = ind[L.win_vstart]
    L.win_ind = np.stack([first[:, 0], first[:, 1] // 8, first[:, 2], first[:, 3]], 1).astype(np.int32)
    check_level(L)
    assert n % 16 != 0 and (L.pair_win[:n] < 0).any()
    return L


# ---------------------------------------------------------------------------------------------------------------------
# 2. parameters and inputs (torch, seeded, CPU tensors)
# ---------------------------------------------------------------------------------------------------------------------
class Case(object):
    NAMES = ("xhat", "Wp1", "bp1", "Wp2", "bp2", "Wq", "bq", "Wkv", "bkv", "Wo", "bo")


def _uniform(g, shape, bound):
    return (torch.rand(shape, generator=g) * 2 - 1) * bound


def _linear(g, out_f, in_f):
    """nn.Linear default init: weight and bias uniform in +-1/sqrt(fan_in)."""
    b = 1.0 / math.sqrt(in_f)
    return _uniform(g, (out_f, in_f), b), _uniform(g, (out_f,), b)


def _layer_norm_rows(g, n, C):
    x = torch.randn(n, C, generator=g) * 10.0 ** (torch.rand(n, 1, generator=g) * 2.0 - 1.0)
    d = x - x.mean(1, keepdim=True)
    return d / torch.sqrt((d * d).mean(1, keepdim=True) + 1e-5) * (1.0 + _uniform(g, (C,), 0.1)) + _uniform(g, (C,), 0.1)


def make_case(L, cls="ln", C=128, hd=16, seed=0):
    assert cls in CLASSES and C % hd == 0
    g = torch.Generator().manual_seed(9000 + 17 * seed + C + hd + L.n % 1013)
    c = Case()
    c.L, c.cls, c.C, c.hd, c.scale = L, cls, C, hd, float(hd) ** -0.5
    c.Wp1, c.bp1 = _linear(g, C, 6)
    c.Wp2, c.bp2 = _linear(g, C, C)
    c.Wq, c.bq = _linear(g, C, C)
    c.Wkv, c.bkv = _linear(g, 2 * C, C)
    c.Wo, c.bo = _linear(g, C, C)
    x = _layer_norm_rows(g, L.n, C)
    if cls == "scaled":
        x = x * 10.0 ** (torch.rand(L.n, 1, generator=g) * 4.0 - 2.0)
    if cls == "negative":
        half = torch.randperm(C, generator=g)[:C // 2]
        x[:, half] = -torch.randn(L.n, C // 2, generator=g).abs()
    c.xhat = torch.cat([x, torch.full((32, C), float("nan"))], 0)
    if cls == "far":
        c.Wq, c.bq = c.Wq * 60.0, c.bq * 60.0
    if cls == "edge100":
        m = piece_score_max(c)
        f = 100.0 / float(np.median(m[m > 0]))
        c.Wq, c.bq = c.Wq * f, c.bq * f
    if cls in TOP_CLASSES:
        _near_f16_top(c)
    for k in Case.NAMES[1:]:
        assert bool(torch.isfinite(getattr(c, k)).all())
    assert bool(torch.isfinite(c.xhat[:L.n]).all()) and bool(torch.isnan(c.xhat[L.n:]).all())
    return c


def piece_score_max(c):
    """max |score log2 e| over the listed rows and the heads of every piece [16 k, 16 k + 16) -- the pieces of a launch with all
    work in chunk 0; float64.  (Pieces without a listed row: 0.)"""
    L = c.L
    st = reference(c)[1]
    s = (st["score"].abs().amax(2) * math.log2(math.e)).numpy()  # (nw, ns)
    rows = L.win_vstart[:, None] + np.maximum(L.k_ind, 0)
    per_row = np.zeros(L.n)
    per_row[rows[L.k_ind >= 0]] = s[L.k_ind >= 0]
    pad = (-L.n) % 16
    return np.concatenate([per_row, np.zeros(pad)]).reshape(-1, 16).max(1)


def check_edge100(c):
    """Between 25 % and 75 % of the pieces pass the limit; a window spans a plain piece followed by a merge piece; a window
    spans a merge piece followed by a plain one (its second piece takes the merge form too: the reference has moved)."""
    L = c.L
    over = piece_score_max(c) > 100.0
    frac = float(over.mean())
    assert 0.25 <= frac <= 0.75, frac
    first, last = L.win_vstart // 16, (L.win_vstart + L.win_cnt - 1) // 16
    assert L.runs
    up = down = 0
    for a, b in zip(first, last):
        for p in range(a, b):
            up += (not over[p]) and over[p + 1]
            down += over[p] and (not over[p + 1])
    assert up >= 1 and down >= 1, (up, down)
    return frac, int(up), int(down)


OPERANDS = ("xhat", "hidden", "ktok", "v")


def _near_f16_top(c):
    """ONE channel of one operand at TOP_TARGET x 65504 (module docstring): the channel j in which the operand is largest is
    scaled through what produces it -- column j of xhat, row j of pos_proj.0 / pos_proj.2 / Wv with its bias -- and the
    columns j of the matrices that read it are damped by 1 / 64, so that every other operand stays where it was and the
    softmax stays as sensitive to its scores as in the `ln` class."""
    C, n = c.C, c.L.n
    which = c.cls[4:]
    tgt = TOP_TARGET * F16_MAX
    st = reference(c)[1]
    j = st[which + "_ch"]
    damp = 1.0 / 64.0
    if which == "xhat":
        c.xhat[:n, j] *= tgt / st["xhat"]
        c.Wq[:, j] *= damp
        c.Wkv[:, j] *= damp
    elif which == "hidden":
        s = tgt / st["hidden"]
        c.Wp1[j], c.bp1[j] = c.Wp1[j] * s, c.bp1[j] * s
        c.Wp2[:, j] *= damp
    elif which == "ktok":
        s = tgt / st["pos"]  # (first guess: the positional term dominates after the scaling)
        c.Wp2[j], c.bp2[j] = c.Wp2[j] * s, c.bp2[j] * s
        c.Wkv[:, j] *= damp
        for _ in range(3):
            cur = reference(c)[1]
            assert cur["ktok_ch"] == j
            s = 1.0 + (tgt - cur["ktok"]) / cur["pos"]
            c.Wp2[j], c.bp2[j] = c.Wp2[j] * s, c.bp2[j] * s
    else:
        s = tgt / st["v"]
        c.Wkv[C + j], c.bkv[C + j] = c.Wkv[C + j] * s, c.bkv[C + j] * s
        c.Wo[:, j] *= damp
    smax = reference(c)[1]["score_max"]
    if smax > 20.0:  # (the damped column still carries 0.6 x 65504 / 64 of one channel into the scores)
        c.scale = c.scale * 20.0 / smax


def check_top(c, st):
    """The operand the class names sits at 0.6 x 65504 (2 %), the others below 0.5 x -- except the key token of top_xhat,
    which is xhat plus a positional term and so sits with it."""
    which = c.cls[4:]
    assert abs(st[which] / (TOP_TARGET * F16_MAX) - 1.0) < 0.02, (which, st[which])
    for op in OPERANDS:
        if op != which and not (which == "xhat" and op == "ktok"):
            assert st[op] < 0.5 * F16_MAX, (c.cls, op, st[op])
        assert st[op] < 0.9 * F16_MAX
    for W in (c.Wp2, c.Wq, c.Wkv, c.Wo):  # the matrices are operands too: inside the range, damped columns fp16 normals
        assert float(W.abs().max()) < 0.5 * F16_MAX
    assert st["score_max"] <= 20.0 * (1 + 1e-9)


# ---------------------------------------------------------------------------------------------------------------------
# 3. reference
# ---------------------------------------------------------------------------------------------------------------------
def split22(t):
    """(hi, lo) of the split-fp16 operands (cw_split4 / cf_split4): hi = fp16(v) and lo = fp16((v - hi) 2^11) / 2^11, both
    rounded TOWARD ZERO (v_cvt_pkrtz_f16_f32), fp16 subnormals included: 22 of fp32's 24 mantissa bits, truncated."""
    def rtz16(v):
        a = v.abs()
        e = torch.floor(torch.log2(a.clamp(min=2.0 ** -40))).clamp(min=-14.0)
        q = torch.pow(torch.full_like(a, 2.0), e - 10.0)
        return torch.sign(v) * (torch.floor(a / q) * q).clamp(max=F16_MAX)
    hi = rtz16(t)
    return hi, rtz16((t - hi) * 2048.0) / 2048.0


def _product(x, W, split):
    """x W^T; split: as the three MFMA chains form it from the halves, hi hi + (hi lo + lo hi) -- lo lo is dropped."""
    if not split:
        return x @ W.T
    xh, xl = split22(x)
    Wh, Wl = split22(W)
    return xh @ Wh.T + (xl @ Wh.T + xh @ Wl.T)


def reference(case, dtype=torch.float64, device="cpu", mutate=None, chunk=1024, split=False):
    """(out (nw, C), stats) in `dtype`: the header's formula of mssvt_compress_fused on the lists of the level.  stats
    (float64 only meaningful): max|xhat| over the rows, max of the positional hidden layer / the positional term / the key
    tokens / |V| over the listed slots, the scores (nw, ns, heads; -inf where not listed) when the level is small.
    split: the four C x C products with their operands cut to two fp16 halves (`split22`), everything else unchanged --
    in float64 this isolates what the split-fp16 FORMAT costs, whatever the kernel's summation order."""
    c, L = case, case.L
    C, hd, ns, nw, n = c.C, c.hd, L.ns, L.nw, L.n
    NH = C // hd
    f = lambda t: t.to(device).to(dtype)  # noqa: E731
    i64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device).long()  # noqa: E731
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=device)  # noqa: E731
    xhat = f(c.xhat[:n])
    Wp1, bp1, Wp2, bp2, Wq, bq, Wkv, bkv, Wo, bo = [f(getattr(c, k)) for k in Case.NAMES[1:]]
    ind, wind = i64(L.indices[:n]), i64(L.win_ind)
    vs, mn, wsz = f32(VS), f32(MN), f32(L.win_size)
    vcen = (ind[:, [3, 2, 1]].float() + 0.5) * vs + mn    # fp32, ((i + 0.5) cell) + lo, then promoted
    wcen = (wind[:, [3, 2, 1]].float() + 0.5) * wsz + mn
    out = torch.empty((nw, C), dtype=dtype, device=device)
    stats = dict(xhat=float(xhat.abs().max()) if n else 0.0, xhat_ch=int(xhat.abs().amax(0).argmax()) if n else 0, hidden=0.0,
                 pos=0.0, ktok=0.0, v=0.0, score_max=0.0)
    scores = []
    slot = torch.arange(ns, device=device)[None, :]
    cnt_all, k_all, vst_all = i64(L.win_cnt), i64(L.k_ind), i64(L.win_vstart)
    for w0 in range(0, nw, chunk):
        w1 = min(nw, w0 + chunk)
        cnt, k_ind = cnt_all[w0:w1], k_all[w0:w1]
        valid = slot < cnt[:, None]
        if mutate == "drop_cross16_last":  # the last row of every window that crosses a 16-row boundary left out
            rows_ = vst_all[w0:w1, None] + k_ind.clamp(min=0)
            lo = torch.where(valid, rows_, torch.full_like(rows_, 1 << 40)).amin(1)
            hi = torch.where(valid, rows_, torch.full_like(rows_, -1)).amax(1)
            cross = (lo // 16 != hi // 16) & (cnt > 0)
            valid = valid & ~(cross[:, None] & (rows_ == hi[:, None]))
        rows = vst_all[w0:w1, None] + k_ind.clamp(min=0)
        x = xhat[rows] * valid[..., None]                                  # zero padded key features
        neg = torch.full_like(x, float("-inf"))
        q_tok = torch.where(valid[..., None], x, neg).amax(1)
        padded = cnt < ns                                                  # the zero padding takes part exactly then
        if mutate == "pad_never":
            padded = torch.zeros_like(padded)
        if mutate == "pad_always":
            padded = torch.ones_like(padded)
        q_tok = torch.where(padded[:, None], q_tok.clamp(min=0.0), q_tok)
        q_tok = torch.where(torch.isfinite(q_tok), q_tok, torch.zeros_like(q_tok))  # (an empty full list cannot exist)
        vc = vcen[rows].to(dtype)
        wc = wcen[w0:w1, None, :].expand(-1, ns, -1).to(dtype)
        if mutate == "centre_voxel_z":
            wc = torch.cat([wc[..., :2], vc[..., 2:]], -1)
        rel = vc - wc                                                      # NOT masked
        if mutate == "mask_rel":  # as the Block masks it: the slots that are not listed
            rel = rel * valid[..., None]
        if mutate == "mask_rel_inverted":  # ... with the mask's polarity wrong: the listed slots
            rel = rel * (~valid)[..., None]
        geo = torch.cat([rel, wc], -1)
        h = torch.relu(geo @ Wp1.T + bp1)
        pos = _product(h, Wp2, split) + bp2
        if mutate != "no_relu2":
            pos = torch.relu(pos)
        k_tok = x + pos
        q = _product(q_tok, Wq, split) + bq
        if mutate != "no_scale":
            q = q * c.scale
        if mutate == "group_first_pred_query" and nw > 1:
            # every window that opens a group of 16 takes the query of the window before it
            assert nw <= chunk
            first = (torch.arange(nw, device=device) % 16 == 0) & (torch.arange(nw, device=device) > 0)
            q = torch.where(first[:, None], torch.cat([q[:1], q[:-1]], 0), q)
        kv = _product(k_tok, Wkv, split) + bkv
        K, V = kv[..., :C], kv[..., C:]
        if mutate == "no_bv":
            V = V - bkv[C:]
        V = V.reshape(w1 - w0, ns, NH, hd)
        if mutate == "swap_heads":
            V = torch.cat([V[:, :, 1:2], V[:, :, 0:1], V[:, :, 2:]], 2)
        s = (q[:, None, :] * K).reshape(w1 - w0, ns, NH, hd).sum(-1)
        s = s.masked_fill(~valid[..., None], float("-inf"))
        if mutate == "pow2":
            s = s * math.log(2.0)
        pr = torch.softmax(s, 1)
        pr = torch.where(valid[..., None], pr, torch.zeros_like(pr))       # (an empty list: 0, not NaN -> the row is bo)
        o = (pr[..., None] * V).sum(1).reshape(w1 - w0, C)
        out[w0:w1] = _product(o, Wo, split) + bo
        if dtype == torch.float64 and bool(valid.any()):
            m = valid[..., None]
            for key, t in (("hidden", h), ("pos", pos), ("ktok", k_tok), ("v", V.reshape(w1 - w0, ns, C))):
                per_ch = (t * m).abs().reshape(-1, C).amax(0)
                if float(per_ch.max()) > stats[key]:
                    stats[key], stats[key + "_ch"] = float(per_ch.max()), int(per_ch.argmax())
            stats["score_max"] = max(stats["score_max"], float(s[valid].abs().max()))
            if nw * ns <= (1 << 20):
                scores.append(s.cpu())
    if scores:
        stats["score"] = torch.cat(scores, 0)
    return out, stats


def row_scale(want):
    return want.abs().amax(1, keepdim=True).clamp(min=1.0)


def tolerance_ratios(cls, got, want, e32, e16=None):
    """error / bound of the three rules (module docstring): (max rule, mean rule, cap).  e16: the split-fp16 format's own
    error (split forms, classes held to the factor 4), added to the bound of the max and of the mean."""
    if want.shape[0] == 0:
        return 0.0, 0.0, 0.0
    diff = (got - want).abs()
    e = diff / row_scale(want)
    gs = max(1.0, float(want.abs().max()))
    if cls in LOOSE:
        r_max, r_mean = float(e.max()) / (LOOSE_RATIO * float(e32.max())), float(e.mean()) / (LOOSE_RATIO * float(e32.mean()))
    else:
        x_max, x_mean = (0.0, 0.0) if e16 is None else (float(e16.max()), float(e16.mean()))
        r_max = float(e.max()) / (TIGHT_RATIO * float(e32.max()) + 1e-6 + x_max)
        r_mean = float(e.mean()) / (TIGHT_RATIO * float(e32.mean()) + x_mean)
    if cls in ("far", "edge100"):
        cap = max(float(diff.max()) / (2e-3 * gs), float(diff.mean()) / (2e-5 * gs))
    else:
        cap = float(diff.max()) / (2e-5 * gs)
    return r_max, r_mean, cap


# ---------------------------------------------------------------------------------------------------------------------
# 4. launch arithmetic (the launchers' own formulas)
# ---------------------------------------------------------------------------------------------------------------------
def ws_groups(capacity, cus):
    """mssvt_compress_ws_groups (csrc/compress_ws.hip): min(ceil(capacity / 16), CUs)."""
    return min((capacity + 15) // 16, cus) if capacity > 0 else 0


def fused_lds(C, ns):
    """launch_compress (csrc/compress_fused.hip): (query launch, output launch) bytes."""
    lds1 = (C * (C + 4) + C) * 4
    return lds1 + 12 * 16 * ns * 4, lds1 + 16 * 16 * ns * 4


def fused_ns_limit(C):
    """The largest list capacity launch_compress admits: both launches within 160 KiB."""
    return (LDS_BYTES - (C * (C + 4) + C) * 4) // (16 * 16 * 4)


def fused_grids(C, ns, n, capacity, split, cus):
    """(g_w, g_v): query and key workgroups of k_cmp_query_keys."""
    per_q = max(1, LDS_BYTES // fused_lds(C, ns)[0])
    slots = cus * per_q
    vt, wt = (n + 15) // 16, (capacity + 15) // 16
    g_w = min(max(slots // 2 if split else slots // 3, 1), max(wt, 1))
    return g_w, min(max(slots - g_w, 1), max(vt, 1))


def ends_from_cuts(L, G, cuts):
    """(G + 1, 2) chunk ends (window, first row) with a cut in front of every window of `cuts` (at most G - 1 of them are
    used; repeated cuts give empty chunks), (0, 0) first, (nw, n) for the rest."""
    cuts = [w for w in cuts if 0 < w < L.nw][:max(G - 1, 0)]
    rows = [(0, 0)] + [(w, int(L.win_vstart[w])) for w in cuts]
    rows += [(L.nw, L.n)] * (G + 1 - len(rows))
    e = np.asarray(rows, dtype=np.int32)
    assert e.shape == (G + 1, 2) and (np.diff(e, axis=0) >= 0).all()
    return e


def hand_made_ends(L, G):
    """name -> ends: all work in chunk 0; a cut after every one of the first G - 1 windows; chunks of 1, 15, 16, 17 and 33
    windows; repeated ends (empty chunks in the middle)."""
    third = max(L.nw // 3, 1)
    return {"all0": ends_from_cuts(L, G, []), "each": ends_from_cuts(L, G, range(1, G)),
            "sizes": ends_from_cuts(L, G, [1, 16, 32, 49, 82]),
            "repeat": ends_from_cuts(L, G, sorted([third] * 3 + [2 * third] * 2))}


# ---------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------
def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


class OnGpu(object):
    """A case on the device, its float64 reference and float32 evaluation (computed once, shared)."""

    def __init__(self, case):
        from mssvt_amd import _lib
        self.case, L = case, case.L
        self.lib = _lib.lib()
        for k in Case.NAMES:
            setattr(self, k, getattr(case, k).to(DEV).contiguous())
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
        one = lambda a, shape: dev(a) if a.size else torch.zeros(shape, dtype=torch.int32, device=DEV)  # noqa: E731
        self.indices, self.pair_win = dev(L.indices), dev(L.pair_win)
        self.win_cnt, self.win_vstart = one(L.win_cnt, (1,)), one(L.win_vstart, (1,))
        self.win_ind, self.k_ind = one(L.win_ind, (1, 4)), one(L.k_ind, (1, L.ns))
        self.num_wins = torch.tensor([L.nw], dtype=torch.int32, device=DEV)
        self.vs3, self.mn3, self.ws3 = _lib.f3(VS), _lib.f3(MN), _lib.f3(L.win_size)
        self.want, self.stats = reference(case, device=DEV)
        self._e32 = self._e16 = self._packed = None

    def e32(self):
        if self._e32 is None:
            o32 = reference(self.case, dtype=torch.float32, device=DEV)[0]
            assert bool(torch.isfinite(o32).all())
            self._e32 = (o32.double() - self.want).abs() / row_scale(self.want)
        return self._e32

    def e16(self):
        if self._e16 is None:
            o16 = reference(self.case, device=DEV, split=True)[0]
            self._e16 = (o16 - self.want).abs() / row_scale(self.want)
        return self._e16

    def packed(self):
        from mssvt_amd import _lib
        if self._packed is None:
            nbytes = int(self.lib.mssvt_compress_ws_packed_bytes(128))
            self._packed = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
            assert self.lib.mssvt_compress_ws_pack(128, self.Wp2.data_ptr(), self.Wq.data_ptr(), self.Wkv.data_ptr(),
                                                   self.Wo.data_ptr(), self._packed.data_ptr(), _lib.stream()) == 0
        return self._packed

    def out_buffer(self, capacity, fill=SENTINEL):
        return torch.full((max(self.case.L.nw, capacity) + 32, self.case.C), fill, dtype=torch.float32, device=DEV)

    def ws(self, capacity=None, ends=None, fill=SENTINEL, out=None, num_wins=None, n=None, **over):
        """mssvt_compress_ws (ends None) / mssvt_compress_ws_chunked; returns (status, out).  `over`: C, head_dim, z_ws, ns,
        chunk_groups and null=<argument name> build the declined calls."""
        from mssvt_amd import _lib
        c, L = self.case, self.case.L
        capacity = max(L.n, 1) if capacity is None else capacity
        out = self.out_buffer(capacity, fill) if out is None else out
        nwd = self.num_wins if num_wins is None else torch.tensor([num_wins], dtype=torch.int32, device=DEV)
        a = dict(num_wins=nwd.data_ptr(), indices=self.indices.data_ptr(), win_cnt=self.win_cnt.data_ptr(),
                 pair_win=self.pair_win.data_ptr(), vs=self.vs3, mn=self.mn3, ws=self.ws3, xhat=self.xhat.data_ptr(),
                 Wp1=self.Wp1.data_ptr(), bp1=self.bp1.data_ptr(), bp2=self.bp2.data_ptr(), bq=self.bq.data_ptr(),
                 bkv=self.bkv.data_ptr(), bo=self.bo.data_ptr(), packed=self.packed().data_ptr(), out=out.data_ptr())
        if over.get("null"):
            a[over["null"]] = None
        args = [over.get("C", c.C), over.get("head_dim", c.hd), c.scale, over.get("z_ws", L.z_ws), over.get("ns", L.ns),
                L.n if n is None else n, a["num_wins"], capacity, a["indices"], a["win_cnt"], a["pair_win"], a["vs"], a["mn"],
                a["ws"], a["xhat"], a["Wp1"], a["bp1"], a["bp2"], a["bq"], a["bkv"], a["bo"], a["packed"], a["out"]]
        if ends is None:
            st = self.lib.mssvt_compress_ws(*(args + [_lib.stream()]))
        else:
            e = torch.from_numpy(np.ascontiguousarray(ends)).to(DEV) if isinstance(ends, np.ndarray) else ends
            st = self.lib.mssvt_compress_ws_chunked(*(args + [e.data_ptr(), over.get("chunk_groups", e.shape[0] - 1), _lib.stream()]))
        torch.cuda.synchronize()
        return int(st), out

    def table_ends(self, G):
        """Chunk ends of mssvt_voxel_tables for a grid of G workgroups."""
        from mssvt_amd import _lib
        ends = torch.full((G + 1, 2), -7, dtype=torch.int32, device=DEV)
        st = self.lib.mssvt_voxel_tables(self.case.L.n, None, None, None, 0, None, None, None, 0, 0, 0, None, None, 0, None, None,
                                         None, None, None, G, self.num_wins.data_ptr(), self.pair_win.data_ptr(),
                                         ends.data_ptr(), _lib.stream())
        torch.cuda.synchronize()
        assert st == 0, st
        return ends

    def fused(self, split, capacity=None, fill=float("nan"), ns=None):
        """mssvt_compress_fused with every scratch buffer pre-filled with `fill`; returns (status, out, scratch)."""
        from mssvt_amd import _lib
        c, L = self.case, self.case.L
        capacity = max(L.nw, 1) if capacity is None else capacity
        out = self.out_buffer(capacity)
        full = lambda r, w: torch.full((r, w), fill, dtype=torch.float32, device=DEV)  # noqa: E731
        scratch = [full(max(capacity, L.nw) + 1, c.C), full(L.n + 1, c.C), full(L.n + 1, c.C // c.hd), full(L.n + 1, c.C)]
        st = self.lib.mssvt_compress_fused(
            c.C, c.hd, c.scale, L.ns if ns is None else ns, L.n, self.num_wins.data_ptr(), capacity, self.win_ind.data_ptr(),
            self.indices.data_ptr(), self.k_ind.data_ptr(), self.win_vstart.data_ptr(), self.win_cnt.data_ptr(),
            self.pair_win.data_ptr(), self.vs3, self.mn3, self.ws3, self.xhat.data_ptr(), self.Wp1.data_ptr(), self.bp1.data_ptr(),
            self.Wp2.data_ptr(), self.bp2.data_ptr(), self.Wq.data_ptr(), self.bq.data_ptr(), self.Wkv.data_ptr(),
            self.bkv.data_ptr(), self.Wo.data_ptr(), self.bo.data_ptr(), scratch[0].data_ptr(), scratch[1].data_ptr(),
            scratch[2].data_ptr(), scratch[3].data_ptr(), out.data_ptr(), 1 if split else 0, _lib.stream())
        torch.cuda.synchronize()
        return int(st), out, scratch

    def check(self, out, what, split=True):
        """Rows [0, nw) against float64 under the class's tolerance; the rows behind keep the sentinel."""
        c, nw = self.case, self.case.L.nw
        assert bool((out[nw:] == SENTINEL).all()), (what, "rows past nw were written")
        got = out[:nw].double()
        assert bool(torch.isfinite(got).all()), what
        r = tolerance_ratios(c.cls, got, self.want, self.e32(), self.e16() if split and c.cls not in LOOSE else None)
        if c.L.nw:
            e = (got - self.want).abs() / row_scale(self.want)
            print("RATIO %s %s max/bound=%.3f mean/bound=%.3f cap=%.3f (x e32: max %.2f mean %.2f; e32 max %.2e mean %.2e; e16 max %.2e mean %.2e)" % (
                what, c.cls, r[0], r[1], r[2], float(e.max() / self.e32().max()), float(e.mean() / self.e32().mean()),
                float(self.e32().max()), float(self.e32().mean()), float(self.e16().max()), float(self.e16().mean())))
        assert max(r) <= 1.0, (what, c.cls, r)
        empty = np.nonzero(c.L.win_cnt == 0)[0]
        for w in empty:
            assert torch.equal(out[w], self.bo), (what, "empty list", int(w))
        return r


_cache = {}


def on_gpu(key, build):
    """One case kept on the device: the tests of a case follow each other."""
    if key not in _cache:
        _cache.clear()
        _cache[key] = OnGpu(build())
    return _cache[key]


def _structural(name, cls="ln"):
    return on_gpu(("ws", name, cls), lambda: make_case(structural_level(name), cls))


# ---- compress_ws.hip: structural cases under every cut -----------------------------------------------------------------------
def _all_cuts(g):
    """name -> (status, out) of one level under every cut of the issue's list."""
    L, cus = g.case.L, _cus()
    runs = {}
    for k in (1, 2, 3):
        assert ws_groups(16 * k, cus) == k
        runs["search%d" % k] = g.ws(capacity=16 * k)
    cap = max(L.n, 1)
    G = int(g.lib.mssvt_compress_ws_groups(cap))
    assert G == ws_groups(cap, cus)
    runs["search"] = g.ws()
    runs["tables"] = g.ws(ends=g.table_ends(G))
    for name, e in hand_made_ends(L, G).items():
        runs[name] = g.ws(ends=e)
    return runs, G


def _same_bits(name, L, runs):
    """Every cut of one level: status OK, the rows behind nw untouched, rows [0, nw) bit-identical to the search form."""
    st0, base = runs["search"]
    assert st0 == 0
    for cut, (st, out) in runs.items():
        assert st == 0, (cut, st)
        assert bool((out[L.nw:] == SENTINEL).all()), cut
        bad = (out[:L.nw] != base[:L.nw]).any(1).nonzero()[:, 0]
        assert bad.numel() == 0, "%s: cut `%s` differs from the search form in %d windows, first %s" % (name, cut, bad.numel(), bad[:8].tolist())


@pytest.mark.parametrize("name", STRUCTURAL)
def test_ws_structural_case_under_every_cut(name):
    g = _structural(name)
    L = g.case.L
    runs, G = _all_cuts(g)
    _same_bits(name, L, runs)
    g.check(runs["search"][1], "ws %s G=%d n=%d nw=%d" % (name, G, L.n, L.nw))


@pytest.mark.parametrize("name", ("mixed16", "full32", "unlisted", "two_samples"))
def test_ws_two_runs_and_stale_memory(name):
    g = _structural(name)
    nw = g.case.L.nw
    a, b, c = g.ws()[1], g.ws()[1], g.ws(fill=float("nan"))[1]
    assert torch.equal(a, b)
    assert torch.equal(a[:nw], c[:nw]) and bool(torch.isnan(c[nw:]).all())


def test_ws_grid_equals_the_cu_count():
    cus = _cus()
    cols = 16 * cus + 40  # z_ws = 32: one window per column
    g = on_gpu(("ws", "big"), lambda: make_case(mixed_level(32, 32, cols, 77), "ln"))
    L = g.case.L
    assert L.nw >= 16 * cus + 17
    runs, G = _all_cuts(g)
    assert G == cus
    _same_bits("grid = CUs", L, runs)
    g.check(runs["search"][1], "ws grid=CUs n=%d nw=%d" % (L.n, L.nw))


# ---- compress_ws.hip: input classes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls", [pytest.param(n_, c_, id="%s-%s" % (n_, c_)) for n_ in CLASS_LEVELS for c_ in CLASSES])
def test_ws_input_classes(name, cls):
    g = _structural(name, cls)
    L = g.case.L
    what = "ws %s" % name
    if cls in TOP_CLASSES:
        check_top(g.case, g.stats)
    if cls == "edge100":
        if name != "unlisted":  # (module docstring)
            print("edge100 %s: fraction over the limit %.2f, plain->merge %d, merge->plain %d" % ((name,) + check_edge100(g.case)))
        G = int(g.lib.mssvt_compress_ws_groups(max(L.n, 1)))
        st, out = g.ws(ends=ends_from_cuts(L, G, []))
    else:
        st, out = g.ws()
    assert st == 0
    g.check(out, what)
    if cls == "negative":  # the zero padding decides: partial windows have a query token >= 0, full ones need not
        assert bool((L.win_cnt < L.ns).any())


# ---- compress_ws.hip: no work, the pack, declined calls ------------------------------------------------------------------------
def test_ws_no_windows_and_no_rows_write_nothing():
    g = _structural("mixed16")
    st, out = g.ws(num_wins=0)
    assert st == 0 and bool((out == SENTINEL).all())
    st, out = g.ws(n=0)
    assert st == 0 and bool((out == SENTINEL).all())


def test_ws_pack_is_deterministic_and_stays_inside_its_bytes():
    from mssvt_amd import _lib
    g = _structural("mixed16")
    nbytes = int(g.lib.mssvt_compress_ws_packed_bytes(128))
    assert nbytes == 5 * 8 * 4 * 2 * 64 * 16 == 5 * 128 * 128 * 2 * 2  # hi + lo halves of five C x C matrices
    bufs = []
    for fill in (0x5A, 0xA5):
        b = torch.full((nbytes + 4096,), fill, dtype=torch.uint8, device=DEV)
        assert g.lib.mssvt_compress_ws_pack(128, g.Wp2.data_ptr(), g.Wq.data_ptr(), g.Wkv.data_ptr(), g.Wo.data_ptr(),
                                            b.data_ptr(), _lib.stream()) == 0
        torch.cuda.synchronize()
        assert bool((b[nbytes:] == fill).all()), "guard bytes behind the fragments were written"
        bufs.append(b[:nbytes])
    assert torch.equal(bufs[0], bufs[1])  # every byte written (two different fills), the same bytes
    assert torch.equal(bufs[0], g.packed())
    assert int(g.lib.mssvt_compress_ws_packed_bytes(64)) == 0
    junk = torch.full((64,), 7, dtype=torch.uint8, device=DEV)
    assert g.lib.mssvt_compress_ws_pack(64, g.Wp2.data_ptr(), g.Wq.data_ptr(), g.Wkv.data_ptr(), g.Wo.data_ptr(), junk.data_ptr(),
                                        _lib.stream()) == E_TOOLARGE
    assert g.lib.mssvt_compress_ws_pack(128, None, g.Wq.data_ptr(), g.Wkv.data_ptr(), g.Wo.data_ptr(), junk.data_ptr(),
                                        _lib.stream()) == E_BADARG
    torch.cuda.synchronize()
    assert bool((junk == 7).all())


def test_ws_declined_calls_launch_nothing():
    g = _structural("mixed16")
    L = g.case.L
    G = int(g.lib.mssvt_compress_ws_groups(max(L.n, 1)))
    ends = ends_from_cuts(L, G, [])
    table = [(dict(C=64), E_TOOLARGE), (dict(head_dim=32), E_TOOLARGE), (dict(ns=33, z_ws=16), E_TOOLARGE),
             (dict(z_ws=17, ns=16), E_TOOLARGE), (dict(chunk_groups=G + 1), E_BADARG), (dict(chunk_groups=G - 1), E_BADARG)]
    table += [(dict(null=k), E_BADARG) for k in ("num_wins", "indices", "win_cnt", "pair_win", "vs", "mn", "ws", "xhat", "Wp1", "bp1",
                                                 "bp2", "bq", "bkv", "bo", "packed")]
    for over, want in table:
        st, out = g.ws(ends=ends if "chunk_groups" in over else None, **over)
        assert st == want, (over, st)
        assert bool((out == SENTINEL).all()), over
    from mssvt_amd import _lib
    st = g.lib.mssvt_compress_ws(128, 16, g.case.scale, L.z_ws, L.ns, L.n, g.num_wins.data_ptr(), L.n, g.indices.data_ptr(),
                                 g.win_cnt.data_ptr(), g.pair_win.data_ptr(), g.vs3, g.mn3, g.ws3, g.xhat.data_ptr(), g.Wp1.data_ptr(),
                                 g.bp1.data_ptr(), g.bp2.data_ptr(), g.bq.data_ptr(), g.bkv.data_ptr(), g.bo.data_ptr(),
                                 g.packed().data_ptr(), None, _lib.stream())
    assert st == E_BADARG  # out = NULL


# ---- compress_fused.hip ----------------------------------------------------------------------------------------------------------
FUSED_NW = (1, 15, 16, 17, 33)


def _fused_case(C, hd, nw, cls="ln", ns=12, long_list=0):
    return on_gpu(("fused", C, hd, nw, cls, ns, long_list),
                  lambda: make_case(fused_level(nw, ns, 500 + nw + ns, long_list), cls, C, hd))


def _fused_ids():
    return [pytest.param(C, hd, sp, nw, id="%dx%d-%s-nw%d" % (C, hd, "split" if sp else "f32", nw))
            for C, hd in FUSED_SHAPES for nw in FUSED_NW for sp in (0, 1)]


def _check_fused(g, split, what, capacity=None):
    L = g.case.L
    st, out, scratch = g.fused(split, capacity)
    assert st == 0, (what, st)
    g.check(out, what, split=bool(split))
    unlisted = torch.from_numpy(L.pair_win[:L.n] < 0).to(DEV)
    assert bool(torch.isnan(scratch[2][:L.n][unlisted]).all())  # scores of rows in no list are never written
    for t, rows in zip(scratch, (L.nw, L.n, L.n, L.n)):
        assert bool(torch.isnan(t[rows:]).all()), (what, "scratch rows behind the level were written")
    return out


@pytest.mark.parametrize("C,hd,split,nw", _fused_ids())
def test_fused_every_form_vs_float64(C, hd, split, nw):
    g = _fused_case(C, hd, nw)
    L = g.case.L
    assert L.n % 16 != 0 and ((L.win_cnt == 0).sum() == 1) == (nw >= 15)
    _check_fused(g, split, "fused %dx%d %s nw=%d n=%d" % (C, hd, "split" if split else "f32", nw, L.n))


@pytest.mark.parametrize("C,hd", [(128, 16), (64, 8), (32, 32)], ids=lambda v: str(v))
@pytest.mark.parametrize("split", (0, 1), ids=("f32", "split"))
@pytest.mark.parametrize("regime", ("w<v", "w==v", "w>v"))
def test_fused_grid_regimes(C, hd, split, regime):
    """The roles of k_cmp_query_keys: fewer, as many, and more query workgroups than key workgroups (the last by a large
    win_capacity over a small n: the `query_blocks > key_blocks` branch of the role mapping)."""
    g = _fused_case(C, hd, 33)
    L, cus = g.case.L, _cus()
    vt = (L.n + 15) // 16
    cap = {"w<v": 33, "w==v": 16 * vt, "w>v": 16 * (vt + 9)}[regime]
    g_w, g_v = fused_grids(C, L.ns, L.n, cap, split, cus)
    assert {"w<v": g_w < g_v, "w==v": g_w == g_v, "w>v": g_w > g_v}[regime], (g_w, g_v)
    assert cap >= L.nw and vt > 3
    _check_fused(g, split, "fused %dx%d %s grid %s (%d, %d)" % (C, hd, "split" if split else "f32", regime, g_w, g_v), capacity=cap)


@pytest.mark.parametrize("split,cls", [pytest.param(sp, c_, id="%s-%s" % ("split" if sp else "f32", c_))
                                       for sp in (0, 1) for c_ in CLASSES if c_ != "edge100" and (sp or c_ not in TOP_CLASSES)])
@pytest.mark.parametrize("C,hd", [(128, 16), (64, 8)], ids=lambda v: str(v))
def test_fused_input_classes(C, hd, split, cls):
    g = _fused_case(C, hd, 33, cls)
    if cls in TOP_CLASSES:
        check_top(g.case, g.stats)
    _check_fused(g, split, "fused %dx%d %s" % (C, hd, "split" if split else "f32"))


@pytest.mark.parametrize("C", (128, 64, 32))
@pytest.mark.parametrize("split", (0, 1), ids=("f32", "split"))
def test_fused_list_capacity_at_the_lds_limit(C, split):
    """ns at the largest value launch_compress's LDS formula admits (93 / 142 / 155), one list that long; one above it is
    MSSVT_E_TOOLARGE and writes nothing."""
    ns = fused_ns_limit(C)
    assert ns == {128: 93, 64: 142, 32: 155}[C]
    assert max(fused_lds(C, ns)) <= LDS_BYTES < max(fused_lds(C, ns + 1))
    g = _fused_case(C, 16, 17, ns=ns, long_list=ns)
    assert int(g.case.L.win_cnt.max()) == ns
    _check_fused(g, split, "fused %dx16 %s ns=%d" % (C, "split" if split else "f32", ns))
    h = OnGpu(make_case(fused_level(17, ns + 1, 3), "ln", C, 16))
    st, out, scratch = h.fused(split)
    assert st == E_TOOLARGE
    assert bool((out == SENTINEL).all()) and all(bool(torch.isnan(t).all()) for t in scratch)


def test_fused_declined_calls_launch_nothing():
    g = _fused_case(32, 8, 17)
    c = g.case
    for C, hd, want in ((48, 16, E_TOOLARGE), (128, 8, E_TOOLARGE), (64, 24, E_BADARG)):
        c.C, c.hd, keep = C, hd, (c.C, c.hd)
        try:
            st, out, scratch = g.fused(1)
        finally:
            c.C, c.hd = keep
        assert st == want, (C, hd, st)
        assert bool((out == SENTINEL).all()) and all(bool(torch.isnan(t).all()) for t in scratch)


@pytest.mark.parametrize("name", STRUCTURAL)
def test_fused_agrees_with_ws(name):
    """Both files on the same level: each within its bound of float64, and of each other within the sum of the bounds."""
    g = _structural(name)
    L = g.case.L
    st, a = g.ws()
    assert st == 0
    b = _check_fused(g, 1, "fused on ws level %s" % name, capacity=max(L.n, 1))
    e32 = g.e32()
    d = (a[:L.nw].double() - b[:L.nw].double()).abs() / row_scale(g.want)
    bound = 2 * (TIGHT_RATIO * float(e32.max()) + 1e-6)
    print("RATIO ws-vs-fused %s max/bound=%.3f" % (name, float(d.max()) / bound))
    assert float(d.max()) <= bound
