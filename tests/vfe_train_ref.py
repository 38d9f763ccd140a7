"""A numpy float64 statement of the operators of mssvt_amd/vfe_train.py (csrc/vfe_train.hip) -- grouping, feature augmentation,
run_max_concat and run_max with their backward and the tie rule -- and the hand-built cases the CPU and GPU tests share.

The tie rule: the rows of a run that EQUAL its maximum (numpy ``==``: -0.0 == +0.0) share the maximum's gradient equally
(``scatter_reduce("amax")`` of the torch branch, and oracle/gen_golden_vfe.py's restatement of torch_scatter).  An empty run
has a zero maximum and passes no gradient.  Non-finite inputs are not covered.

tests/test_vfe_train_ref_cpu.py holds this statement to torch autograd in float64."""
import numpy as np

# the kernels' piece size (MSSVT_VFE_TRAIN_CHUNK; tests/test_vfe_train_fused_cpu.py holds this copy to the header): stated here, not
# imported, so that the cases do not move with the code under test
CHUNK = 128


def group(point_voxel, num_voxels):
    """order (P',) and run_off (N + 1,): the kept points sorted by voxel, ascending point index inside a voxel."""
    pv = np.asarray(point_voxel)
    kept = np.flatnonzero((pv >= 0) & (pv < num_voxels))
    order = kept[np.argsort(pv[kept], kind="stable")]
    counts = np.bincount(pv[kept], minlength=num_voxels)[:num_voxels] if num_voxels else np.zeros(0, np.int64)
    run_off = np.concatenate(([0], np.cumsum(counts)))
    return order.astype(np.int32), run_off.astype(np.int32)


def augment(points, order, run_off, voxel_coords, voxel_size, offset, npf, cluster=True, centre=True, distance=False):
    """(P', C) float64: [features, xyz - mean of the run's xyz, xyz - (cell * voxel_size + offset), |xyz|]; voxel_size and
    offset are taken as the float32 values the device gets."""
    rows = np.asarray(points, np.float64)[order]
    xyz = rows[:, 1:4]
    N = len(run_off) - 1
    row_voxel = np.repeat(np.arange(N), np.diff(run_off))
    cols = [rows[:, 1:1 + npf]]
    if cluster:
        mean = np.zeros((N, 3))
        for v in range(N):
            if run_off[v + 1] > run_off[v]:
                mean[v] = xyz[run_off[v]:run_off[v + 1]].mean(axis=0)
        cols.append(xyz - mean[row_voxel])
    if centre:
        vs = np.asarray(voxel_size, np.float32).astype(np.float64)
        off = np.asarray(offset, np.float32).astype(np.float64)
        cell = np.asarray(voxel_coords)[row_voxel][:, [3, 2, 1]].astype(np.float64)
        cols.append(xyz - (cell * vs + off))
    if distance:
        cols.append(np.sqrt((xyz * xyz).sum(axis=1, keepdims=True)))
    return np.concatenate(cols, axis=1)


def run_max(x, run_off):
    x = np.asarray(x, np.float64)
    N = len(run_off) - 1
    out = np.zeros((N, x.shape[1]))
    for v in range(N):
        s, e = run_off[v], run_off[v + 1]
        if e > s:
            out[v] = x[s:e].max(axis=0)
    return out


def run_max_concat(x, run_off):
    x = np.asarray(x, np.float64)
    row_voxel = np.repeat(np.arange(len(run_off) - 1), np.diff(run_off))
    return np.concatenate((x, run_max(x, run_off)[row_voxel]), axis=1)


def _share(x, run_off, gm):
    """gm (N, F), the gradient of every run's maximum -> its part in every row (P', F), and the tie counts (N, F)"""
    x = np.asarray(x, np.float64)
    N = len(run_off) - 1
    out = np.zeros_like(x)
    cnt = np.zeros((N, x.shape[1]), np.int64)
    for v in range(N):
        s, e = run_off[v], run_off[v + 1]
        if e > s:
            hit = x[s:e] == x[s:e].max(axis=0)
            cnt[v] = hit.sum(axis=0)
            out[s:e] = hit * (gm[v] / cnt[v])
    return out, cnt


def run_max_backward(x, run_off, g):
    """gx (P', F) and the bound of a float32 evaluation: the element is one term divided by the tie count."""
    gx, _ = _share(x, run_off, np.asarray(g, np.float64))
    return gx, 2.0 ** -23 * np.abs(gx)


def run_max_concat_backward(x, run_off, g):
    """gx (P', F) = g[:, :F] + share(sum over the run of g[:, F:]), and the bound of a float32 evaluation: an element that
    attains the maximum is a sum of n = L + 1 float32 terms t (its own gradient and the L rows' g[:, F:] / count): (n - 1)
    2^-24 sum|t| + 2^-23 |value| for the division; any other element is g[:, :F] itself, passed through: bound 0."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    F = x.shape[1]
    N = len(run_off) - 1
    gm, ga = np.zeros((N, F)), np.zeros((N, F))
    for v in range(N):
        s, e = run_off[v], run_off[v + 1]
        gm[v], ga[v] = g[s:e, F:].sum(axis=0), np.abs(g[s:e, F:]).sum(axis=0)
    share, cnt = _share(x, run_off, gm)
    gx = g[:, :F] + share
    L = np.repeat(np.diff(run_off), np.diff(run_off))[:, None]
    row_voxel = np.repeat(np.arange(N), np.diff(run_off))
    sum_abs = np.abs(g[:, :F]) + ga[row_voxel] / np.maximum(cnt[row_voxel], 1)
    hit = np.asarray(x == run_max(x, run_off)[row_voxel])
    bound = np.where(hit, L * 2.0 ** -24 * sum_abs + 2.0 ** -23 * np.abs(gx), 0.0)
    return gx, bound


# ---------------------------------------------------------------------------------------------------------------- cases

# run lengths mixed in one table: an empty run first, last and inside; both sides of the 16- and 64-row marks and of the
# piece size; two long runs side by side (one row window then meets two of them); one run of 1 000
MIXED = [0, 1, 2, 3, 15, 16, 17, 0, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 2, 1000, 1, 0]
TABLES = {"mixed": MIXED, "single_short": [5], "single_long": [2 * CHUNK + 44], "ones": [1] * 70}
WIDTHS = {"mixed": (4, 20, 32, 64, 128, 256), "single_short": (20, 64), "single_long": (20, 64), "ones": (4, 64)}
CASES = sorted((t, F) for t in TABLES for F in WIDTHS[t])

_CACHE = {}


def make_case(table, F):
    """x (P', F) float32, run_off, the upstream gradients of run_max_concat (P', 2F) and run_max (N, F) -- float32 values with
    the planted rows below -- built once and left unchanged."""
    key = (table, F)
    if key in _CACHE:
        return _CACHE[key]
    lengths = TABLES[table]
    rng = np.random.default_rng(1000 * len(lengths) + F)
    run_off = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    rows, N = int(run_off[-1]), len(lengths)
    x = rng.standard_normal((rows, F)).astype(np.float32)
    planted = []
    for v in range(N):
        s, e = int(run_off[v]), int(run_off[v + 1])
        L = e - s
        kind = v % 6
        if L >= 2 and kind == 0:      # a two-way tie in every channel: two equal rows above the rest
            x[s] = np.abs(x[s]) + 10
            x[s + L // 2] = x[s]
            planted.append(("tie2", v))
        elif L >= 3 and kind == 1:    # a three-way tie, its rows spread over the run (over the pieces of a long one)
            x[e - 1] = np.abs(x[e - 1]) + 10
            x[s] = x[s + L // 2] = x[e - 1]
            planted.append(("tie3", v))
        elif L >= 2 and kind == 2:    # all negative: the maximum is negative, not zero
            x[s:e] = -np.abs(x[s:e]) - 1
            planted.append(("negative", v))
        elif L >= 2 and kind == 3:    # after a ReLU: a column that is zero across the run, and one of mixed signed zeros
            x[s:e] = np.maximum(x[s:e], 0)
            x[s:e, 0] = 0.0
            x[s:e, F - 1] = np.where(np.arange(L) % 2 == 0, 0.0, -0.0)
            planted.append(("zeros", v))
        elif L >= 2 and kind == 4:    # huge magnitudes of both signs; a column whose maximum is -1e30
            x[s, 1] = 1e30
            x[e - 1, 2] = -1e30
            x[s:e, 3] = -1e30
            planted.append(("huge", v))
    g_cat = rng.standard_normal((rows, 2 * F)).astype(np.float32)
    g_max = rng.standard_normal((N, F)).astype(np.float32)
    if rows:
        g_cat[rows // 2, F:] = 1e30  # a gradient sum that carries a huge term
        g_cat[rows // 3, :F] = -1e30
    c = dict(x=x, run_off=run_off, g_cat=g_cat, g_max=g_max, planted=planted, lengths=lengths, F=F)
    c["cat"] = run_max_concat(x, run_off)
    c["max"] = run_max(x, run_off)
    c["gx_cat"], c["bound_cat"] = run_max_concat_backward(x, run_off, g_cat)
    c["gx_max"], c["bound_max"] = run_max_backward(x, run_off, g_max)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[key] = c
    return c


def grouping_cases():
    """point_voxel (with -1 entries), num_voxels"""
    rng = np.random.default_rng(7)
    mixed = rng.integers(-1, 40, size=3000).astype(np.int32)
    mixed[mixed == 17] = 16  # id 17: no point carries it
    mixed[mixed == 39] = 38  # nor the last id
    one = np.full(700, 0, np.int32)
    one[::9] = -1
    return {"mixed": (mixed, 40), "one_voxel": (one, 1), "all_outside": (np.full(50, -1, np.int32), 3),
            "single_point": (np.array([0], np.int32), 1),
            "large": (rng.integers(-1, 50000, size=70000).astype(np.int32), 50000)}
