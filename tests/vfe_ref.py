"""Float64 statements of DynamicVFE's inference kernels (csrc/voxelize.hip, csrc/vfe.hip, csrc/pfn_fused.hip,
csrc/pfn_sorted.hip), with a bound for every element.  CPU, numpy (torch only inside train_matrix_ref.linear_h_bound).

    cell     = floor((xyz - range_min) / voxel_size)                     keep 0 <= cell < grid, 0 <= b < B
    key      = ((b X + cx) Y + cy) Z + cz;  voxels = sorted unique keys;  voxel_coords = [b, cz, cy, cx]
    mean3    = per-voxel mean of xyz (the cluster centre)
    f        = [x, y, z, f4, f5,  xyz - mean3[voxel],  xyz - (coord * voxel_size + offset)]                 (rows, 11)
    x1       = relu(bn1(W1 f + b1));      m1  = max over the voxel's rows of x1                              (rows, 64) / (N, 64)
    x2       = relu(bn2(W2 [x1 ; m1[voxel]] + b2));     out = max over the voxel's rows of x2                (N, 128)
    bn(z)    = (z - mean) / sqrt(var + eps) * weight + bias

EXACT parts (no bound: the kernels must return these bits).
  Cells: the reference's own float32 expression, every operation rounded once; numpy float32 gives the same bits (IEEE
  subtract and divide, floor exact).  Keep test, key order, coordinates and the point -> voxel map follow from it in integers.
  Cluster centre: the kernels add rint(float64(x) 2^20) as 64-bit integers (any order gives the same sum) and return
  float32(float64(sum) / 2^20 / n): two float64 operations, of which the first is exact, and one conversion.  Stated as is.
  The eleven inputs: float32, one rounding per operation, the voxel centre as float32(float32(coord * vs) + off).

BOUNDED parts.  U = 2^-24; every bound comes from the float64 magnitudes of the element's OWN terms; none looks at a
kernel's result.  The inputs f are exact, so layer 1 starts without an input error.

  chain(K, mag): a chain of K fused multiply-adds from 0 and one bias add rounds K + 1 partial sums, each at most mag =
  |b| + sum |f W| in magnitude: (K + 1) U mag to first order; (K + 2) U mag with the second-order terms.

  bn(ez, z): with t = z - mean, A = |weight| / sqrt(var + eps), in torch's operation order (t * invstd * weight + bias):
      error of z carried through:                 A ez
      t rounded, invstd off by at most 3 U of itself (the add var + eps U, halved by the square root; the square root and
      the division are correctly rounded: U each), two products and one add rounded:   (1 + 3 + 2) U A |t| + U (A |t| + |bias|)
  bound = A ez + 8 U A |t| + 2 U |bias| + 2^-140 (7 roundings, the eighth U and the second U of |bias| pay for the second
  order; 2^-140 for results below the normal range, where a rounding is absolute: at most 2^-150 each).
  ANY-ORDER form (a library may fold the transform into z * alpha + beta, alpha = invstd * weight, beta = bias - mean * alpha,
  which rounds |z| A and |mean| A instead of |z - mean| A): the same expression with |z| + |mean| in place of |t|.

  relu and max are exact and 1-Lipschitz: b_x1 = bn bound of the row, b_m1[v] = max over the voxel's rows of b_x1.

  Layer 2 on split-fp16 operands: train_matrix_ref.linear_h_bound (K = 128: (K + 40) U mag + 2^-35 (2^ex sum |W| + 2^ew sum |x|),
  with the row's and the matrix's own powers of two), evaluated at |x| + b_x: the kernel's row is the statement's row off by
  at most b_x = [b_x1 ; b_m1[voxel]], so every magnitude and the row's power of two are taken at their upper ends; plus the
  input error itself through the matrix, |W2| b_x.  That is ez of layer 2's bn bound; b_out[v] = max over the voxel's rows.
  Any-order fp32 form: train_matrix_ref.linear_bound (K + 4) U mag in place of linear_h_bound.

  Input slack of another cluster centre (only for comparing with a float mean, as the reference's scatter_mean): the fixed
  point sum is off by at most 2^-21 per point (exact for |x| >= 8: the float's spacing is 2^-20 or more), so the two means
  differ by at most 2^-21 + 2 U |mean| and f[5..7] by that plus U |f| (its own rounding): carried through |W1[:, 5:8]|.
"""
import numpy as np
import torch

from tests.train_matrix_ref import U32, linear_bound, linear_h_bound

F32, F64 = np.float32, np.float64
FIX = 1048576.0
TINY = 2.0 ** -140


# ---------------------------------------------------------------------------------------------------------
# exact parts
# ---------------------------------------------------------------------------------------------------------

def cells(points, range_min, voxel_size, grid, batch_size):
    """(keep (P) bool, cell (P, 3) int64 [cx, cy, cz], key (P) int64; -1 where not kept)."""
    p = np.asarray(points, F32)
    lo, vs = np.asarray(range_min, F32), np.asarray(voxel_size, F32)
    g = np.asarray(grid, np.int64)
    with np.errstate(all="ignore"):
        fl = np.floor((p[:, 1:4] - lo) / vs)  # float32 throughout
    keep = ((fl >= 0) & (fl < g.astype(F32))).all(1)  # (NaN compares false)
    b = p[:, 0].astype(np.int64)  # C truncation
    keep &= (b >= 0) & (b < batch_size)
    c = np.where(keep[:, None], fl, 0).astype(np.int64)
    key = ((b * g[0] + c[:, 0]) * g[1] + c[:, 1]) * g[2] + c[:, 2]
    return keep, c, np.where(keep, key, -1)


def voxelize(points, range_min, voxel_size, grid, batch_size):
    """(voxel_coords (N, 4) int32 [b, z, y, x] sorted by key, point_voxel (P) int32 with -1 outside)."""
    keep, _, key = cells(points, range_min, voxel_size, grid, batch_size)
    unq, inv = np.unique(key[keep], return_inverse=True)
    pv = np.full(len(key), -1, np.int32)
    pv[keep] = inv.astype(np.int32)
    X, Y, Z = (int(v) for v in grid)
    coords = np.stack([unq // (X * Y * Z), unq % Z, (unq // Z) % Y, (unq // (Y * Z)) % X], 1).astype(np.int32)
    return coords, pv


def cluster_centre(xyz, voxel, n_voxels):
    """(mean3 (N, 3) float32, count (N) int64): the kernels' exact fixed-point mean; empty voxels 0."""
    fx = np.rint(np.asarray(xyz, F32).astype(F64) * FIX).astype(np.int64)
    s = np.zeros((n_voxels, 3), np.int64)
    np.add.at(s, voxel, fx)
    cnt = np.bincount(voxel, minlength=n_voxels).astype(np.int64)
    with np.errstate(all="ignore"):
        mean = (s.astype(F64) / FIX / cnt[:, None].astype(F64)).astype(F32)
    return np.where(cnt[:, None] > 0, mean, F32(0)), cnt


def pfn_inputs(pts, voxel, mean3, coords, voxel_size, offset):
    """f (rows, 11) float32 exactly as the kernels build it.  pts rows [b, x, y, z, f4, f5]."""
    pts = np.asarray(pts, F32)
    vs, off = np.asarray(voxel_size, F32), np.asarray(offset, F32)
    xyz = pts[:, 1:4]
    centre = coords[voxel][:, [3, 2, 1]].astype(F32) * vs + off  # two float32 roundings
    return np.concatenate([pts[:, 1:6], xyz - mean3[voxel], xyz - centre], 1).astype(F32)


# ---------------------------------------------------------------------------------------------------------
# bounded parts
# ---------------------------------------------------------------------------------------------------------

def _bn(z, ez, prm, i, any_order):
    g, h, mu = (prm["%s%d" % (k, i)].astype(F64) for k in ("g", "h", "mu"))
    var_eps = prm["var%d" % i].astype(F64) + float(F32(prm["eps%d" % i]))  # (eps as the float the kernels are handed)
    inv = 1.0 / np.sqrt(var_eps)
    t = z - mu
    y = t * inv * g + h
    A = np.abs(inv * g)
    size = np.abs(z) + np.abs(mu) if any_order else np.abs(t)
    return y, A * ez + 8 * U32 * A * size + 2 * U32 * np.abs(h) + TINY


def _group_max(x, voxel, n):
    out = np.full((n, x.shape[1]), -np.inf, F64)
    np.maximum.at(out, voxel, x)
    return out


def pfn_statement(pts, voxel, n_voxels, coords, voxel_size, offset, prm, mean3=None, any_order=False, centre_slack=False):
    """The PFN statement for points `pts` (rows [b, x, y, z, f4, f5], all inside the grid) of voxels [0, n_voxels): `voxel`
    (rows) int.  A voxel's features depend only on its own points, so any subset of voxels (renumbered, with ALL their
    points) may be passed.  prm: float32 arrays W1 (64, 11), b1, g1, h1, mu1, var1, W2 (128, 128), b2, g2, h2, mu2, var2 and
    floats eps1, eps2.  mean3: the cluster centres to use (default: the exact fixed-point ones).
    Returns a dict: mean3, f (float32); x1, m1, out (float64) and their bounds b_x1, b_m1, b_out."""
    voxel = np.asarray(voxel, np.int64)
    if mean3 is None:
        mean3, _ = cluster_centre(np.asarray(pts, F32)[:, 1:4], voxel, n_voxels)
    f = pfn_inputs(pts, voxel, mean3, coords, voxel_size, offset)
    f64 = f.astype(F64)
    W1 = prm["W1"].astype(F64)
    z1 = f64 @ W1.T + prm["b1"].astype(F64)
    mag1 = np.abs(f64) @ np.abs(W1).T + np.abs(prm["b1"].astype(F64))
    ez1 = (11 + 4) * U32 * mag1 if any_order else (11 + 2) * U32 * mag1
    if centre_slack:
        ef = 2.0 ** -21 + 2 * U32 * np.abs(mean3[voxel].astype(F64)) + U32 * np.abs(f64[:, 5:8])
        ez1 = ez1 + ef @ np.abs(W1[:, 5:8]).T
    y1, b_x1 = _bn(z1, ez1, prm, 1, any_order)
    x1 = np.maximum(y1, 0.0)
    m1, b_m1 = _group_max(x1, voxel, n_voxels), _group_max(b_x1, voxel, n_voxels)
    if "W2" not in prm:  # a one-layer VFE: m1 is its output
        return dict(mean3=mean3, f=f, x1=x1, b_x1=b_x1, m1=m1, b_m1=b_m1)
    W2 = prm["W2"].astype(F64)
    row = np.concatenate([x1, m1[voxel]], 1)
    b_row = np.concatenate([b_x1, b_m1[voxel]], 1)
    up = np.abs(row) + b_row
    z2 = row @ W2.T + prm["b2"].astype(F64)
    mag2 = up @ np.abs(W2).T + np.abs(prm["b2"].astype(F64))
    if any_order:
        e_lin = linear_bound(128, mag2, 1.0)
    else:
        e_lin = linear_h_bound(torch.from_numpy(up), torch.from_numpy(prm["W2"]), 0, torch.from_numpy(mag2), 1.0).numpy()
    ez2 = e_lin + b_row @ np.abs(W2).T
    y2, b_x2 = _bn(z2, ez2, prm, 2, any_order)
    x2 = np.maximum(y2, 0.0)
    return dict(mean3=mean3, f=f, x1=x1, b_x1=b_x1, m1=m1, b_m1=b_m1, x2=x2, b_x2=b_x2,
                out=_group_max(x2, voxel, n_voxels), b_out=_group_max(b_x2, voxel, n_voxels))


def params_from_state_dict(sd, eps):
    """prm of `pfn_statement` from a DynamicVFE state dict (numpy arrays), one or two layers."""
    prm = {}
    for i in (1, 2):
        p = "pfn.%d." % (i - 1)
        if p + "0.weight" not in sd:
            break
        prm.update({"W%d" % i: sd[p + "0.weight"], "b%d" % i: sd[p + "0.bias"], "g%d" % i: sd[p + "1.weight"], "h%d" % i: sd[p + "1.bias"],
                    "mu%d" % i: sd[p + "1.running_mean"], "var%d" % i: sd[p + "1.running_var"], "eps%d" % i: float(eps)})
    return {k: (np.asarray(v, F32) if not k.startswith("eps") else v) for k, v in prm.items()}


def subset(point_voxel, voxels):
    """(rows, local): the points of the given voxels (ascending ids) and their index into `voxels`."""
    voxels = np.asarray(voxels, np.int64)
    pv = np.asarray(point_voxel, np.int64)
    at = np.searchsorted(voxels, pv)
    hit = (pv >= 0) & (at < len(voxels))
    hit[hit] = voxels[at[hit]] == pv[hit]
    rows = np.nonzero(hit)[0]
    return rows, at[rows]


def voxel_max(feat, voxel, n_voxels):
    """scatter_max(feat, voxel)[0] with -inf for empty voxels; rows with voxel < 0 skipped.  -0.0 < +0.0 (the order of the
    sign-magnitude bits, which is what an integer view compares)."""
    feat = np.asarray(feat, F32)
    keep = np.asarray(voxel) >= 0
    out = np.full((n_voxels, feat.shape[1]), -np.inf, F32)
    np.maximum.at(out, np.asarray(voxel)[keep], feat[keep])
    # np.maximum may return either zero for (-0.0, +0.0): a column holds +0.0 iff one of its values is +0.0
    pz = np.zeros((n_voxels, feat.shape[1]), bool)
    np.logical_or.at(pz, np.asarray(voxel)[keep], (feat[keep] == 0) & ~np.signbit(feat[keep]))
    zero = out == 0
    return np.where(zero & pz, F32(0.0), np.where(zero, F32(-0.0), out))


# ---------------------------------------------------------------------------------------------------------
# a float32 evaluation in kernel order, the split-fp16 halves emulated by truncation
# ---------------------------------------------------------------------------------------------------------

def _pow2_norm(m):
    bits = np.asarray(m, F32).view(np.int32).astype(np.int64)
    eb = bits & 0x7F800000
    norm = (eb != 0) & (eb <= 0x7F000000)
    sb = np.maximum(0x7F000000 - eb, 0x00800000)
    s_in = np.where(norm, sb.astype(np.int32).view(F32), F32(1))
    un = np.where(norm, (0x7F000000 - sb).astype(np.int32).view(F32), F32(1))
    return s_in.astype(F32), un.astype(F32)


def _rtz16(v):
    """float32 -> fp16 toward zero, as float32."""
    h = np.asarray(v, F32).astype(np.float16)
    over = np.abs(h.astype(F32)) > np.abs(v)
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(F32)


def _split(v):
    hi = _rtz16(v)
    lo = _rtz16((v - hi) * F32(2048))  # exact before the conversion
    return hi.astype(F64), lo.astype(F64)


def _bn32(z, prm, i):
    inv = (F32(1) / np.sqrt(prm["var%d" % i] + F32(prm["eps%d" % i]))).astype(F32)
    return np.maximum((z - prm["mu%d" % i]) * inv * prm["g%d" % i] + prm["h%d" % i], F32(0)).astype(F32)


def pfn_emulated(pts, voxel, n_voxels, coords, voxel_size, offset, prm):
    """(x1 (rows, 64), m1 (N, 64), out (N, 128)) float32 as the kernels' arithmetic gives them: layer 1 as a chain of 11 fused
    multiply-adds (a float64 product and add rounded to float32: the product is exact there), layer 2 per 32-column step on
    truncated hi / lo halves with float32 accumulators (the order inside a step is not modelled: summed exactly, rounded once)."""
    voxel = np.asarray(voxel, np.int64)
    mean3, _ = cluster_centre(np.asarray(pts, F32)[:, 1:4], voxel, n_voxels)
    f = pfn_inputs(pts, voxel, mean3, coords, voxel_size, offset)
    acc = np.zeros((f.shape[0], 64), F32)
    for k in range(11):
        acc = (f[:, k:k + 1].astype(F64) * prm["W1"][:, k].astype(F64)[None] + acc.astype(F64)).astype(F32)
    x1 = _bn32(acc + prm["b1"], prm, 1)
    m1 = np.full((n_voxels, 64), -np.inf, F32)
    np.maximum.at(m1, voxel, x1)
    row = np.concatenate([x1, m1[voxel]], 1)
    s_in, s_un = _pow2_norm(np.abs(row).max(1))
    w_in, w_un = _pow2_norm(np.abs(prm["W2"]).max())
    ah, al = _split(row * s_in[:, None])
    bh, bl = _split(prm["W2"] * w_in)
    mm, cr = np.zeros((row.shape[0], 128), F32), np.zeros((row.shape[0], 128), F32)
    for k0 in range(0, 128, 32):
        k = slice(k0, k0 + 32)
        mm = (mm.astype(F64) + ah[:, k] @ bh[:, k].T).astype(F32)
        t = (cr.astype(F64) + al[:, k] @ bh[:, k].T).astype(F32)
        cr = (t.astype(F64) + ah[:, k] @ bl[:, k].T).astype(F32)
    r = (cr.astype(F64) * 2.0 ** -11 + mm.astype(F64)).astype(F32) * (s_un * w_un)[:, None]
    x2 = _bn32(r + prm["b2"], prm, 2)
    out = np.full((n_voxels, 128), -np.inf, F32)
    np.maximum.at(out, voxel, x2)
    return x1, m1, out


# ---------------------------------------------------------------------------------------------------------
# operand families and hand-built run layouts
# ---------------------------------------------------------------------------------------------------------

FAMILIES = ("unit", "big", "small", "signed", "int")
# the integer family's geometry (`layout_points(..., dyadic=True)`): dyadic voxel size, range minimum and offset, coordinates
# within +-8 so that every sum of the statement stays below 2^24 sixteenths
DY_VS, DY_MIN, DY_GRID = [0.25, 0.25, 0.5], [-8.0, -8.0, -2.0], [64, 64, 8]
DY_OFF = [DY_VS[k] / 2 + DY_MIN[k] for k in range(3)]


def params(kind, seed):
    """Layer parameters of one operand family.  "unit": random at unit scale; "big" / "small": layer 1's BatchNorm scaled so
    that x1 is about 2^30 / 2^-30; "signed": negative and zero BatchNorm weights; "int": small integer weights, var = 1,
    eps = 0 (with `layout_points(..., dyadic=True)` every sum is exact)."""
    rng = np.random.default_rng(seed)
    if kind == "int":
        p = dict(W1=rng.integers(-2, 3, (64, 11)), b1=rng.integers(-3, 4, 64), g1=rng.integers(-2, 3, 64), h1=rng.integers(-2, 3, 64),
                 mu1=rng.integers(-2, 3, 64), var1=np.ones(64), eps1=0.0,
                 W2=rng.integers(-2, 3, (128, 128)) * (rng.random((128, 128)) < 0.25), b2=rng.integers(-3, 4, 128),
                 g2=rng.integers(-2, 3, 128), h2=rng.integers(-2, 3, 128), mu2=rng.integers(-2, 3, 128), var2=np.ones(128), eps2=0.0)
    else:
        p = dict(W1=rng.standard_normal((64, 11)) / 11 ** 0.5, b1=rng.standard_normal(64) * 0.1,
                 g1=rng.uniform(0.5, 1.5, 64), h1=rng.standard_normal(64) * 0.2, mu1=rng.standard_normal(64) * 0.3,
                 var1=rng.uniform(0.5, 1.5, 64), eps1=1e-3,
                 W2=rng.standard_normal((128, 128)) / 128 ** 0.5, b2=rng.standard_normal(128) * 0.1,
                 g2=rng.uniform(0.5, 1.5, 128), h2=rng.standard_normal(128) * 0.2, mu2=rng.standard_normal(128) * 0.3,
                 var2=rng.uniform(0.5, 1.5, 128), eps2=1e-3)
        if kind in ("big", "small"):
            s = 2.0 ** 30 if kind == "big" else 2.0 ** -30
            p["g1"], p["h1"] = p["g1"] * s, p["h1"] * s
            if kind == "small":  # the second layer's own terms at the scale of its input: the split's floor shows in out
                p["b2"], p["mu2"] = p["b2"] * s, p["mu2"] * s
        elif kind == "signed":
            for i, n in ((1, 64), (2, 128)):
                g = rng.standard_normal(n)
                g[rng.random(n) < 0.2] = 0.0
                p["g%d" % i] = g
                h = p["h%d" % i]
                h[np.nonzero(g == 0)[0][::2]] = -0.0  # a channel that is -0.0 or +0.0 before the ReLU, whatever the row
        else:
            assert kind == "unit"
    return {k: (np.asarray(v, F64).astype(F32) if not k.startswith("eps") else float(v)) for k, v in p.items()}


# name -> (run lengths, points outside the grid: (leading, interleaved, trailing)).  Read off csrc/pfn_sorted.hip: k_ps_pfn2 deals
# the sorted rows in windows of 16; a voxel cut by a window edge takes atomic max on a row k_ps_place zeroed, every other a store.
LAYOUTS = {
    "runs_of_16": ([16] * 5, (0, 0, 0)),                      # no run cut: every row a plain store, nothing zeroed
    "cut_15_1_16": ([15, 1, 16], (0, 3, 0)),                  # run 1 is the window's last row; run 2 starts at a window edge
    "cut_17_15": ([17, 15], (0, 3, 0)),                       # run 0 crosses the edge by one row, run 1 ends at an edge
    "cut_1_16_15": ([1, 16, 15], (0, 3, 0)),                  # run 1 is cut after 15 rows, its last row opens window 1
    "covers_windows": ([8, 40, 3], (2, 5, 2)),                # run 1 = rows 8 .. 47: cut twice, window 1 wholly inside it
    "two_windows_edge_to_edge": ([16, 32, 16], (0, 4, 0)),    # run 1 starts AT rs and ends AT re of two windows: still atomics
    "singles_33": ([1] * 33, (1, 7, 1)),                      # sixteen voxel changes per tile, last window of one row
    "total_mod16_0": ([3, 5, 9, 2, 13], (0, 2, 0)),           # 32 rows
    "total_mod16_1": ([3, 5, 9, 2, 13, 1], (0, 2, 0)),        # 33 rows: last window of 1
    "total_mod16_15": ([3, 5, 9, 2, 13, 15], (0, 2, 0)),      # 47 rows: last window of 15
    "strides": ([1, 7, 1, 8, 1, 9, 1, 15, 1, 16, 1, 17, 1, 300, 1], (0, 9, 0)),  # k_ps_max1's 8-row step, k_ps_mean's 16 lanes
    "outside_leading": ([4, 1, 20], (40, 0, 0)),
    "outside_trailing": ([4, 1, 20], (0, 0, 40)),
    "outside_all_but_one": ([1], (30, 0, 30)),
}


def layout_points(runs, outside, seed, voxel_size, range_min, grid, dyadic=False, spread=3):
    """Points of a hand-built run layout.  Voxel v holds runs[v] points; the voxels are cells of the grid in key order
    (cell = spread * v + 1 of sample 0: neighbours are not adjacent cells), their points random inside the cell; `outside`
    = (leading, interleaved, trailing) points with voxel -1; the rest arrive in shuffled order.
    dyadic: coordinates in sixteenths whose sum over a run is n times a dyadic point, features small integers.
    Returns (points (P, 6) float32, point_voxel (P) int32, voxel_coords (N, 4) int32)."""
    rng = np.random.default_rng(seed)
    runs = np.asarray(runs, np.int64)
    N = len(runs)
    X, Y, Z = (int(v) for v in grid)
    cell = spread * np.arange(N, dtype=np.int64) + 1
    assert cell[-1] < X * Y * Z
    coords = np.stack([np.zeros(N, np.int64), cell % Z, (cell // Z) % Y, cell // (Y * Z)], 1).astype(np.int32)
    voxel = np.repeat(np.arange(N), runs)
    rows = len(voxel)
    vs, lo = np.asarray(voxel_size, F64), np.asarray(range_min, F64)
    corner = coords[voxel][:, [3, 2, 1]].astype(F64) * vs + lo
    if dyadic:
        d = rng.integers(-8, 9, (rows, 3)).astype(F64) / 16
        first = np.concatenate([[0], np.cumsum(runs)[:-1]])
        tot = np.zeros((N, 3))
        np.add.at(tot, voxel, d)
        d[first] -= tot  # every run's offsets add up to zero: the mean is the dyadic point below, exactly
        xyz = corner + np.asarray([0.125, 0.0625, 0.125]) + d
        feat = rng.integers(-3, 4, (rows, 2)).astype(F64)
    else:
        xyz = corner + rng.uniform(0.05, 0.95, (rows, 3)) * vs
        feat = rng.uniform(0, 1, (rows, 2))
    inside = np.concatenate([np.zeros((rows, 1)), xyz, feat], 1).astype(F32)
    lead, mid, trail = outside
    order = rng.permutation(rows)
    slots = np.sort(rng.choice(rows + mid, mid, replace=False)) if mid else np.zeros(0, np.int64)
    is_out = np.zeros(rows + mid, bool)
    is_out[slots] = True
    is_out = np.concatenate([np.ones(lead, bool), is_out, np.ones(trail, bool)])
    P = len(is_out)
    pts = np.zeros((P, 6), F32)
    pv = np.full(P, -1, np.int32)
    pts[~is_out], pv[~is_out] = inside[order], voxel[order].astype(np.int32)
    junk = rng.uniform(-1, 1, (int(is_out.sum()), 6)).astype(F32) * F32(100)
    junk[:, 0] = 0
    pts[is_out] = junk
    return pts, pv, coords
