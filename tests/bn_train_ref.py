"""A numpy float64 statement of BatchNorm2d in training mode with an optional ReLU behind it -- what mssvt_bn_train_fwd /
mssvt_bn_train_bwd and ``bn_train.BnReluFunction`` compute -- on a (P, C) matrix of P = B H W rows and C channels, and of the
per-element error bounds the kernels of csrc/bn_train.hip are held to.  Per channel:

    mean = sum x / P,  var = sum (x - mean)^2 / P,  invstd = 1 / sqrt(var + eps),  xhat = (x - mean) invstd
    z = xhat gamma + beta,  y = max(z, 0) with the ReLU, z without
    running_mean' = (1 - m) running_mean + m mean,  running_var' = (1 - m) running_var + m var P / (P - 1)
    g = dy mask,  dbeta = sum g,  dgamma = sum g xhat,  dx = gamma invstd (g - dbeta / P - xhat dgamma / P)

``backward_ref`` takes the ReLU mask as an argument (all ones without a ReLU).

The bounds, with u = 2^-24 (one fp32 rounding to nearest).  Second-order terms (u^2) are covered by the spare unit each count
below carries.  The kernel's geometry (csrc/bn_train.hip): pieces of R = piece_rows(C) = 8192 / C rows; a thread adds 8 rows of
a piece in row order, G = R / 8 threads of a channel are then added in order: an element passes A = 8 + G adds inside its
piece.  A workgroup owns `run` = ceil(pieces / 1024) consecutive pieces and merges them in piece order (L = run adds); the merge
launch then adds the workgroups' partials in 64 consecutive runs and the 64 run sums in order (L = ceil(workgroups / 64) + 64).

Statistics.  Piece i has n_i rows, the pivot K_i = its first row, D_i = sum |x - K_i|, Q_i = sum (x - K_i)^2, the exact piece
mean mean_i, q_i = mean_i - K_i:
  * s1 = sum (x - K_i): one rounding per difference, A per element for the adds: |error| <= (A + 1) u D_i =: e1_i;
    s2 = sum (x - K_i)^2 by fma: 2 u per square from the rounded difference, A for the adds: <= (A + 3) u Q_i;
  * mean_i~ = K_i + s1 / n_i: |error| <= e1_i / n_i + u |q_i| + u |mean_i| =: em_i;
  * M2_i~ = s2 - s1 (s1 / n_i): <= (A + 3) u Q_i + 2 |q_i| e1_i + 2 u n_i q_i^2 + u Q_i =: eM_i (clamping at 0 moves it towards
    the exact value, which is not negative);
  * a merge (``merge_bounds``; the same two formulas at both levels) of parts (n_i, mean_i~, M2_i~) with errors em_i, eM_i into
    N = sum n_i values with L adds per sum.  The mean, pivot K' = the first mean_i~ (the formula K' + sum n_i (mean_i - K') / N
    is exact in K'): with T = sum n_i |mean_i - K'|: e_mean = ((L + 2) u T + sum n_i em_i) / N + 2 u |mean - K'| + u |mean|
    (difference, product and L adds; division and the conversion of N; the last add).  M2 = sum M2_i + n_i (mean_i - mean)^2:
    the difference e_i = mean_i - mean is off by d_i = em_i + e_mean + u |e_i|, so
    e_M2 = sum [eM_i + n_i (2 |e_i| d_i + d_i^2) + 3 u n_i e_i^2] + (L + 2) u M2;
  * the pieces of a workgroup are merged with L = run, the workgroups with L = ceil(workgroups / 64) + 64; e_var = e_M2 / P + 2 u var;
  * invstd = 1 / sqrt(var + eps), three correctly rounded operations: with hi = 1 / sqrt(max(var - e_var, 0) + eps) and
    lo = 1 / sqrt(var + e_var + eps): e_invstd = max(hi - invstd, invstd - lo) + 3 u hi (no linearisation);
  * running_mean': m e_mean + 3 u (|1 - m| |running_mean| + m |mean|); running_var', with unb = var P / (P - 1):
    m (P / (P - 1) e_var + 4 u unb) + 3 u (|1 - m| |running_var| + m unb).
Forward values, per element with d = x - mean: e_xhat = (e_mean + u |d|) invstd + |d| e_invstd + u |xhat|,
    e_z = |gamma| e_xhat + u |xhat gamma| + u |z|; the ReLU does not enlarge it.
Backward, N = A + run + ceil(workgroups / 64) + 64 adds per element of a sum, SG = sum |g|, SGX = sum |g xhat|:
    e_dbeta = N u SG;  e_dgamma = (N + 1) u SGX + sum |g| e_xhat;
    a = dbeta / P: e_a = e_dbeta / P + 2 u |a|;  b = dgamma / P: e_b = e_dgamma / P + 2 u |b|;
    t = g - a - xhat b: e_t = e_a + |xhat| e_b + |b| e_xhat + 2 u (|g| + |a| + |xhat b|);
    f = gamma invstd: e_f = |gamma| e_invstd + u |f|;  dx = f t: e_dx = |f| e_t + |t| e_f + u |dx|.
"""
import numpy as np

U = 2.0 ** -24
PIECE_FLOATS = 8192
RUNS = 64
MAX_BLOCKS = 1024


def piece_rows(C):
    return PIECE_FLOATS // C


def num_pieces(P, R):
    return -(-P // R)


def run_pieces(pieces):
    """Pieces per workgroup (the launch rule)."""
    return -(-pieces // MAX_BLOCKS)


def merge_adds(parts):
    return -(-parts // RUNS) + RUNS


def merge_bounds(n, mean_i, M2_i, em, eM, starts, L):
    """Parts (rows of the arrays) merged in groups that begin at `starts`: exact (n, mean, M2) per group and the error bounds of
    the computed mean and M2, L adds per sum."""
    group = np.searchsorted(starts, np.arange(n.shape[0]), side="right") - 1
    N = np.add.reduceat(n, starts, axis=0)
    mean = np.add.reduceat(n * mean_i, starts, axis=0) / N
    first = mean_i[starts]
    T = np.add.reduceat(n * np.abs(mean_i - first[group]), starts, axis=0)
    e_mean = ((L + 2) * U * T + np.add.reduceat(n * em, starts, axis=0)) / N + 2 * U * np.abs(mean - first) + U * np.abs(mean)
    e = np.abs(mean_i - mean[group])
    d = em + e_mean[group] + U * e
    M2 = np.add.reduceat(M2_i + n * e * e, starts, axis=0)
    e_M2 = np.add.reduceat(eM + n * (2 * e * d + d * d) + 3 * U * n * e * e, starts, axis=0) + (L + 2) * U * M2
    return N, mean, M2, e_mean, e_M2


def forward_ref(x, gamma, beta, eps, momentum, running_mean, running_var, relu=True):
    """x (P, C); everything float64.  `eps` and `momentum` are used as given (hand over the float32 values the kernel gets)."""
    x = np.asarray(x, np.float64)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    P = x.shape[0]
    with np.errstate(all="ignore"):
        mean = x.sum(0) / P
        var = ((x - mean) ** 2).sum(0) / P
        invstd = 1.0 / np.sqrt(var + eps)
        xhat = (x - mean) * invstd
        z = xhat * gamma + beta
        y = np.where(z <= 0, 0.0, z) if relu else z
        rm = (1.0 - momentum) * np.asarray(running_mean, np.float64) + momentum * mean
        rv = (1.0 - momentum) * np.asarray(running_var, np.float64) + momentum * var * P / (P - 1.0)
    return dict(y=y, z=z, xhat=xhat, mean=mean, var=var, invstd=invstd, running_mean=rm, running_var=rv)


def backward_ref(x, dy, gamma, mean, invstd, mask):
    """dx (P, C), dgamma (C), dbeta (C) float64; `mask` (P, C): 1 where the gradient passes the ReLU."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    P = x.shape[0]
    with np.errstate(all="ignore"):
        g = np.where(mask, dy, 0.0)
        xhat = (x - mean) * invstd
        dbeta = g.sum(0)
        dgamma = (g * xhat).sum(0)
        dx = np.asarray(gamma, np.float64) * invstd * (g - dbeta / P - xhat * dgamma / P)
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, g=g, xhat=xhat)


def _piece_sums(v, R):
    return np.add.reduceat(v, np.arange(0, v.shape[0], R), axis=0)


def forward_bounds(x, gamma, beta, eps, momentum, running_mean, running_var, R):
    """{name: bound} for y / z (P, C), mean, var, invstd, running_mean, running_var (C), plus xhat's (P, C) for the backward."""
    x = np.asarray(x, np.float64)
    gamma = np.asarray(gamma, np.float64)
    P, C = x.shape
    f = forward_ref(x, gamma, beta, eps, momentum, running_mean, running_var, relu=False)
    mean, var, invstd = f["mean"], f["var"], f["invstd"]
    pieces, G = num_pieces(P, R), R // 8
    run = run_pieces(pieces)
    blocks = num_pieces(pieces, run)
    A = 8 + G
    starts = np.arange(0, P, R)
    n = np.minimum(R, P - starts).astype(np.float64)[:, None]
    piece_of = np.arange(P) // R
    dK = x - x[starts][piece_of]
    D, Q = _piece_sums(np.abs(dK), R), _piece_sums(dK * dK, R)
    q = _piece_sums(dK, R) / n
    mean_i = x[starts] + q
    e1 = (A + 1) * U * D
    em = e1 / n + U * np.abs(q) + U * np.abs(mean_i)
    eM = (A + 3) * U * Q + 2 * np.abs(q) * e1 + 2 * U * n * q * q + U * Q
    nb, mean_b, M2_b, em_b, eM_b = merge_bounds(n, mean_i, Q - n * q * q, em, eM, np.arange(0, pieces, run), run)
    _, _, M2, e_mean, e_M2 = merge_bounds(nb, mean_b, M2_b, em_b, eM_b, np.array([0]), merge_adds(blocks))
    e_mean, e_M2 = e_mean[0], e_M2[0]
    e_var = e_M2 / P + 2 * U * var
    hi = 1.0 / np.sqrt(np.maximum(var - e_var, 0.0) + eps)
    lo = 1.0 / np.sqrt(var + e_var + eps)
    e_invstd = np.maximum(hi - invstd, invstd - lo) + 3 * U * hi
    unb = var * P / (P - 1.0)
    rm, rv = np.abs(np.asarray(running_mean, np.float64)), np.abs(np.asarray(running_var, np.float64))
    e_rm = momentum * e_mean + 3 * U * (abs(1 - momentum) * rm + momentum * np.abs(mean))
    e_rv = momentum * (P / (P - 1.0) * e_var + 4 * U * unb) + 3 * U * (abs(1 - momentum) * rv + momentum * unb)
    dd = np.abs(x - mean)
    e_xhat = (e_mean + U * dd) * invstd + dd * e_invstd + U * np.abs(f["xhat"])
    e_z = np.abs(gamma) * e_xhat + U * np.abs(f["xhat"] * gamma) + U * np.abs(f["z"])
    return dict(y=e_z, z=e_z, xhat=e_xhat, mean=e_mean, var=e_var, invstd=e_invstd, running_mean=e_rm, running_var=e_rv)


def backward_bounds(x, dy, gamma, mean, invstd, mask, fwd_bounds, R):
    """{dx (P, C), dgamma (C), dbeta (C)}: `mean`, `invstd` the float64 statistics, `fwd_bounds` from ``forward_bounds``."""
    gamma = np.asarray(gamma, np.float64)
    b = backward_ref(x, dy, gamma, mean, invstd, mask)
    P = b["dx"].shape[0]
    pieces = num_pieces(P, R)
    run = run_pieces(pieces)
    N = 8 + R // 8 + run + merge_adds(num_pieces(pieces, run))
    g, xhat, e_xhat = np.abs(b["g"]), np.abs(b["xhat"]), fwd_bounds["xhat"]
    e_dbeta = N * U * g.sum(0)
    e_dgamma = (N + 1) * U * (g * xhat).sum(0) + (g * e_xhat).sum(0)
    a_, b_ = np.abs(b["dbeta"]) / P, np.abs(b["dgamma"]) / P
    e_a, e_b = e_dbeta / P + 2 * U * a_, e_dgamma / P + 2 * U * b_
    t = np.abs(b["g"] - b["dbeta"] / P - b["xhat"] * b["dgamma"] / P)
    e_t = e_a + xhat * e_b + b_ * e_xhat + 2 * U * (g + a_ + xhat * b_)
    f = np.abs(gamma * invstd)
    e_f = np.abs(gamma) * fwd_bounds["invstd"] + U * f
    e_dx = f * e_t + t * e_f + U * np.abs(b["dx"])
    return dict(dx=e_dx, dgamma=e_dgamma, dbeta=e_dbeta)


# ---- the kernels' arithmetic in float32 numpy, in their order of operations
def _padded(v, R, fill):
    """(pieces, 8, G, C): row k G + g of a piece at [k, g]; rows past the end take `fill` (pieces, C) or 0."""
    P, C = v.shape
    pieces = num_pieces(P, R)
    out = np.zeros((pieces * R, C), np.float32)
    out[:P] = v
    if fill is not None:
        out[P:] = fill[-1]
    return out.reshape(pieces, 8, R // 8, C)


def _piece_order_sum(terms):
    """(pieces, 8, G, C) float32 -> (pieces, C): 8 rows per thread in order, then the G threads in order."""
    s = np.zeros_like(terms[:, 0])
    for k in range(terms.shape[1]):
        s = s + terms[:, k]
    t = s[:, 0]
    for j in range(1, s.shape[1]):
        t = t + s[:, j]
    return t


def _block_order_sum(terms, run):
    """(pieces, C) float32 -> (workgroups, C): a workgroup's `run` consecutive pieces in piece order."""
    pieces = terms.shape[0]
    blocks = num_pieces(pieces, run)
    padded = np.zeros((blocks * run,) + terms.shape[1:], np.float32)
    padded[:pieces] = terms
    padded = padded.reshape((blocks, run) + terms.shape[1:])
    s = np.zeros_like(padded[:, 0])
    for j in range(run):
        s = s + padded[:, j]
    return s


def _run_order_sum(terms):
    """(parts, C) float32 -> (C,): 64 consecutive runs in order, then the runs in order."""
    pieces = terms.shape[0]
    length = -(-pieces // RUNS)
    total = None
    for r in range(RUNS):
        s = np.zeros(terms.shape[1], np.float32)
        for p in range(min(r * length, pieces), min((r + 1) * length, pieces)):
            s = s + terms[p]
        total = s if total is None else total + s
    return total


def forward_emulated(x, gamma, beta, eps, momentum, running_mean, running_var, relu, R):
    f32 = np.float32
    x, gamma, beta = np.asarray(x, f32), np.asarray(gamma, f32), np.asarray(beta, f32)
    eps, momentum = f32(eps), f32(momentum)
    P, C = x.shape
    starts = np.arange(0, P, R)
    K = x[starts]
    n = np.minimum(R, P - starts).astype(f32)[:, None]
    d = _padded(x, R, K) - K[:, None, None, :]
    s1 = _piece_order_sum(d)
    s2 = np.zeros((d.shape[0], d.shape[2], C), f32)
    for k in range(8):  # fma: one rounding
        s2 = (d[:, k].astype(np.float64) ** 2 + s2).astype(f32)
    t2 = s2[:, 0]
    for j in range(1, s2.shape[1]):
        t2 = t2 + s2[:, j]
    q = s1 / n
    pmean = K + q
    pm2 = np.maximum(t2 - s1 * q, f32(0))
    Pf = f32(P)
    pieces = pmean.shape[0]
    run = run_pieces(pieces)
    first = np.arange(0, pieces, run)
    group = np.arange(pieces) // run
    nb = _block_order_sum(n, run)  # (exact: row counts)
    bmean = pmean[first] + _block_order_sum(n * (pmean - pmean[first][group]), run) / nb
    e = pmean - bmean[group]
    bm2 = _block_order_sum(pm2, run) + _block_order_sum(n * (e * e), run)
    mean = bmean[0] + _run_order_sum(nb * (bmean - bmean[0])) / Pf
    e = bmean - mean
    var = _run_order_sum(bm2 + nb * (e * e)) / Pf
    invstd = f32(1) / np.sqrt(var + eps)
    rm = (f32(1) - momentum) * np.asarray(running_mean, f32) + momentum * mean
    rv = (f32(1) - momentum) * np.asarray(running_var, f32) + momentum * (var * (Pf / (Pf - f32(1))))
    z = (x - mean) * invstd * gamma + beta
    y = np.where(z <= 0, f32(0), z) if relu else z
    return dict(y=y, z=z, mean=mean, var=var, invstd=invstd, running_mean=rm, running_var=rv)


def backward_emulated(x, dy, gamma, beta, mean, invstd, relu, R):
    """`mean`, `invstd`: the float32 saved statistics.  Returns dx, dgamma, dbeta and the mask it used."""
    f32 = np.float32
    x, dy, gamma, beta = np.asarray(x, f32), np.asarray(dy, f32), np.asarray(gamma, f32), np.asarray(beta, f32)
    P = x.shape[0]
    xhat = (x - mean) * invstd
    mask = (xhat * gamma + beta > 0) if relu else np.ones(x.shape, bool)
    g = np.where(mask, dy, f32(0))
    run = run_pieces(num_pieces(P, R))
    dbeta = _run_order_sum(_block_order_sum(_piece_order_sum(_padded(g, R, None)), run))
    dgamma = _run_order_sum(_block_order_sum(_piece_order_sum(_padded(g * xhat, R, None)), run))
    Pf = f32(P)
    dx = (gamma * invstd) * (g - dbeta / Pf - xhat * (dgamma / Pf))
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta, mask=mask)


# ---- test inputs
PLANTED = dict(constant=0, far_mean=1, gamma_zero=2, gamma_negative=3, all_masked=4)


def inputs(P, C, seed, planted=True):
    """x, dy (P, C), gamma, beta, running_mean, running_var (C), float32: Gaussian with a per-channel scale in [0.1, 10] and a
    shift in [-3, 3]; with `planted`, channels 0 .. 4 are the cases of PLANTED."""
    rng = np.random.default_rng(seed)
    scale = np.exp(rng.uniform(np.log(0.1), np.log(10.0), C))
    shift = rng.uniform(-3, 3, C)
    x = rng.standard_normal((P, C)) * scale + shift
    gamma = rng.uniform(0.5, 1.5, C) * rng.choice([-1.0, 1.0], C)
    beta = rng.uniform(-1, 1, C)
    if planted:
        x[:, PLANTED["constant"]] = 1.7
        x[:, PLANTED["far_mean"]] = 1e4 + rng.standard_normal(P)
        gamma[PLANTED["gamma_zero"]] = 0.0
        gamma[PLANTED["gamma_negative"]] = -1.3
        beta[PLANTED["all_masked"]] = -1e4
    dy = rng.standard_normal((P, C)) * np.exp(rng.uniform(-2, 2, C))
    rm, rv = rng.standard_normal(C), rng.uniform(0.5, 2.0, C)
    return tuple(np.ascontiguousarray(v, np.float32) for v in (x, dy, gamma, beta, rm, rv))


def undecided(z64, e_z):
    """Elements whose float64 pre-activation lies inside the forward bound: the sign of the kernel's is not decided."""
    return np.abs(z64) <= e_z
