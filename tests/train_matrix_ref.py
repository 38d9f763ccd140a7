"""Float64 statements of the training path's four matrix kernels, with a bound for every element.  CPU, torch only.

    linear (csrc/linear_rows.hip, csrc/linear_rows_h.hip)   Y[m][n] = s act(b[n] + sum_k X[m][k] B[n][k])
    wgrad  (csrc/linear_wgrad.hip)                          dW[o][c] = sum_m dY[m][o] X[m][c],  db[o] = sum_m dY[m][o]
    pair attention (csrc/pair_attn.hip), per window and head
        s_ij = q_i . k_j,  P_ij = softmax_j s_ij,  O_i = sum_j P_ij v_j,  lse_i = log sum_j exp s_ij
        dq_i = sum_j ds_ij k_j,  dk_j = sum_i ds_ij q_i,  dv_j = sum_i P_ij dO_i,  ds_ij = P_ij (dO_i . v_j - dO_i . O_i)

Every bound is derived from the length of the operation and the float64 sum of the magnitudes of ITS OWN terms (`mag`);
none looks at a kernel's result or at a tensor's global maximum.  U = 2^-24 is the unit roundoff of float32.

linear_bound (fp32 operands).  A sum of K products, however it is ordered or split, is off by at most (K - 1) U mag to
first order (every add rounds a partial sum of at most mag); a product that is rounded on its own adds U of itself, the
bias add and the output scale one rounding each.  (K + 4) U mag |s| pays for those K + 2 roundings and their second-order
terms.  relu is exact and cannot increase an error.

linear_h_bound (split-fp16 operands, csrc/split_f16.hip.h).  Row and matrix are scaled by exact powers of two, so the
arithmetic is that of x' in (-2, 2) (-4, 4 for a row whose largest exponent is 254).  An operand is carried as hi + 2^-11 lo,
both halves TRUNCATED to fp16's 11 bits: the pair holds the top 22 bits, |x' - (hi + 2^-11 lo)| < 2^-21 |x'|, or 2^-35
where a half is an fp16 subnormal (spacing 2^-24; lo is scaled by 2^-11).  |x' - hi| < 2^-10 |x'|, so the dropped lo lo
product is below 2^-20 |x' w'|.  Per term: (2 2^-21 + 2^-20) |x w| = 32 U |x w|, plus 2^-35 (2^ex |w| + 2^ew |x|) with
2^ex, 2^ew the powers of two the row and the matrix were scaled by.  The hi hi chain is K adds in fp32 (K U mag); the cross
chain is 2 K adds of terms below 4 |x' w'|, scaled by 2^-11: below U mag for K <= 256; then one fma, one bias add, one
output scale.  (K + 40) U mag + the 2^-35 term, times |s|: 32 + K + 4 roundings + 4 for the second order.

wgrad_bound.  The M products of an element are added in slices and the slices in groups, an order that depends on the
device; the any-order bound (M + 2) U mag holds for all of them (M - 1 adds, one product rounding, second order).

Attention.  A dot product over a head of hd channels is off by at most es_ij = (hd + 1) U sum_d |q_id k_jd| in any order.
The kernels take e^x as exp2(x log2 e) in hardware: the rounded product moves the exponent by |x| U twice (the constant
is rounded too), the instruction adds 2 U: relative (2 |x| + 2) U.  Forward, online softmax over nk keys with score
spread D_i = max_j s_ij - min_j s_ij: the weight of key j reaches the sums through one exp of s_j - m (|x| <= D: both
scores off by es, the subtraction by |x| U, the exp by (2 |x| + 2) U) and through the corrections exp(m_old - m_new),
whose exponents add up to at most D and of which at most nk differ from exp(0) = 1 (3 U + 2 |dm| U each), and nk
multiply-add steps of two roundings: every weight is off by a factor e^t, |t| <= T_i = 2 es_i + (6 D_i + 6 nk + 8) U.
The normalised weights are then within e^(2 T) of P, and with the division's rounding
    |O - O~| <= (expm1(2 T_i) + 2 U) sum_j P_ij |v_jd|,       |lse - lse~| <= T_i + 4 U (|lse_i| + log nk + 1)
(log of a sum off by e^T, logf's two ulps, the last add).  Backward recomputes P_ij = exp(s_ij - lse_i) from the lse it
is given (a float32: off by U |lse|): relative Tb_ij = es_ij + (|lse_i| + 3 |x_ij| + 4) U, x_ij = s_ij - lse_i.
dp_ij = dO_i . v_j is off by e_dp = (hd + 1) U sum_d |dO v|, delta_i = dO_i . O_i (O a float32) by e_dl = (hd + 2) U sum_d
|dO O|, ds_ij by P_ij (expm1(Tb) |dp - delta| + 2 U |dp - delta| + e_dp + e_dl), and a sum of n such terms times k_jd
(or q_id) by a further (2 n + 4) U of its magnitudes:
    bound dq[i][d] = sum_j |k_jd| (P_ij ((expm1(Tb_ij) + (2 nk + 6) U) |dp_ij - delta_i| + e_dp_ij + e_dl_i) + z_ij)
    bound dk[j][d] = sum_i |q_id| (P_ij ((expm1(Tb_ij) + (2 nq + 6) U) |dp_ij - delta_i| + e_dp_ij + e_dl_i) + z_ij)
    bound dv[j][d] = sum_i |dO_id| (P_ij (expm1(Tb_ij) + (2 nq + 4) U) + 2^-125)
A probability below the smallest normal float32 comes out of the hardware exp2 as 0: an ABSOLUTE error of at most 2^-126
(taken as 2^-125) on P_ij, whatever P_ij is, hence z_ij = 2^-125 (|dp_ij - delta_i| + e_dp_ij + e_dl_i) on ds_ij and
2^-125 sum_j |v_jd| on O.
"""
import math

import torch

U32 = 2.0 ** -24
FLT_MAX = 3.4028234663852886e38
TINY = 2.0 ** -125


# ---------------------------------------------------------------------------------------------------------
# linear
# ---------------------------------------------------------------------------------------------------------

def linear_ref(x, w, transpose_w, bias, relu, out_scale, dtype=torch.float64):
    """(Y, mag): Y = s act(b + X B^T), B = W (N, K) or W^T for W (K, N); mag = |b| + sum_k |X B| (before s)."""
    x, w = x.to(dtype), w.to(dtype)
    B = w.t() if transpose_w else w
    y = x @ B.t()
    mag = x.abs() @ B.abs().t()
    if bias is not None:
        y = y + bias.to(dtype)
        mag = mag + bias.to(dtype).abs()
    if relu:
        y = y.clamp(min=0)
    return y * out_scale, mag


def linear_bound(K, mag, out_scale):
    return (K + 4) * U32 * mag * abs(out_scale)


def _pow2_floor(v):
    """2^floor(log2 v) for v > 0 (float64 tensor), 1 where v == 0."""
    m, e = torch.frexp(v.double())
    return torch.where(v > 0, torch.ldexp(torch.ones_like(m), e - 1), torch.ones_like(m))


def linear_h_bound(x, w, transpose_w, mag, out_scale):
    x, w = x.double(), w.double()
    B = w.t() if transpose_w else w
    K = x.shape[1]
    ex = _pow2_floor(x.abs().max(1, keepdim=True).values)  # (M, 1)
    ew = _pow2_floor(w.abs().max().reshape(1, 1))
    sub = 2.0 ** -35 * (ex * B.abs().sum(1).unsqueeze(0) + ew * x.abs().sum(1, keepdim=True))
    return ((K + 40) * U32 * mag + sub) * abs(out_scale)


# ---------------------------------------------------------------------------------------------------------
# weight gradient
# ---------------------------------------------------------------------------------------------------------

def wgrad_ref(x, dy, dtype=torch.float64):
    """(dW (Cout, Cin), db (Cout), mag_w, mag_b)."""
    x, dy = x.to(dtype), dy.to(dtype)
    return dy.t() @ x, dy.sum(0), dy.abs().t() @ x.abs(), dy.abs().sum(0)


def wgrad_bound(M, mag):
    return (M + 2) * U32 * mag


# ---------------------------------------------------------------------------------------------------------
# pair attention
# ---------------------------------------------------------------------------------------------------------

def attn_ref(wins, q, kv, dO, heads, hd, O_in=None, lse_in=None, dtype=torch.float64):
    """wins = (q_off, q_cnt, k_off, k_cnt) integer lists; q (R, cg), kv (Kn, 2 cg), dO (R, cg).
    Returns a dict of O, lse (R, heads), dq, dkv and, with dtype float64, their bounds bO, blse, bdq, bdkv.
    The backward takes O_in / lse_in where given (what the kernel is handed), else its own forward."""
    cg = heads * hd
    q, kv, dO = q.to(dtype), kv.to(dtype), dO.to(dtype)
    R, Kn = q.shape[0], kv.shape[0]
    want_b = dtype == torch.float64
    out = dict(O=torch.zeros(R, cg, dtype=dtype), lse=torch.zeros(R, heads, dtype=dtype), dq=torch.zeros(R, cg, dtype=dtype),
               dkv=torch.zeros(Kn, 2 * cg, dtype=dtype))
    if want_b:
        out.update(bO=torch.zeros(R, cg, dtype=dtype), blse=torch.zeros(R, heads, dtype=dtype),
                   bdq=torch.zeros(R, cg, dtype=dtype), bdkv=torch.zeros(Kn, 2 * cg, dtype=dtype))
    for qo, nq, ko, nk in zip(*[[int(v) for v in a] for a in wins]):
        if nq == 0 or nk == 0:
            continue  # no query: dkv rows 0; no key: O, lse, dq rows 0
        qs, ks = slice(qo, qo + nq), slice(ko, ko + nk)
        qi, gi = q[qs].view(nq, heads, hd), dO[qs].view(nq, heads, hd)
        k, v = kv[ks, :cg].view(nk, heads, hd), kv[ks, cg:].view(nk, heads, hd)
        s = torch.einsum("ihd,jhd->hij", qi, k)
        lse = torch.logsumexp(s, dim=-1)  # (h, i)
        P = torch.exp(s - lse.unsqueeze(-1))
        O = torch.einsum("hij,jhd->ihd", P, v)
        out["O"][qs] = O.reshape(nq, cg)
        out["lse"][qs] = lse.t()
        Ob = O if O_in is None else O_in[qs].to(dtype).view(nq, heads, hd)
        lb = lse if lse_in is None else lse_in[qs].to(dtype).t()
        Pb = torch.exp(s - lb.unsqueeze(-1))
        dp = torch.einsum("ihd,jhd->hij", gi, v)
        delta = (gi * Ob).sum(-1).t().unsqueeze(-1)  # (h, i, 1)
        ds = Pb * (dp - delta)
        out["dq"][qs] = torch.einsum("hij,jhd->ihd", ds, k).reshape(nq, cg)
        out["dkv"][ks, :cg] = torch.einsum("hij,ihd->jhd", ds, qi).reshape(nk, cg)
        out["dkv"][ks, cg:] = torch.einsum("hij,ihd->jhd", Pb, gi).reshape(nk, cg)
        if not want_b:
            continue
        es = (hd + 1) * U32 * torch.einsum("ihd,jhd->hij", qi.abs(), k.abs())
        D = s.max(-1).values - s.min(-1).values  # (h, i)
        T = 2 * es.max(-1).values + (6 * D + 6 * nk + 8) * U32
        Av = torch.einsum("hij,jhd->ihd", P, v.abs())
        floor_v = TINY * v.abs().sum(0).unsqueeze(0)  # (1, h, d)
        out["bO"][qs] = ((torch.expm1(2 * T).t().unsqueeze(-1) + 2 * U32) * Av + floor_v).reshape(nq, cg)
        out["blse"][qs] = (T + 4 * U32 * (lse.abs() + math.log(nk) + 1)).t()
        x = s - lse.unsqueeze(-1)
        Tb = torch.expm1(es + (lse.abs().unsqueeze(-1) + 3 * x.abs() + 4) * U32)
        e_dp = (hd + 1) * U32 * torch.einsum("ihd,jhd->hij", gi.abs(), v.abs())
        e_dl = (hd + 2) * U32 * (gi * O).abs().sum(-1).t().unsqueeze(-1)
        dd = (dp - (gi * O).sum(-1).t().unsqueeze(-1)).abs()
        lost = TINY * (dd + e_dp + e_dl)  # a probability the hardware exp2 returns as 0
        t_q = P * ((Tb + (2 * nk + 6) * U32) * dd + e_dp + e_dl) + lost
        t_k = P * ((Tb + (2 * nq + 6) * U32) * dd + e_dp + e_dl) + lost
        t_v = P * (Tb + (2 * nq + 4) * U32) + TINY
        out["bdq"][qs] = torch.einsum("hij,jhd->ihd", t_q, k.abs()).reshape(nq, cg)
        out["bdkv"][ks, :cg] = torch.einsum("hij,ihd->jhd", t_k, qi.abs()).reshape(nk, cg)
        out["bdkv"][ks, cg:] = torch.einsum("hij,ihd->jhd", t_v, gi.abs()).reshape(nk, cg)
    return out


# ---------------------------------------------------------------------------------------------------------
# the hand-built window lists of the attention tests
# ---------------------------------------------------------------------------------------------------------

NQS = (0, 1, 7, 8, 9, 16, 17, 33)  # either side of PA_QB = 8 rows per item and of four items (33 queries: five)
NKS = (0, 1, 3, 4, 5, 8, 9, 17, 33)  # either side of PA_KB = 4 rows per chunk; as dkv items either side of 8 and of four items


def window_grid(seed, pairs=None):
    """(q_off, q_cnt, k_off, k_cnt, R, Kn) as int64 tensors: one window per (nq, nk) pair (default: all 72 of NQS x NKS and
    one more (9, 5): 73 windows, no multiple of 4), in shuffled order; the windows' query rows and key rows partition [0, R)
    and [0, Kn) in two further, different shuffled orders, so consecutive windows do not own ascending rows."""
    g = torch.Generator().manual_seed(seed)
    if pairs is None:
        pairs = [(a, b) for a in NQS for b in NKS] + [(9, 5)]
    pairs = [pairs[i] for i in torch.randperm(len(pairs), generator=g).tolist()]
    nw = len(pairs)
    q_cnt, k_cnt = torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])
    q_off, k_off = torch.zeros(nw, dtype=torch.long), torch.zeros(nw, dtype=torch.long)
    at = 0
    for w in torch.randperm(nw, generator=g).tolist():
        q_off[w] = at
        at += int(q_cnt[w])
    R, at = at, 0
    for w in torch.randperm(nw, generator=g).tolist():
        k_off[w] = at
        at += int(k_cnt[w])
    return q_off, q_cnt, k_off, k_cnt, R, at


def attn_operands(seed, heads, hd, kind, pairs=None):
    """(wins, q, kv, dO) of one attention case, float32 on the CPU.  kind: "grid" plain normal operands; "hot" scores up
    to about 60 in magnitude (the running maximum of the online softmax moves); "same" every key row of a window
    identical; "dominant" one key of every window ahead of the others by more than 100 (their probabilities underflow);
    "int" integers, |q|, |k| <= 3 and |v|, |dO| <= 3 (the exact degenerate cases)."""
    g = torch.Generator().manual_seed(seed)
    q_off, q_cnt, k_off, k_cnt, R, Kn = window_grid(seed, pairs)
    cg = heads * hd
    q, kv, dO = torch.randn(R, cg, generator=g), torch.randn(Kn, 2 * cg, generator=g), torch.randn(R, cg, generator=g)
    if kind == "hot":
        q *= 13.0 / hd ** 0.5
    elif kind == "same":
        for o, n in zip(k_off.tolist(), k_cnt.tolist()):
            kv[o:o + n] = kv[o:o + 1]
    elif kind == "dominant":
        q = 4.0 + 0.25 * torch.rand(R, cg, generator=g)
        kv[:, :cg] *= 0.1
        for o, n in zip(k_off.tolist(), k_cnt.tolist()):
            if n:
                kv[o + n // 2, :cg] = 40.0 / hd
    elif kind == "int":
        q = torch.randint(-3, 4, (R, cg), generator=g).float()
        kv = torch.randint(-3, 4, (Kn, 2 * cg), generator=g).float()
        dO = torch.randint(-3, 4, (R, cg), generator=g).float()
    else:
        assert kind == "grid"
    return (q_off, q_cnt, k_off, k_cnt), q, kv, dO
