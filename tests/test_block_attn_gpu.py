"""Every launch form of the Block attention (csrc/block_attn.hip, csrc/block_attn_bf16.hip) against a float64 evaluation
of the reference formulas (mssvt_backbone.py:260-295, mssvt_utils.py:112-150), on hand-built windows.

The C entry points are driven directly (include/mssvt_hip.h: mssvt_plan_order, mssvt_block_attention,
mssvt_block_attention_kv16 with and without mssvt_attn_pack_weights blobs, mssvt_block_attention_bf16), not through
two_scale_plan: a case is a few hundred windows whose structure the test chooses -- one live key, keys only in the last
16-slot tile, an empty tile between two used ones, row counts off the 16-row tile, no active window, more windows than
the persistent grid has waves, operands near the top of the fp16 range.

Tolerances:
  fp32 / kv16 / kv16+blobs   |got - ref| <= 1e-5 max|ref| + 1e-4 |ref| elementwise over the written rows
  bf16                       max|err| <= 5e-2 max|ref|  and  rms(err) <= 1e-2 rms(ref)
  operands near 65504 (kv16) max|err| <= 8 max(e32), mean|err| <= 8 mean(e32), e32 = |float32 torch evaluation - float64|
                             (split operands keep 22 of 24 mantissa bits = 4 rounding units; the re-association
                             Qt = scale Wk^T q', Wv after the key sum, and the hardware exp2: another factor 2)
The masked slots of the float64 reference are at -inf (the kernels' contract), not the reference's additive -100.
tests/test_block_attn_ref_cpu.py checks the reference itself (a loop restatement, and that mutated formulas leave these
tolerances by a factor >= 10 on every class of inputs used here) without a GPU.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

LOG2E = 1.4426950408889634
F16_MAX = 65504.0
E_TOOLARGE = -2
SENTINEL = -12345.678
MAX_RATIO = 8.0  # case (e): see the module docstring

# the (Cg, head_dim) pairs of MSSVT_ATTN_CASE in dispatch_block_attn (csrc/block_attn.hip)
F32_SHAPES = [(8, 8), (16, 8), (16, 16), (24, 8), (32, 8), (32, 16), (32, 32), (48, 16), (64, 8), (64, 16), (64, 32)]
BLOB_SHAPES = [(32, 16), (64, 16)]  # mssvt_attn_packed_bytes > 0
KEY_TIERS = [1, 8, 16, 17, 32, 33, 48, 64]
MUTATIONS = ("mask_last_live", "swap_heads_v", "drop_bv", "scores_ln2", "drop_centre")


def bf16_shapes():
    from mssvt_amd import fused
    return sorted(fused.ATTN_BF16_SHAPES)


def kv16_runs(cg, K):
    """Where mssvt_block_attention_kv16 runs the split-fp16 window launch (include/mssvt_hip.h); elsewhere the fp32 form."""
    return cg % 32 == 0 and 16 < K <= 64


# ---------------------------------------------------------------------------------------------------------------------
# 1. input builder (torch, seeded, CPU tensors; nothing here needs a GPU)
# ---------------------------------------------------------------------------------------------------------------------
class Case(object):
    """C, groups [(c0, Cg, heads)], hd, nq, K, nw, N, cap; xhat (N,C); wcentre (cap,4); kmeta[g] (cap,K,4) and qmeta
    (cap,nq,4): (offset xyz, bits(row) or bits(-1)); nq_valid (cap); Wq/bq/Wkv/bkv/Wo/bo per group, Wpos (C,6), bpos."""

    def tensors(self):
        return dict(xhat=self.xhat, wcentre=self.wcentre, qmeta=self.qmeta, nq_valid=self.nq_valid, Wpos=self.Wpos,
                    bpos=self.bpos, kmeta=self.kmeta, Wq=self.Wq, bq=self.bq, Wkv=self.Wkv, bkv=self.bkv, Wo=self.Wo,
                    bo=self.bo)

    @property
    def scale(self):
        return float(self.hd) ** -0.5

    @property
    def total_rows(self):
        return int(self.nq_valid[:self.nw].sum())


def _uniform(g, shape, bound):
    return (torch.rand(shape, generator=g) * 2 - 1) * bound


def _linear(g, out_f, in_f):
    """nn.Linear / Conv1d(kernel 1) default init: weight and bias uniform in +-1/sqrt(fan_in)."""
    b = 1.0 / math.sqrt(in_f)
    return _uniform(g, (out_f, in_f), b), _uniform(g, (out_f,), b)


def _with_rows(rel, rows):
    meta = torch.empty(rel.shape[:-1] + (4,), dtype=torch.float32)
    meta[..., :3] = rel
    meta.view(torch.int32)[..., 3] = rows.to(torch.int32)
    return meta


def row_bits(meta):
    return meta.view(torch.int32)[..., 3].long()


def _key_list(g, cap, K, N, mode):
    live = torch.zeros(cap, K, dtype=torch.bool)
    r = torch.rand(cap, K, generator=g)
    if mode == "mixed":
        live = r < torch.rand(cap, 1, generator=g)
    elif mode == "one":
        pass
    elif mode == "first_last_tile":  # slot 0 and the last 16-slot tile only
        t0 = 16 * ((K - 1) // 16)
        assert t0 > 0
        live[:, t0:] = r[:, t0:] < 0.5
        live[:, K - 1] = True
    elif mode == "tile1_empty":  # tile 1 empty between live tiles 0 and 2
        assert K > 32
        live = r < 0.5
        live[:, 16:32] = False
        live[:, min(37, K - 1)] = True
    elif mode in ("all", "repeat"):
        live[:] = True
    else:
        raise ValueError(mode)
    live[:, 0] = True  # slot 0 of a key list is never masked
    rows = torch.randint(0, N, (cap, K), generator=g)
    if mode == "repeat":  # one row in many slots of a window; row 0 (what an empty FPS pick resolves to) in every other window
        rep = torch.randint(0, N, (cap, 1), generator=g)
        rep[0::2] = 0
        rows = torch.where(r < 0.6, rep.expand(-1, K), rows)
    rel = _uniform(g, (cap, K, 3), 1.0) * torch.tensor([3.0, 3.0, 2.0])
    return _with_rows(rel, torch.where(live, rows, torch.full_like(rows, -1)))


def _query_list(g, cap, nw, nq, N, mode):
    r = torch.rand(cap, nq, generator=g)
    if mode == "mixed":  # any count from 0 to nq, valid slots anywhere in the list
        valid = r < torch.rand(cap, 1, generator=g) * 1.2
    elif mode == "most":
        valid = r < 0.75
        valid[nw - 1, :2] = True
    elif mode == "interleave_zero":
        valid = r < 0.6
        valid[1::2] = False
    elif mode == "none":
        valid = torch.zeros(cap, nq, dtype=torch.bool)
    elif mode == "all":
        valid = torch.ones(cap, nq, dtype=torch.bool)
    elif isinstance(mode, tuple) and mode[0] == "total":  # exactly mode[1] valid slots, scattered over the windows
        assert mode[1] <= nw * nq
        valid = torch.zeros(cap * nq, dtype=torch.bool)
        valid[torch.randperm(nw * nq, generator=g)[:mode[1]]] = True
        valid = valid.reshape(cap, nq)
    else:
        raise ValueError(mode)
    valid[nw:] = False
    rows = torch.randint(0, N, (cap, nq), generator=g)
    rel = _uniform(g, (cap, nq, 3), 1.0) * torch.tensor([1.5, 1.5, 1.0])
    return _with_rows(rel, torch.where(valid, rows, torch.full_like(rows, -1))), valid.sum(1).to(torch.int32)


def make_case(C, groups, hd, nq, K, nw, N=600, seed=0, keys="mixed", queries="mixed", centres="mixed", cap=None,
              shared_keys=False):
    g = torch.Generator().manual_seed(1000 + seed)
    c = Case()
    c.C, c.groups, c.hd, c.nq, c.K, c.nw, c.N = C, [tuple(x) for x in groups], hd, nq, K, nw, N
    c.cap = nw + 3 if cap is None else cap
    assert c.cap >= nw >= 1 and C % 4 == 0
    for c0, cg, heads in c.groups:
        assert cg == heads * hd and c0 % 4 == 0 and c0 + cg <= C
    c.xhat = torch.randn(N, C, generator=g)
    # even windows: centres within +-75 m (scores spread over ~40, a few keys carry the softmax); odd: 0 m (flat)
    c.wcentre = torch.zeros(c.cap, 4)
    far = _uniform(g, (c.cap, 3), 1.0) * torch.tensor([75.0, 75.0, 4.0])
    if centres == "mixed":
        c.wcentre[0::2, :3] = far[0::2]
    elif centres == "near":  # within +-10 m: every key carries weight AND the centre matters (the one-row cases)
        c.wcentre[:, :3] = far * (10.0 / 75.0)
    else:
        assert centres == "zero"
    c.kmeta = []
    for gi in range(len(c.groups)):
        c.kmeta.append(c.kmeta[0] if (shared_keys and gi) else _key_list(g, c.cap, K, N, keys))
    c.qmeta, c.nq_valid = _query_list(g, c.cap, nw, nq, N, queries)
    c.Wq, c.bq, c.Wkv, c.bkv, c.Wo, c.bo = [], [], [], [], [], []
    for _, cg, _ in c.groups:
        for W, b, (o, i) in ((c.Wq, c.bq, (cg, cg)), (c.Wkv, c.bkv, (2 * cg, cg)), (c.Wo, c.bo, (cg, cg))):
            w_, b_ = _linear(g, o, i)
            W.append(w_)
            b.append(b_)
    c.Wpos, c.bpos = _linear(g, C, 6)
    check_invariants(c)
    return c


def check_invariants(c):
    """What the kernels' contract asks of the caller: no case may leave it."""
    for km in c.kmeta:
        rows = row_bits(km)
        assert km.shape == (c.cap, c.K, 4) and bool((rows[:, 0] >= 0).all())
        assert bool(((rows >= -1) & (rows < c.N)).all()) and bool(torch.isfinite(km[..., :3]).all())
    rows = row_bits(c.qmeta)
    assert c.qmeta.shape == (c.cap, c.nq, 4) and bool(((rows >= -1) & (rows < c.N)).all())
    assert torch.equal((rows >= 0).sum(1).to(torch.int32), c.nq_valid) and int(c.nq_valid[c.nw:].sum()) == 0
    assert c.cap >= c.nw and c.wcentre.shape == (c.cap, 4)


# ---------------------------------------------------------------------------------------------------------------------
# 2. reference
# ---------------------------------------------------------------------------------------------------------------------
def reference(case, dtype=torch.float64, device="cpu", mutate=None, row_capacity=None, chunk=1024):
    """(attn, stats): attn (cap*nq + 1, C) in `dtype` with NaN wherever the kernels must not write; stats = max|.| over
    valid queries / live keys of tokens, qp (Q'), qt (scale log2e Wk_h^T q'_h), xbar, v, and score.  `mutate` evaluates a
    deliberately wrong formula (tests/test_block_attn_ref_cpu.py).  Windows whose compact rows end past row_capacity are
    dropped (include/mssvt_hip.h, mssvt_plan_order)."""
    f = lambda t: t.to(device).to(dtype)  # noqa: E731
    nw, nq, K, C, hd = case.nw, case.nq, case.K, case.C, case.hd
    out = torch.full((case.cap * nq + 1, C), float("nan"), dtype=dtype, device=device)
    stats = dict(tokens=0.0, qp=0.0, qt=0.0, xbar=0.0, v=0.0, score=0.0)

    def bump(name, t):
        if t.numel():
            stats[name] = max(stats[name], float(t.abs().max()))

    xh, Wp, bp = f(case.xhat), f(case.Wpos), f(case.bpos)
    wc = f(case.wcentre[:, :3])  # the f32 values handed to the kernel
    if mutate == "drop_centre":
        wc = torch.zeros_like(wc)
    qm = case.qmeta.to(device)
    qrow = row_bits(qm)
    qvalid = qrow >= 0
    nqv = qvalid.sum(1)
    if row_capacity is not None:
        qvalid = qvalid & ((nqv.cumsum(0) <= row_capacity)[:, None])
    for gi, (c0, cg, heads) in enumerate(case.groups):
        km = case.kmeta[gi].to(device)
        krow = row_bits(km)
        live = krow >= 0
        if mutate == "mask_last_live":  # the last live slot of every window that has two
            last = (live * torch.arange(K, device=device)).max(1).values
            sel = live.sum(1) >= 2
            live = live.clone()
            live[sel.nonzero()[:, 0], last[sel]] = False
        Wq, bq, Wkv, bkv, Wo, bo = [f(t[gi]) for t in (case.Wq, case.bq, case.Wkv, case.bkv, case.Wo, case.bo)]
        xg, Wpg, bpg = xh[:, c0:c0 + cg], Wp[c0:c0 + cg], bp[c0:c0 + cg]

        def tokens(meta, rows, centre):
            geo = torch.cat([f(meta[..., :3]), centre[:, None, :].expand(-1, meta.shape[1], -1)], dim=-1)
            return xg[rows.clamp(min=0)] + torch.relu(geo @ Wpg.T + bpg)

        for w0 in range(0, nw, chunk):
            w1 = min(w0 + chunk, nw)
            n, lv, qv = w1 - w0, live[w0:w1], qvalid[w0:w1]
            tk = tokens(km[w0:w1], krow[w0:w1], wc[w0:w1])  # (n, K, cg)
            tq = tokens(qm[w0:w1], qrow[w0:w1], wc[w0:w1])  # (n, nq, cg)
            qp = tq @ Wq.T + bq
            kv = tk @ Wkv.T + bkv
            Kp, V = kv[..., :cg], kv[..., cg:]
            if mutate == "drop_bv":
                V = V - bkv[cg:]
            s = torch.einsum("nqhd,nkhd->nhqk", (qp * case.scale).reshape(n, nq, heads, hd), Kp.reshape(n, K, heads, hd))
            if mutate == "scores_ln2":
                s = s * math.log(2.0)
            s = s.masked_fill(~lv[:, None, None, :], float("-inf"))
            p = torch.softmax(s, dim=-1)
            Vh = V.reshape(n, K, heads, hd)
            if mutate == "swap_heads_v":  # heads h and h + 1 swapped in the V product
                order = list(range(heads))
                for h in range(0, heads - 1, 2):
                    order[h], order[h + 1] = h + 1, h
                Vh = Vh[:, :, order]
            o = torch.einsum("nhqk,nkhd->nqhd", p, Vh).reshape(n, nq, cg)
            res = o @ Wo.T + bo
            dest = (torch.arange(w0, w1, device=device)[:, None] * nq + torch.arange(nq, device=device))[qv]
            out[dest, c0:c0 + cg] = res[qv]
            bump("tokens", tk[lv])
            bump("tokens", tq[qv])
            bump("qp", qp[qv])
            bump("qt", torch.einsum("nqhd,hdc->nqhc", qp.reshape(n, nq, heads, hd), Wkv[:cg].reshape(heads, hd, cg))[qv]
                 * (case.scale * LOG2E))
            bump("xbar", torch.einsum("nhqk,nkc->nqhc", p, tk)[qv])
            bump("v", V[lv])
            bump("score", s[(qv[:, None, :, None] & lv[:, None, None, :]).expand_as(s)])
    return out, stats


def reference_f64(case, **kw):
    return reference(case, dtype=torch.float64, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# 3. cases
# ---------------------------------------------------------------------------------------------------------------------
def case_a(cg, hd, K):
    """One group, nq = 3, mixed masks, both score regimes."""
    return make_case(cg, [(0, cg, cg // hd)], hd, 3, K, 200, seed=cg * 100 + hd + K)


# group layouts at C = 128 / 96: name -> (C, groups, head_dim); `shared_keys` False: every group its own key lists
LAYOUTS = {
    "one_group_at_c0_64": (128, [(64, 64, 4)], 16),  # channels [0, 64) stay untouched
    "two_equal": (128, [(0, 64, 4), (64, 64, 4)], 16),
    "two_unequal_32_64": (96, [(0, 32, 2), (32, 64, 4)], 16),  # both kv16-capable, both with blobs
    "two_unequal_16_48": (96, [(0, 16, 1), (16, 48, 3)], 16),  # neither width is a multiple of 32: kv16 keeps the fp32 form
    "two_unequal_48_32": (96, [(0, 48, 3), (48, 32, 2)], 16),  # only the second group kv16-capable; [80, 96) uncovered
    "four_equal_16x8": (128, [(0, 16, 2), (16, 16, 2), (32, 16, 2), (48, 16, 2)], 8),  # [64, 128) uncovered
    "four_equal_32x16": (128, [(0, 32, 2), (32, 32, 2), (64, 32, 2), (96, 32, 2)], 16),
    "three_equal_32x16": (128, [(0, 32, 2), (32, 32, 2), (64, 32, 2)], 16),  # [96, 128) uncovered
}


def case_b(layout, K):
    C, groups, hd = LAYOUTS[layout]
    return make_case(C, groups, hd, 4, K, 150, seed=7 + K + len(layout))


# window structure: name -> make_case arguments (at (64,16) and (32,16), K = 32 and 64)
STRUCTURES = {
    "one_live_key": dict(keys="one"),
    "slot0_and_last_tile": dict(keys="first_last_tile"),
    "tile1_empty": dict(keys="tile1_empty"),  # K = 64 only: K = 32 has no tile 2
    "all_live": dict(keys="all"),
    "repeated_rows": dict(keys="repeat"),
    "nq1": dict(nq=1), "nq4": dict(nq=4), "nq5": dict(nq=5), "nq16": dict(nq=16), "nq20": dict(nq=20), "nq45": dict(nq=45),
    "zero_query_windows_interleaved": dict(queries="interleave_zero"),
    "rows1": dict(queries=("total", 1), nw=20, centres="near"), "rows15": dict(queries=("total", 15), nw=20, centres="near"),
    "rows16": dict(queries=("total", 16), nw=20, centres="near"), "rows17": dict(queries=("total", 17), nw=20, centres="near"),
    "rows33": dict(queries=("total", 33), nw=20, centres="near"),
    "no_active_window": dict(queries="none", nw=40),
    "one_window": dict(nw=1, queries="all"),
}
C_SHAPES = [(64, 32), (64, 64), (32, 32), (32, 64)]  # (Cg, K); head_dim 16


def structure_applies(name, K):
    return K > 32 or name != "tile1_empty"


def case_c(name, cg, K):
    kw = dict(nq=5, nw=120)
    kw.update(STRUCTURES[name])
    return make_case(cg, [(0, cg, cg // 16)], 16, kw.pop("nq"), K, kw.pop("nw"), seed=cg + K + len(name), **kw)


def case_d(K, cus):
    """More windows than three rounds of the largest per-window grid (cus x 4 workgroups x 4 waves), and more rows than two
    rounds of the row-tiled grids: all three pipeline stages run on real and on clamped indices."""
    nw = 3 * (cus * 4 * 4) + 17
    c = make_case(64, [(0, 64, 4)], 16, 16, K, nw, seed=50 + K, queries="most")
    assert c.total_rows > 2 * cus * 2 * 8 * 16 or cus < 64
    return c


E_QUANTITIES = ("tokens", "qp", "qt", "xbar", "v")  # what the kv16 caller bounds (fused._attn_kv16_ok)
E_SUBCASES = E_QUANTITIES + ("sharp", "tiny_wq")
E_SHAPES = [(64, 32), (64, 64), (32, 32), (32, 64)]  # (Cg, K); head_dim 16
E_TARGET = dict(tokens=0.7, qp=0.7, qt=0.7, xbar=0.55, v=0.7, tiny_wq=0.7)
# The halves of a split-fp16 operand bottom out at 2^-24 / 2^11 = 2^-35 absolute, so a matrix keeps the form's 22 bits
# relative to its largest entry only while that entry is >= 2^-13: where a sub-case has to shrink a projection to keep the
# scores moderate it stops there (and lets the scores grow instead), so that case (e) tests the TOP of the range alone.
# `tiny_wq` is the finding that drew this line: Wq shrunk to ~1e-7 -- the pre-split fragments lose the small weights, the
# caller's guard (fused.ATTN_F16_FLOOR) keeps such projections off the blobs.
SPLIT_FLOOR = 2.0 ** -13


def _shrink(W, factor, folded=1.0):
    """W *= factor, but no further than max|W| * folded = 1.05 x SPLIT_FLOOR; returns the factor applied."""
    f = max(factor, 1.05 * SPLIT_FLOOR / (float(W.abs().max()) * folded))
    W *= f
    return f


def case_e(cg, K, sub):
    """One of the five quantities the kv16 caller bounds at E_TARGET x 65504 (float64 reference), the others below it.
    Every scaling is exactly homogeneous in the scaled quantity (s = target / its value on the unscaled case):
      tokens / xbar   xhat, Wpos, bpos x s;  Wq x fq, bq x fq s, Wk x fk with fq ~ 1/s, fk ~ 1/(s^2 fq) (see SPLIT_FLOOR):
                      Q' as before, scores x s^2 fq fk.  (Xbar is a convex combination of key tokens: it can reach the
                      token maximum, never pass it -- so for `xbar` the tokens stay below 0.9 x 65504 instead.)
      qp              Wq, bq x s;  Wk x fk ~ 1/s
      qt              xhat, Wpos, bpos / (s / 4);  Wq, Wk x s / 2;  bq x 2:  Q' x 2, Qt x s, scores x 4
      v               Wv, bv x s
      tiny_wq         as tokens, but Wq / s^2, bq / s, Wk as it is: Wq ~ 1e-7, far below SPLIT_FLOOR
    `sharp`: Wq, bq x 30 (scores of magnitude 1e3 .. 1e4)."""
    c = make_case(cg, [(0, cg, cg // 16)], 16, 3, K, 200, seed=900 + cg + K)
    if sub == "sharp":
        c.Wq[0] *= 30.0
        c.bq[0] *= 30.0
        return c
    base = reference_f64(c)[1]
    s = E_TARGET[sub] * F16_MAX / base["tokens" if sub == "tiny_wq" else sub]
    Wk = c.Wkv[0][:cg]
    if sub in ("tokens", "xbar", "tiny_wq"):
        for t in (c.xhat, c.Wpos, c.bpos):
            t *= s
        if sub == "tiny_wq":
            c.Wq[0] /= s * s
            c.bq[0] /= s
        else:
            fq = _shrink(c.Wq[0], 1.0 / s)
            c.bq[0] *= fq * s
            _shrink(Wk, 1.0 / (s * s * fq), c.scale)
    elif sub == "qp":
        c.Wq[0] *= s
        c.bq[0] *= s
        _shrink(Wk, 1.0 / s, c.scale)
    elif sub == "qt":
        for t in (c.xhat, c.Wpos, c.bpos):
            t /= s / 4.0
        c.Wq[0] *= s / 2.0
        c.bq[0] *= 2.0
        Wk *= s / 2.0
    else:
        c.Wkv[0][cg:] *= s
        c.bkv[0][cg:] *= s
    return c


def weights_above_split_floor(c):
    """Whether every matrix mssvt_attn_pack_weights splits keeps its largest entry >= SPLIT_FLOOR (Wk with the scale folded)."""
    least = []
    for (_, cg, _), Wq, Wkv, Wo in zip(c.groups, c.Wq, c.Wkv, c.Wo):
        least += [float(Wq.abs().max()), float(Wkv[:cg].abs().max()) * c.scale, float(Wkv[cg:].abs().max()), float(Wo.abs().max())]
    return min(least) >= SPLIT_FLOOR


def check_e_window(c, stats, sub):
    """The precondition of case (e), from the float64 reference's own figures."""
    assert weights_above_split_floor(c) == (sub != "tiny_wq")
    for W in c.Wq + c.Wkv + c.Wo:
        assert float(W.abs().max()) < 0.5 * F16_MAX  # the weights are operands too
    if sub == "sharp":
        assert 1e3 <= stats["score"] <= 1e5, stats
        assert max(stats[k] for k in E_QUANTITIES) < 0.5 * F16_MAX, stats
        return
    top = "tokens" if sub == "tiny_wq" else sub
    assert 0.5 * F16_MAX <= stats[top] <= 0.9 * F16_MAX, (sub, stats)
    for other in E_QUANTITIES:
        if other == top:
            continue
        if top == "xbar" and other == "tokens":
            assert stats["xbar"] <= stats["tokens"] <= 0.9 * F16_MAX, stats
        elif top == "tokens" and other == "xbar":
            assert stats["xbar"] <= stats["tokens"], stats  # (a convex combination of key tokens)
        else:
            assert stats[other] < stats[top], (sub, other, stats)


# ---------------------------------------------------------------------------------------------------------------------
# GPU side: work order, the four forms
# ---------------------------------------------------------------------------------------------------------------------
def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    from mssvt_amd import _lib
    return _lib.stream()


class OnGpu(object):
    """A case's tensors on the device, its work order from mssvt_plan_order (checked array by array), the reference."""

    def __init__(self, case, row_capacity=None):
        from mssvt_amd import _lib
        self.case = c = case
        to = lambda t: t.to(DEV).contiguous()  # noqa: E731
        for k, v in case.tensors().items():
            setattr(self, k, [to(t) for t in v] if isinstance(v, list) else to(v))
        self.row_cap = rc = max(c.total_rows, 1) if row_capacity is None else row_capacity
        i32 = lambda n, fill: torch.full(n, fill, dtype=torch.int32, device=DEV)  # noqa: E731
        self.num_wins = i32((1,), c.nw)
        self.perm, self.n_act, self.q_off, self.n_rows = i32((c.cap,), -7), i32((1,), -7), i32((c.cap,), -7), i32((1,), -7)
        self.row_meta = torch.full((rc, 4), float("nan"), dtype=torch.float32, device=DEV)
        self.row_src = i32((rc, 2), -7)
        st = _lib.lib().mssvt_plan_order(_P(self.num_wins), _P(self.nq_valid), ctypes.c_int(c.nq), _P(self.qmeta),
                                         ctypes.c_int(c.cap), ctypes.c_int(rc), _P(self.perm), _P(self.n_act),
                                         _P(self.q_off), _P(self.row_meta), _P(self.row_src), _P(self.n_rows), _stream())
        assert st == 0
        torch.cuda.synchronize()
        self.check_plan_order()
        self.width = sum(4 * ((h + 3) // 4) * cg for _, cg, h in c.groups)
        self.results = {}
        self.ref, self.stats = reference_f64(case, device=DEV, row_capacity=row_capacity)
        self.written = ~torch.isnan(self.ref)
        self._blobs = None

    def check_plan_order(self):
        """mssvt_plan_order against the statement of its contract (tests/window_plan_ref.py; include/mssvt_hip.h:324-336) on the
        same arrays.  nq <= 256 here, so min(nq_valid, 256) is nq_valid itself."""
        from tests.window_plan_ref import check_plan_order
        c = self.case
        assert c.nq <= 256
        np_ = lambda t: t.cpu().numpy()  # noqa: E731
        check_plan_order(np_(c.nq_valid), c.nw, c.nq, np_(c.qmeta.contiguous().view(torch.int32)), self.row_cap, np_(self.perm),
                         int(self.n_act.item()), np_(self.q_off), int(self.n_rows.item()), np_(self.row_src),
                         np_(self.row_meta.view(torch.int32)))

    def blobs(self):
        from mssvt_amd import _lib
        if self._blobs is None:
            c, lib = self.case, _lib.lib()
            self._blobs = []
            for gi, (_, cg, _) in enumerate(c.groups):
                n = int(lib.mssvt_attn_packed_bytes(ctypes.c_int(cg), ctypes.c_int(c.hd)))
                assert n > 0
                blob = torch.empty((n,), dtype=torch.uint8, device=DEV)
                st = lib.mssvt_attn_pack_weights(ctypes.c_int(cg), ctypes.c_int(c.hd), ctypes.c_float(c.scale), _P(self.Wq[gi]),
                                                 _P(self.Wkv[gi]), _P(self.Wo[gi]), _P(blob), _stream())
                assert st == 0
                self._blobs.append(blob)
        return self._blobs

    def run(self, form, fresh=False):
        """(status, attn): attn pre-filled with SENTINEL, qbuf with NaN."""
        from mssvt_amd import _lib
        if form in self.results and not fresh:
            return self.results[form]
        c, lib = self.case, _lib.lib()
        ia = lambda v: (ctypes.c_int * len(v))(*[int(x) for x in v])  # noqa: E731
        pa = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
        head = [ctypes.c_int(c.C), ctypes.c_int(len(c.groups)), ia([g[0] for g in c.groups]), ia([g[1] for g in c.groups]),
                ia([g[2] for g in c.groups]), ctypes.c_int(c.hd), ctypes.c_float(c.scale), ctypes.c_int(c.nq),
                ctypes.c_int(c.K), _P(self.xhat), _P(self.n_act), _P(self.perm), _P(self.q_off), _P(self.nq_valid),
                _P(self.n_rows), ctypes.c_int(self.row_cap), _P(self.row_meta), _P(self.row_src), pa(self.kmeta),
                _P(self.wcentre), pa(self.Wq), pa(self.bq), pa(self.Wkv), pa(self.bkv), pa(self.Wo), pa(self.bo),
                _P(self.Wpos), _P(self.bpos)]
        attn = torch.full((c.cap * c.nq + 1, c.C), SENTINEL, dtype=torch.float32, device=DEV)
        qbuf = torch.full((self.row_cap, self.width), float("nan"), dtype=torch.float32, device=DEV)
        if form == "fp32":
            st = lib.mssvt_block_attention(*head, _P(qbuf), _P(attn), _stream())
        elif form == "kv16":
            st = lib.mssvt_block_attention_kv16(*head, _P(qbuf), _P(attn), ctypes.c_void_p(0), _stream())
        elif form == "kv16_blobs":
            st = lib.mssvt_block_attention_kv16(*head, _P(qbuf), _P(attn), pa(self.blobs()), _stream())
        else:
            assert form == "bf16"
            st = lib.mssvt_block_attention_bf16(*head, _P(attn), _stream())
        torch.cuda.synchronize()
        self.results[form] = (int(st), attn)
        return self.results[form]


_cache = {}


def on_gpu(key, build, row_capacity=None):
    """The case of `key` on the device; the tests of one case follow each other, so one is kept."""
    if key not in _cache:
        _cache.clear()
        _cache[key] = OnGpu(build(), row_capacity)
    return _cache[key]


def forms_for(groups, hd, with_bf16=True):
    forms = ["fp32", "kv16"]
    if all((cg, hd) in BLOB_SHAPES for _, cg, _ in groups):
        forms.append("kv16_blobs")
    if with_bf16 and all((cg, hd) in bf16_shapes() for _, cg, _ in groups):
        forms.append("bf16")
    return forms


def sentinel_kept(g, attn):
    """Rows of invalid slots, row cap*nq and uncovered channels: bit for bit what they held before the call."""
    assert torch.equal(attn[~g.written], torch.full_like(attn[~g.written], SENTINEL))


def check_form(g, form, what):
    """Run `form` on the case, compare with float64 under the form's tolerance; for kv16 assert which launches ran."""
    c = g.case
    st, attn = g.run(form)
    assert st == 0, (what, form, st)
    sentinel_kept(g, attn)
    rows = int(g.written.any(1).sum())
    assert rows == int(g.n_rows.item())
    if rows == 0:
        print("RATIO %s %s rows=0" % (what, form))
        return
    got, ref = attn.double()[g.written], g.ref[g.written]
    err = (got - ref).abs()
    assert bool(torch.isfinite(got).all())
    if form == "bf16":
        mx = float(err.max() / ref.abs().max())
        rms = float((err.pow(2).mean() / ref.pow(2).mean()).sqrt())
        print("RATIO %s bf16 max/bound=%.3f rms/bound=%.3f rows=%d" % (what, mx / 5e-2, rms / 1e-2, rows))
        assert mx <= 5e-2 and rms <= 1e-2, (what, mx, rms)
        return
    tol = 1e-5 * ref.abs().max() + 1e-4 * ref.abs()
    ratio = float((err / tol).max())
    print("RATIO %s %s err/bound=%.3f rows=%d" % (what, form, ratio, rows))
    assert ratio <= 1.0, (what, form, ratio)
    if form != "fp32":
        which_form_ran(g, form, rows)


def which_form_ran(g, form, rows):
    """Columns of a head group on which the split-fp16 launches ran differ in bits from the fp32 launches' somewhere (given a
    few rows); a group that kept the fp32 form is bit-identical to mssvt_block_attention."""
    c = g.case
    st, base = g.run("fp32")
    assert st == 0
    _, attn = g.run(form)
    for c0, cg, _ in c.groups:
        same = torch.equal(attn[:, c0:c0 + cg], base[:, c0:c0 + cg])
        if kv16_runs(cg, c.K):
            assert not same or rows < 8, (form, c0, cg)
        else:
            assert same, (form, c0, cg)
    if form == "kv16_blobs" and rows >= 8 and all(kv16_runs(cg, c.K) for _, cg, _ in c.groups):
        assert not torch.equal(attn, g.run("kv16")[1])  # the row-tiled launches ran on the blobs


# ---- (a) every instantiated shape, every key tier -------------------------------------------------------------------
def _a_params():
    out = []
    for cg, hd in F32_SHAPES:
        for K in KEY_TIERS:
            for form in forms_for([(0, cg, cg // hd)], hd):
                out.append(pytest.param(cg, hd, K, form, id="%dx%d-K%d-%s" % (cg, hd, K, form)))
    return out


@pytest.mark.parametrize("cg,hd,K,form", _a_params())
def test_every_shape_and_key_tier_vs_float64(cg, hd, K, form):
    g = on_gpu(("a", cg, hd, K), lambda: case_a(cg, hd, K))
    check_form(g, form, "a %dx%d K%d" % (cg, hd, K))


def test_declined_shapes_return_toolarge():
    """What the parametrisations above leave out is declined by the library: bf16 at the two pairs only the fp32 kernels
    instantiate, blobs outside head_dim 16 / Cg 32, 64, and any form at more than 64 keys."""
    from mssvt_amd import _lib
    lib = _lib.lib()
    for cg, hd in F32_SHAPES:
        g = OnGpu(case_a(cg, hd, 8))
        st, attn = g.run("bf16")
        assert (st == 0) == ((cg, hd) in bf16_shapes()) and st in (0, E_TOOLARGE)
        if st:
            assert bool((attn == SENTINEL).all())
        n = int(lib.mssvt_attn_packed_bytes(ctypes.c_int(cg), ctypes.c_int(hd)))
        assert (n > 0) == ((cg, hd) in BLOB_SHAPES)
        if n == 0:
            junk = torch.empty((16,), dtype=torch.uint8, device=DEV)
            assert lib.mssvt_attn_pack_weights(ctypes.c_int(cg), ctypes.c_int(hd), ctypes.c_float(1.0), _P(g.Wq[0]), _P(g.Wkv[0]),
                                               _P(g.Wo[0]), _P(junk), _stream()) == E_TOOLARGE
    g = OnGpu(case_a(64, 16, 65))
    for form in ("fp32", "kv16", "kv16_blobs", "bf16"):
        st, attn = g.run(form)
        assert st == E_TOOLARGE and bool((attn == SENTINEL).all())
    g = OnGpu(make_case(20, [(0, 20, 1)], 20, 3, 8, 10))  # (20, 20): no instantiation
    for form in ("fp32", "kv16", "bf16"):
        assert g.run(form)[0] == E_TOOLARGE


# ---- (b) group layouts ------------------------------------------------------------------------------------------------
def _b_params():
    return [pytest.param(name, K, form, id="%s-K%d-%s" % (name, K, form)) for name in LAYOUTS for K in (32, 48)
            for form in forms_for(LAYOUTS[name][1], LAYOUTS[name][2])]


@pytest.mark.parametrize("layout,K,form", _b_params())
def test_group_layouts_vs_float64(layout, K, form):
    g = on_gpu(("b", layout, K), lambda: case_b(layout, K))
    c = g.case
    if len(c.groups) > 1:
        assert not torch.equal(c.kmeta[0], c.kmeta[1])  # every group attends to its own key lists
    covered = torch.zeros(c.C, dtype=torch.bool)
    for c0, cg, _ in c.groups:
        covered[c0:c0 + cg] = True
    assert bool(torch.isnan(g.ref[:, ~covered]).all())  # uncovered channels are never written (checked bit for bit below)
    check_form(g, form, "b %s K%d" % (layout, K))


# ---- (c) window structure ---------------------------------------------------------------------------------------------
def _c_params():
    return [pytest.param(name, cg, K, form, id="%s-%dx16-K%d-%s" % (name, cg, K, form)) for name in STRUCTURES
            for cg, K in C_SHAPES if structure_applies(name, K) for form in forms_for([(0, cg, cg // 16)], 16)]


@pytest.mark.parametrize("name,cg,K,form", _c_params())
def test_window_structures_vs_float64(name, cg, K, form):
    g = on_gpu(("c", name, cg, K), lambda: case_c(name, cg, K))
    c = g.case
    if name == "no_active_window":
        assert int(g.n_act.item()) == 0 and int(g.n_rows.item()) == 0 and not bool(g.written.any())
    if name.startswith("rows"):
        assert c.total_rows == int(name[4:])
    if name == "zero_query_windows_interleaved":
        assert int((c.nq_valid[:c.nw] == 0).sum()) >= c.nw // 2 and c.total_rows > 0
    check_form(g, form, "c %s %dx16 K%d" % (name, cg, K))


# ---- (d) pipeline depth -------------------------------------------------------------------------------------------------
def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("form", ["fp32", "kv16", "kv16_blobs"])
def test_more_windows_than_three_rounds_of_the_grid(K, form):
    g = on_gpu(("d", K), lambda: case_d(K, _cus()))
    assert g.case.nw == 3 * _cus() * 16 + 17 and int(g.n_rows.item()) > 2 * _cus() * 2 * 8 * 16
    check_form(g, form, "d K%d" % K)


@pytest.mark.parametrize("K", [32, 64])
@pytest.mark.parametrize("form", ["fp32", "kv16", "kv16_blobs"])
def test_a_window_past_the_row_capacity_is_dropped_whole(K, form):
    """row_capacity one row short of the last window's end: that window's rows stay unwritten (none of them holds a
    half-finished result), every other row is right, and nothing is written past the capacity (qbuf has exactly
    row_capacity rows)."""
    case = case_d(K, _cus())
    nqv = case.nq_valid[:case.nw]
    assert int(nqv[-1]) >= 2
    g = on_gpu(("d-short", K), lambda: case, row_capacity=case.total_rows - 1)
    last = slice((case.nw - 1) * case.nq, case.nw * case.nq)
    assert not bool(g.written[last].any()) and int(g.written.any(1).sum()) == case.total_rows - int(nqv[-1])
    check_form(g, form, "d-short K%d" % K)


# ---- (e) operands near the top of the fp16 range ------------------------------------------------------------------------
@pytest.mark.parametrize("cg,K", E_SHAPES)
@pytest.mark.parametrize("sub", E_SUBCASES)
@pytest.mark.parametrize("form", ["kv16", "kv16_blobs"])
def test_split_fp16_forms_near_the_top_of_the_fp16_range(cg, K, sub, form):
    g = on_gpu(("e", cg, K, sub), lambda: case_e(cg, K, sub))
    from mssvt_amd import fused
    c = g.case
    check_e_window(c, g.stats, sub)
    # the caller's guard hands out blobs exactly where every split matrix resolves its entries
    assert (float(fused._attn_fragment_floor(c.Wq, c.Wkv, c.Wo, c.scale)) >= fused.ATTN_F16_FLOOR) == (sub != "tiny_wq")
    if not hasattr(g, "e32"):
        ref32 = reference(g.case, dtype=torch.float32, device=DEV)[0]
        g.e32 = (ref32.double() - g.ref)[g.written].abs()
    st, attn = g.run(form)
    assert st == 0
    sentinel_kept(g, attn)
    got = attn.double()[g.written]
    assert bool(torch.isfinite(got).all())
    err = (got - g.ref[g.written]).abs()
    r_max, r_mean = float(err.max() / g.e32.max()), float(err.mean() / g.e32.mean())
    print("RATIO e %dx16 K%d %s %s max/e32=%.3f mean/e32=%.3f (max e32 / max|ref| = %.2e, max|score| = %.3g)"
          % (cg, K, sub, form, r_max, r_mean, float(g.e32.max() / g.ref[g.written].abs().max()), g.stats["score"]))
    if (sub, form) == ("tiny_wq", "kv16_blobs"):
        # measured 56 .. 124: fragments of magnitude 1e-7 sit below the 2^-35 floor of the split halves.  The guard asserted
        # above never hands such blobs to the entry point; what it runs instead is the `kv16` form of this same case.
        assert fused.ATTN_F16_FLOOR == SPLIT_FLOOR
    else:
        assert r_max <= MAX_RATIO and r_mean <= MAX_RATIO, (sub, form, r_max, r_mean)
    which_form_ran(g, form, int(g.n_rows.item()))


def test_guard_keeps_projections_below_the_split_floor_off_the_blobs():
    """fused._attn_kv16_ok: a projection whose largest entry is below 2^-13 keeps the split-fp16 window launch (its operands
    are in range) but gets no pre-split fragments -- the row-tiled launches stay on the fp32 instruction."""
    from mssvt_amd import config, fused
    torch.manual_seed(0)
    net = config.build_backbone_from_cfg().to(DEV).eval()
    blk = net.backbone[0]

    class P(object):
        coord_bound = 80.0
    r = fused._attn_refs(blk, None)
    assert fused._attn_kv16_ok(blk, r, P) and r["kv16_packed"] is not None
    with torch.no_grad():
        blk.ms_attn.to_qs[0].weight.mul_(1.0e-6)
    r = fused._attn_refs(blk, None)
    assert fused._attn_kv16_ok(blk, r, P) and r["kv16_packed"] is None


# ---- (f) hygiene ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cg,K", C_SHAPES)
@pytest.mark.parametrize("form", ["fp32", "kv16", "kv16_blobs", "bf16"])
def test_stale_memory_is_ignored_and_runs_repeat_bit_for_bit(cg, K, form):
    """The longest list of (c) (nq = 45): qbuf arrives full of NaN and attn full of a sentinel (OnGpu.run), 64 MB of NaN were
    just freed; rows of invalid slots and row cap * nq keep the sentinel; two runs give the same bits."""
    g = on_gpu(("c", "nq45", cg, K), lambda: case_c("nq45", cg, K))
    junk = torch.full((16 << 20,), float("nan"), dtype=torch.float32, device=DEV)
    del junk
    st1, a1 = g.run(form, fresh=True)
    st2, a2 = g.run(form, fresh=True)
    assert st1 == 0 and st2 == 0
    sentinel_kept(g, a1)
    assert bool((a1[g.case.cap * g.case.nq] == SENTINEL).all())
    assert torch.equal(a1, a2) and bool(torch.isfinite(a1[g.written]).all())
    check_form(g, form, "f nq45 %dx16 K%d" % (cg, K))
