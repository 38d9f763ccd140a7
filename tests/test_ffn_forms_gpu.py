"""Every launch form of the FFN tail (csrc/ffn.hip) against a float64 restatement of include/mssvt_hip.h:541-562, 588-597.

The C entry points are driven directly (mssvt_ffn_fused, mssvt_ffn_fused_interp, mssvt_ffn_pack_weights): a case is a
seeded set of rows whose count is computed from the device's CU count with the launchers' own formulas, so that every
regime of the two software pipelines exists -- k_ffn_ws at 1, 2, 3 and >= 4 tiles per workgroup and on both sides of the
XCD-contiguous dealing, k_ffn_up / k_ffn_down with idle waves, one tile per wave, one looping wave and a steady state.

Kernels reached (15 k_ffn_ws = 3 shapes x 5 template forms, 3 x 2 two-launch kernels), by parametrised id:
  ws-plain-norm-*, ws-owner-norm-*        k_ffn_ws<C, FF, TABBED=false, NORM2=true>
  ws-plain-nonorm-*, ws-owner-nonorm-*    k_ffn_ws<C, FF, false, false>       (plain-nonorm = the CompressBlock tail of the frame)
  ws-table-norm-*                         k_ffn_ws<C, FF, true, true>
  ws-table-nonorm-*                       k_ffn_ws<C, FF, true, false>
  ws-table-noy                            k_ffn_ws<C, FF, true, true, STOREY=false>
  (*-packed: fragments of k_ffn_pack<C, FF>; *-unpacked: hidden = NULL, split in the kernel's prologue)
  split-{plain,owner,table}-{norm,nonorm} k_ffn_up<C, FF> + k_ffn_down<C, FF>  (phases = 3), table-fed for `table`
each at C x FF = 128x256, 64x128, 32x64.

Tolerances, per row: s_r = max(1, max_c |want[r, c]|), errors of y are divided by s_r (never by a global maximum)
  phases 4, plain / owner     |y - want| <= 4e-6 s_r,  |y_norm - want_n| <= 2e-5       (the bounds of test_fused_gpu.py)
  phases 4, table             6e-6 s_r and 3e-5
  phases 3                    max(err / s_r) <= 4 max(e32 / s_r) + 1e-6,  mean(err / s_r) <= 4 mean(e32 / s_r), for y and
                              y_norm alike; e32 = |float32 torch evaluation of the same formulas - float64| (re-association
                              of the 16x16x4 MFMA chains, hardware rsqrt)
  near_f16_top (phases 4)     max <= 8 max(e32), mean <= 8 mean(e32) (same scaling): the split keeps 22 of 24 mantissa
                              bits = 4 rounding units, re-association and rsqrt another factor 2
Input classes (builder modes): `mixed` (rows scaled by 10^U(-3,3), 2 % zero rows, 20 % unowned, table rows with three
distinct attention rows / one row three times / weight-0 slots on the zero row), `nan_unreferenced` (every attention row
no owned voxel references with a non-zero weight is NaN), `all_unowned`, `all_owned`, `near_f16_top_ln` (LayerNorm weight
scaled: max|LN(x)| = 0.6 x 65504) and `near_f16_top_hidden` (W1 scaled: max|hidden| = 0.6 x 65504).  In the last two b2
is scaled with the branch, so that the bias stays a visible part of the output.
Tolerance-free properties: rows in [n, capacity) keep a sentinel under a device row count and rows below it equal the
host-count launch bit for bit; fragments packed once = split in the prologue; two launches agree; every row of the
largest launch equals the same row computed by a launch in which its workgroup (wave) does that one tile only.
tests/test_ffn_ref_cpu.py checks the reference itself without a GPU.

Measured on the MI355X (256 CUs), worst over all cases of a kind, error / bound (every test prints its own RATIO line):
  phases 4, plain / owner     y 0.23, y_norm 0.11            phases 4, table     y 0.15, y_norm 0.09
  phases 3                    y max 0.21 mean 0.30, y_norm max 0.23 mean 0.31 -- i.e. 0.9 x max(e32), 1.2 x mean(e32)
  near_f16_top_ln             y max 0.28 mean 0.46, y_norm max 0.25 mean 0.27 -- i.e. at most 2.3 x max, 3.7 x mean(e32)
  near_f16_top_hidden         y max 0.33 mean 0.44, y_norm max 0.24 mean 0.26 -- i.e. at most 2.7 x max, 3.5 x mean(e32)
The tolerance-free properties held on every form, shape and count; nothing in csrc/ffn.hip had to change.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"

F16_MAX = 65504.0
E_BADARG, E_TOOLARGE = -1, -2
SENTINEL = -12345.678
SHAPES = [(128, 256), (64, 128), (32, 64)]
EPS1, EPS2 = 1e-5, 1e-3  # norm2 and the next block's norm1: different, so that swapping them shows
SOURCES = ("plain", "owner", "table")
TOP_CLASSES = ("near_f16_top_ln", "near_f16_top_hidden")
CLASSES = ("mixed", "nan_unreferenced", "all_unowned", "all_owned") + TOP_CLASSES
MUTATIONS = ("unowned_once", "drop_w3", "drop_b2", "relu_skip_last_tile", "swap_eps", "norm_of_branch")
TOP_TARGET = 0.6  # x 65504: inside [0.5, 0.9], and the caller's guard (a bound, not the value) still accepts
TOP_RATIO = 8.0
SPLIT_RATIO = 4.0


# ---------------------------------------------------------------------------------------------------------------------
# 1. input builder (torch, seeded, CPU tensors; nothing here needs a GPU)
# ---------------------------------------------------------------------------------------------------------------------
class Case(object):
    """C, FF, n (rows), cap (rows allocated; rows [n, cap) hold NaN features), source, cls; the residual source of the
    form under test -- plain: x_new; owner: x_new, x_in, owner (cap) int32; table: x_in, attn (R + 1, C) with zero_row = R,
    tab_row (cap,4) int32, tab_w (cap,4) -- and ln_w, ln_b, eps (norm2), W1 (FF,C), b1, W2 (C,FF), b2, ln2_w, ln2_b, eps2."""
    NAMES = ("x_new", "x_in", "owner", "tab_row", "tab_w", "attn", "ln_w", "ln_b", "W1", "b1", "W2", "b2", "ln2_w", "ln2_b")

    def tensors(self):
        return dict((k, getattr(self, k)) for k in self.NAMES)


def _uniform(g, shape, bound):
    return (torch.rand(shape, generator=g) * 2 - 1) * bound


def _linear(g, out_f, in_f):
    """nn.Linear default init: weight and bias uniform in +-1/sqrt(fan_in)."""
    b = 1.0 / math.sqrt(in_f)
    return _uniform(g, (out_f, in_f), b), _uniform(g, (out_f,), b)


def _features(g, rows, C):
    x = torch.randn(rows, C, generator=g) * 10.0 ** (torch.rand(rows, 1, generator=g) * 6.0 - 3.0)
    x[torch.rand(rows, generator=g) < 0.02] = 0.0
    return x


def make_case(C, FF, n, source, cls="mixed", cap=None, seed=0):
    assert source in SOURCES and cls in CLASSES and n >= 0
    assert cls != "nan_unreferenced" or source == "table"
    g = torch.Generator().manual_seed(7000 + 31 * seed + C + n % 1009)
    c = Case()
    cap = max(n, 1) if cap is None else cap
    assert cap >= max(n, 1)
    c.C, c.FF, c.n, c.cap, c.source, c.cls = C, FF, n, cap, source, cls
    c.W1, c.b1 = _linear(g, FF, C)
    c.W2, c.b2 = _linear(g, C, FF)
    c.ln_w, c.ln_b = 1.0 + _uniform(g, (C,), 0.1), _uniform(g, (C,), 0.1)
    c.ln2_w, c.ln2_b = 1.0 + _uniform(g, (C,), 0.1), _uniform(g, (C,), 0.1)
    c.eps, c.eps2 = EPS1, EPS2
    c.x_new = c.x_in = c.owner = c.tab_row = c.tab_w = c.attn = None
    c.zero_row = -1
    unowned = torch.rand(cap, generator=g) < {"all_unowned": 2.0, "all_owned": -1.0}.get(cls, 0.2)
    if source != "table":
        c.x_new = _features(g, cap, C)
    if source == "owner":
        c.x_in = _features(g, cap, C)
        c.owner = torch.randint(0, 3, (cap,), generator=g).to(torch.int32)
        c.owner[unowned] = -1
    if source == "table":
        R = n + 8
        c.zero_row = R
        c.x_in = _features(g, cap, C)
        c.attn = _features(g, R + 1, C)
        c.attn[R] = 0.0
        c.tab_row = torch.randint(0, R, (cap, 4), generator=g).to(torch.int32)
        c.tab_w = 0.05 + torch.rand(cap, 4, generator=g)
        kind = torch.randint(0, 3, (cap,), generator=g)  # 0: three distinct rows
        c.tab_row[kind == 1, 1:3] = c.tab_row[kind == 1, 0:1]  # one row in all three slots
        c.tab_row[kind == 2, 1:3] = R  # weight-0 slots point at the zero row
        c.tab_w[kind == 2, 1:3] = 0.0
        c.tab_row[unowned] = -1
    if cls in TOP_CLASSES:
        _near_f16_top(c, g)
    if cls == "nan_unreferenced":
        used = torch.zeros(c.zero_row + 1, dtype=torch.bool)
        tr, tw = c.tab_row[:n].long(), c.tab_w[:n]
        for i in range(3):
            sel = (tr[:, 0] >= 0) & (tw[:, i] != 0)
            used[tr[sel, i]] = True
        used[c.zero_row] = True
        c.attn[~used] = float("nan")
    for t in (c.x_new, c.x_in, c.tab_w):  # a read past the device row count shows up as a NaN
        if t is not None:
            t[n:] = float("nan")
    check_invariants(c)
    return c


def _set_row(c, row, x):
    """Row `row` gets the residual input x exactly: through x_new, or as an unowned voxel (2 x_in)."""
    if c.source == "plain":
        c.x_new[row] = x
    else:
        c.x_in[row] = 0.5 * x
        if c.source == "owner":
            c.owner[row] = -1
        else:
            c.tab_row[row] = -1


def _near_f16_top(c, g):
    """ln: every 37th row is one-hot at the channel of the largest LayerNorm weight (|LN(x)| ~ sqrt(C - 1) |w|: the largest
    value a LayerNorm can give, which keeps the guard's bound sqrt(C) max|w| + max|b| next to the value itself), then ln_w
    is scaled so that max|LN(x)| = TOP_TARGET x 65504.  hidden: every 37th row is aligned with one of the four W1 rows of
    the largest norm (x = W1_h * ln_w minus its mean: the direction that maximises hidden unit h), then W1 is scaled so
    that max|hidden| = TOP_TARGET x 65504.  b2 follows the branch in both."""
    rows = torch.arange(3, c.n, 37)
    mag = 10.0 ** (torch.rand(rows.numel(), generator=g) * 2.0 - 1.0)
    if c.cls == "near_f16_top_ln":
        ch = int(c.ln_w.abs().argmax())
        for k, r in enumerate(rows.tolist()):
            x = torch.zeros(c.C)
            x[ch] = float(mag[k]) * (1.0 if k % 2 else -1.0)
            _set_row(c, r, x)
        s = TOP_TARGET * F16_MAX / reference_f64(c)[2]["ln"]
        c.ln_w *= s
    else:
        z = c.W1 * c.ln_w
        z = z - z.mean(1, keepdim=True)
        top = z.norm(dim=1).topk(4).indices.tolist()
        for k, r in enumerate(rows.tolist()):
            _set_row(c, r, z[top[k % 4]] * float(mag[k]))
        s = TOP_TARGET * F16_MAX / reference_f64(c)[2]["hidden"]
        c.W1 *= s
    c.b2 *= s


def check_invariants(c):
    """What the kernels' contract asks of the caller, also on the rows past n: no case may leave it."""
    for k in ("x_new", "x_in", "tab_w"):
        t = getattr(c, k)
        if t is not None:
            assert t.shape[0] == c.cap and bool(torch.isfinite(t[:c.n]).all()) and bool(torch.isnan(t[c.n:]).all())
    if c.source == "owner":
        assert c.owner.shape == (c.cap,) and c.owner.dtype == torch.int32
    if c.source == "table":
        assert c.tab_row.shape == (c.cap, 4) and c.tab_row.dtype == torch.int32 and c.attn.shape == (c.zero_row + 1, c.C)
        assert bool(((c.tab_row >= -1) & (c.tab_row <= c.zero_row)).all())
        assert bool((c.attn[c.zero_row] == 0).all())
        tr = c.tab_row[:c.n].long()
        owned = tr[:, 0] >= 0
        assert bool((tr[owned, :3] >= 0).all())
        live = c.attn[tr[owned, :3]]  # rows an owned voxel gathers: finite wherever the weight is not zero
        assert bool(torch.isfinite(live[c.tab_w[:c.n][owned, :3] != 0]).all())
        if c.cls == "nan_unreferenced":
            assert bool(torch.isnan(c.attn).any()) or c.n < 8
    for t in (c.ln_w, c.ln_b, c.W1, c.b1, c.W2, c.b2, c.ln2_w, c.ln2_b):
        assert bool(torch.isfinite(t).all())


# ---------------------------------------------------------------------------------------------------------------------
# 2. reference
# ---------------------------------------------------------------------------------------------------------------------
def _layer_norm(x, w, b, eps):
    mean = x.mean(1, keepdim=True)
    d = x - mean
    return d / torch.sqrt((d * d).mean(1, keepdim=True) + eps) * w + b


def reference(case, dtype=torch.float64, device="cpu", mutate=None, chunk=1 << 17):
    """(y, y_norm, stats) over the rows [0, n) in `dtype`; stats = max|LN(x)| and max|hidden| (hidden = relu(W1 LN(x) + b1),
    the operand of the second product).  `mutate` evaluates a deliberately wrong formula (tests/test_ffn_ref_cpu.py)."""
    c = case
    f = lambda t: t.to(device).to(dtype)  # noqa: E731
    ln_w, ln_b, W1, b1, W2, b2, ln2_w, ln2_b = [f(t) for t in (c.ln_w, c.ln_b, c.W1, c.b1, c.W2, c.b2, c.ln2_w, c.ln2_b)]
    eps, eps2 = (c.eps2, c.eps) if mutate == "swap_eps" else (c.eps, c.eps2)
    twice = 1.0 if mutate == "unowned_once" else 2.0
    attn = f(c.attn) if c.source == "table" else None
    y = torch.empty((c.n, c.C), dtype=dtype, device=device)
    yn = torch.empty((c.n, c.C), dtype=dtype, device=device)
    stats = dict(ln=0.0, hidden=0.0)
    for r0 in range(0, c.n, chunk):
        sl = slice(r0, min(c.n, r0 + chunk))
        if c.source == "plain":
            x = f(c.x_new[sl])
        elif c.source == "owner":
            x = torch.where((c.owner[sl].to(device) >= 0)[:, None], f(c.x_new[sl]), twice * f(c.x_in[sl]))
        else:
            tr, tw, x_in = c.tab_row[sl].to(device).long(), f(c.tab_w[sl]), f(c.x_in[sl])
            idx = tr[:, :3].clamp(min=0)
            upd = tw[:, 0:1] * attn[idx[:, 0]] + tw[:, 1:2] * attn[idx[:, 1]]
            if mutate != "drop_w3":
                upd = upd + tw[:, 2:3] * attn[idx[:, 2]]
            x = torch.where((tr[:, 0] >= 0)[:, None], x_in + upd, twice * x_in)
        h = _layer_norm(x, ln_w, ln_b, eps)
        u = h @ W1.T + b1
        if mutate == "relu_skip_last_tile":
            u = torch.cat([torch.relu(u[:, :c.FF - 16]), u[:, c.FF - 16:]], 1)
        else:
            u = torch.relu(u)
        yy = x + u @ W2.T
        if mutate != "drop_b2":
            yy = yy + b2
        y[sl] = yy
        yn[sl] = _layer_norm(yy - x if mutate == "norm_of_branch" else yy, ln2_w, ln2_b, eps2)
        if sl.stop > sl.start:
            stats["ln"] = max(stats["ln"], float(h.abs().max()))
            stats["hidden"] = max(stats["hidden"], float(u.abs().max()))
    return y, yn, stats


def reference_f64(case, **kw):
    return reference(case, dtype=torch.float64, **kw)


def row_scale(want):
    return want.abs().amax(1, keepdim=True).clamp(min=1.0)


def check_top_window(c, stats):
    """The precondition of the near_f16_top classes, from the float64 reference's own figures."""
    top, other = ("ln", "hidden") if c.cls == "near_f16_top_ln" else ("hidden", "ln")
    assert 0.5 * F16_MAX <= stats[top] <= 0.9 * F16_MAX, (c.cls, stats)
    assert stats[other] < 0.5 * F16_MAX, (c.cls, stats)
    for W in (c.W1, c.W2):
        assert float(W.abs().max()) < 0.5 * F16_MAX  # the weights are operands too


# ---------------------------------------------------------------------------------------------------------------------
# 3. row counts: the launchers' own formulas
# ---------------------------------------------------------------------------------------------------------------------
def ws_grid(C, FF, cus):
    """launch_ffn_ws (csrc/ffn.hip:975-977): grid = min(cus * (NW >= 8 ? 1 : 8 / NW), tiles), NW = FF / 32; k_ffn_ws
    (:614-620) deals XCD-contiguous when gridDim % 8 == 0 and tiles >= 8 * gridDim."""
    return cus * max(1, 8 // (FF // 32))


def split_grid(C, FF, cus):
    """launch_ffn_split (csrc/ffn.hip:1017, :1034-1036): grid = min(cus * (160 KiB / max(lds_up, lds_down)), tiles); one
    wave per tile, tile k * grid + block on wave k, stride 8 * grid (k_ffn_up :189, :217)."""
    lds_up, lds_down = (FF * (C + 4) + FF + 2 * C) * 4, (C * (FF + 4) + 3 * C) * 4
    return cus * (163840 // max(lds_up, lds_down))


# name -> rows(G).  ws: one partial tile | one full tile | two workgroups, the second with one row | 1, 2, 3, 4, 5 tiles on
# the busiest workgroup | one tile below the dealing threshold | on it | per_xcd not dividing the tiles: the last XCD 6 tiles
# short | 2 tiles short
WS_COUNTS = {
    "1": lambda G: 1, "15": lambda G: 15, "16": lambda G: 16, "17": lambda G: 17,
    "16G-1": lambda G: 16 * G - 1, "16G+1": lambda G: 16 * G + 1, "32G+5": lambda G: 32 * G + 5,
    "48G+5": lambda G: 48 * G + 5, "64G+55": lambda G: 64 * G + 55, "16(8G-1)-3": lambda G: 16 * (8 * G - 1) - 3,
    "128G": lambda G: 128 * G, "16(8G+1)+9": lambda G: 16 * (8 * G + 1) + 9, "16(8G+13)+1": lambda G: 16 * (8 * G + 13) + 1,
}
# two launches: one tile | two | waves 1..7 idle | every wave exactly one tile | one wave loops | steady state
SPLIT_COUNTS = {
    "1": lambda G: 1, "17": lambda G: 17, "16G+1": lambda G: 16 * G + 1, "16*8G-3": lambda G: 16 * 8 * G - 3,
    "16*8G+17": lambda G: 16 * 8 * G + 17, "16*20G+5": lambda G: 16 * 20 * G + 5,
}
SPLIT_REGIMES = tuple(SPLIT_COUNTS)
SPLIT_COUNTS["48G+5"] = lambda G: 48 * G + 5  # waves 0..3 of a workgroup: the count every form runs at
WS_FOUR = ("17", "16G+1", "48G+5", "16(8G+1)+9")
SPLIT_FOUR = ("17", "16G+1", "48G+5", "16*8G+17")


def ws_regime(n, G):
    """(grid, tiles of the busiest workgroup, dealt XCD-contiguous) of a k_ffn_ws launch over n rows."""
    tiles = (n + 15) // 16
    grid = min(G, tiles)
    if grid % 8 == 0 and tiles >= 8 * grid:
        per_xcd, step = (tiles + 7) // 8, grid // 8
        return grid, (per_xcd + step - 1) // step, True
    return grid, (tiles + grid - 1) // grid, False


def split_regime(n, G):
    """(grid, waves of workgroup 0 with a tile, tiles of the busiest wave)."""
    tiles = (n + 15) // 16
    grid = min(G, tiles)
    return grid, min(8, (tiles + grid - 1) // grid), (tiles + 8 * grid - 1) // (8 * grid)


# ---------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------
def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def grid_of(kernel, C, FF):
    return (ws_grid if kernel == "ws" else split_grid)(C, FF, _cus())


def rows_of(kernel, C, FF, count):
    return (WS_COUNTS if kernel == "ws" else SPLIT_COUNTS)[count](grid_of(kernel, C, FF))


class Form(object):
    """kernel "ws" (phases 4) or "split" (phases 3); source; norm: with y_norm; packed: fragments of
    mssvt_ffn_pack_weights as `hidden` (ws); store_y False: y = NULL."""

    def __init__(self, kernel, source, norm, packed=True, store_y=True):
        self.kernel, self.source, self.norm, self.packed, self.store_y = kernel, source, norm, packed, store_y
        self.phases = 4 if kernel == "ws" else 3
        self.id = "%s-%s-%s" % (kernel, source, "noy" if not store_y else ("norm" if norm else "nonorm"))
        if kernel == "ws" and store_y:
            self.id += "-packed" if packed else "-unpacked"


WS_FORMS = [Form("ws", s, nm, pk) for s in SOURCES for nm in (True, False) for pk in (True, False)] + \
           [Form("ws", "table", True, True, store_y=False)]
SPLIT_FORMS = [Form("split", s, nm) for s in SOURCES for nm in (True, False)]
FORMS = dict((f.id, f) for f in WS_FORMS + SPLIT_FORMS)
WS_MAIN, SPLIT_MAIN, WS_FRAME = "ws-table-norm-packed", "split-table-norm", "ws-plain-nonorm-packed"


class Run(object):
    pass


class OnGpu(object):
    """A case's tensors on the device and its float64 reference (computed once, shared by the tests of the case)."""

    def __init__(self, case):
        self.case = c = case
        for k, v in c.tensors().items():
            setattr(self, k, None if v is None else v.to(DEV).contiguous())
        self.y_ref, self.yn_ref, self.stats = reference_f64(c, device=DEV)
        self._packed = self._e32 = None
        self.results = {}

    def packed(self):
        from mssvt_amd import _lib
        if self._packed is None:
            c, lib = self.case, _lib.lib()
            nbytes = int(lib.mssvt_ffn_packed_bytes(c.C, c.FF))
            assert nbytes == 2 * 2 * c.C * c.FF * 2  # hi + lo halves of both matrices
            self._packed = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
            assert lib.mssvt_ffn_pack_weights(c.C, c.FF, self.W1.data_ptr(), self.W2.data_ptr(), self._packed.data_ptr(),
                                              _lib.stream()) == 0
        return self._packed

    def e32(self):
        """|float32 evaluation - float64| / s_r for y and y_norm."""
        if self._e32 is None:
            y32, yn32, _ = reference(self.case, dtype=torch.float32, device=DEV)
            self._e32 = ((y32.double() - self.y_ref).abs() / row_scale(self.y_ref),
                         (yn32.double() - self.yn_ref).abs() / row_scale(self.yn_ref))
        return self._e32

    def buffers(self, form, rows):
        y = torch.full((rows, self.case.C), SENTINEL, dtype=torch.float32, device=DEV)
        yn = torch.full((rows, self.case.C), SENTINEL, dtype=torch.float32, device=DEV)
        hidden = torch.full((rows, self.case.FF), SENTINEL, dtype=torch.float32, device=DEV) if form.phases == 3 else None
        return y, yn, hidden

    def launch(self, form, r0=0, n_rows=None, n_dev=None, out=None, C=None, FF=None, phases=None, hidden_null=False,
               y_null=None, norm=None):
        """One call of the entry point of `form` on the rows [r0, r0 + n_rows) of the case: every row pointer is offset by
        r0, attn stays whole.  out: (y, y_norm, hidden) to write into (at row r0); default: fresh buffers of
        n_rows + 32 rows pre-filled with SENTINEL.  The keyword overrides build the declined calls."""
        from mssvt_amd import _lib
        c, lib = self.case, _lib.lib()
        n_rows = c.n - r0 if n_rows is None else n_rows
        y, yn, hidden = out if out is not None else self.buffers(form, n_rows + 32)
        at = lambda t: None if t is None else t[r0:].data_ptr()  # noqa: E731
        norm = form.norm if norm is None else norm
        y_null = (not form.store_y) if y_null is None else y_null
        if form.phases == 4:
            ws = self.packed().data_ptr() if form.packed else None
        else:
            ws = None if hidden_null else at(hidden)
        dev = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
        tail = [self.ln_w.data_ptr(), self.ln_b.data_ptr(), c.eps, self.W1.data_ptr(), self.b1.data_ptr(),
                self.W2.data_ptr(), self.b2.data_ptr(), None if y_null else at(y),
                self.ln2_w.data_ptr() if norm else None, self.ln2_b.data_ptr() if norm else None, c.eps2,
                at(yn) if norm else None, ws, None if dev is None else dev.data_ptr(),
                form.phases if phases is None else phases, _lib.stream()]
        head = [n_rows, c.C if C is None else C, c.FF if FF is None else FF]
        if c.source == "table":
            st = lib.mssvt_ffn_fused_interp(*(head + [at(self.x_in), at(self.tab_row), at(self.tab_w), self.attn.data_ptr()] + tail))
        else:
            st = lib.mssvt_ffn_fused(*(head + [at(self.x_new), at(self.x_in), at(self.owner)] + tail))
        torch.cuda.synchronize()
        r = Run()
        r.st, r.y, r.yn, r.hidden, r.n_rows = int(st), y, yn, hidden, n_rows
        return r

    def run(self, form):
        """The whole case through `form`, once."""
        if form.id not in self.results:
            assert form.source == self.case.source
            self.results[form.id] = self.launch(form)
        return self.results[form.id]


_cache = {}


def on_gpu(C, FF, n, source, cls="mixed", cap=None):
    """The case on the device; the tests of one case follow each other, so one is kept."""
    key = (C, FF, n, source, cls, cap)
    if key not in _cache:
        _cache.clear()
        _cache[key] = OnGpu(make_case(C, FF, n, source, cls, cap=cap))
    return _cache[key]


def check_outputs(g, form, r, what):
    """`r` of the whole case against float64 under the form's tolerance; rows past n keep the sentinel."""
    c = g.case
    assert r.st == 0, (what, r.st)
    outs = []
    if form.store_y:
        outs.append(("y", r.y, g.y_ref))
    else:
        assert bool((r.y == SENTINEL).all())
    if form.norm:
        outs.append(("y_norm", r.yn, g.yn_ref))
    else:
        assert bool((r.yn == SENTINEL).all())
    for name, got, want in outs:
        assert bool((got[c.n:] == SENTINEL).all()), (what, name)
        got = got[:c.n].double()
        assert bool(torch.isfinite(got).all()), (what, name)
        if c.n == 0:
            continue
        err = (got - want).abs()
        if c.cls in TOP_CLASSES or form.phases == 3:
            e32 = g.e32()[0 if name == "y" else 1]
            err = err / row_scale(want)
            k, add = (TOP_RATIO, 0.0) if c.cls in TOP_CLASSES else (SPLIT_RATIO, 1e-6)
            r_max = float(err.max()) / (k * float(e32.max()) + add)
            r_mean = float(err.mean()) / (k * float(e32.mean()))
            print("RATIO %s %s %s max/bound=%.3f mean/bound=%.3f (max e32 %.2e)" % (what, form.id, name, r_max, r_mean, float(e32.max())))
            assert r_max <= 1.0 and r_mean <= 1.0, (what, form.id, name, r_max, r_mean)
        else:
            ty, tn = (6e-6, 3e-5) if c.source == "table" else (4e-6, 2e-5)
            ratio = float((err / row_scale(want)).max()) / ty if name == "y" else float(err.max()) / tn
            print("RATIO %s %s %s err/bound=%.3f" % (what, form.id, name, ratio))
            assert ratio <= 1.0, (what, form.id, name, ratio)


def _what(C, FF, count, cls="mixed"):
    return "%dx%d n=%s %s" % (C, FF, count, cls)


def _ids(v):
    return "%dx%d" % v if isinstance(v, tuple) else str(v)


# ---- every form at four counts ------------------------------------------------------------------------------------------
def _form_params(forms, counts):
    return [pytest.param(C, FF, count, f.id, id="%dx%d-%s-%s" % (C, FF, count, f.id))
            for C, FF in SHAPES for count in counts for s in SOURCES for f in forms if f.source == s]


@pytest.mark.parametrize("C,FF,count,form", _form_params(WS_FORMS, WS_FOUR) + _form_params(SPLIT_FORMS, SPLIT_FOUR))
def test_every_form_vs_float64(C, FF, count, form):
    form = FORMS[form]
    g = on_gpu(C, FF, rows_of(form.kernel, C, FF, count), form.source)
    check_outputs(g, form, g.run(form), _what(C, FF, count))


# ---- every count on one form per kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("C,FF,count", [pytest.param(C, FF, k, id="%dx%d-%s" % (C, FF, k)) for C, FF in SHAPES for k in WS_COUNTS])
def test_ws_every_regime_of_the_pipeline_vs_float64(C, FF, count):
    G, n = grid_of("ws", C, FF), rows_of("ws", C, FF, count)
    assert G % 8 == 0  # the dealing needs it (256 CUs)
    grid, per_wg, dealt = ws_regime(n, G)
    want = {"1": (1, 1, False), "15": (1, 1, False), "16": (1, 1, False), "17": (2, 1, False), "16G-1": (G, 1, False),
            "16G+1": (G, 2, False), "32G+5": (G, 3, False), "48G+5": (G, 4, False), "64G+55": (G, 5, False),
            "16(8G-1)-3": (G, 8, False), "128G": (G, 8, True), "16(8G+1)+9": (G, 9, True), "16(8G+13)+1": (G, 9, True)}[count]
    assert (grid, per_wg, dealt) == want, (count, grid, per_wg, dealt)
    tiles = (n + 15) // 16
    if dealt and count != "128G":  # per_xcd = ceil(tiles / 8) does not divide the tiles: the last XCD's eighth ends early
        assert tiles % ((tiles + 7) // 8) != 0 and 8 * ((tiles + 7) // 8) - tiles in (6, 2)
    g = on_gpu(C, FF, n, "table")
    check_outputs(g, FORMS[WS_MAIN], g.run(FORMS[WS_MAIN]), _what(C, FF, count))


@pytest.mark.parametrize("C,FF,count", [pytest.param(C, FF, k, id="%dx%d-%s" % (C, FF, k)) for C, FF in SHAPES
                                        for k in SPLIT_REGIMES])
def test_split_every_regime_of_the_wave_loop_vs_float64(C, FF, count):
    G, n = grid_of("split", C, FF), rows_of("split", C, FF, count)
    want = {"1": (1, 1, 1), "17": (2, 1, 1), "16G+1": (G, 2, 1), "16*8G-3": (G, 8, 1), "16*8G+17": (G, 8, 2),
            "16*20G+5": (G, 8, 3)}[count]
    assert split_regime(n, G) == want, (count, split_regime(n, G))
    g = on_gpu(C, FF, n, "table")
    check_outputs(g, FORMS[SPLIT_MAIN], g.run(FORMS[SPLIT_MAIN]), _what(C, FF, count))


# ---- input classes ----------------------------------------------------------------------------------------------------------
def _class_params():
    out = []
    for C, FF in SHAPES:
        for cls, sources in (("nan_unreferenced", ("table",)), ("all_unowned", ("owner", "table")), ("all_owned", ("owner", "table"))):
            for s in sources:
                forms = ["ws-%s-norm-packed" % s, "ws-%s-nonorm-unpacked" % s, "split-%s-norm" % s]
                if s == "table":
                    forms.append("ws-table-noy")
                out += [pytest.param(C, FF, cls, f, id="%dx%d-%s-%s" % (C, FF, cls, f)) for f in forms]
    return out


@pytest.mark.parametrize("C,FF,cls,form", _class_params())
def test_input_classes_vs_float64(C, FF, cls, form):
    form = FORMS[form]
    count = "48G+5"
    g = on_gpu(C, FF, rows_of(form.kernel, C, FF, count), form.source, cls)
    c = g.case
    if cls == "nan_unreferenced":
        assert int(torch.isnan(c.attn).any(1).sum()) > c.n // 100  # there ARE poisoned rows
    if cls == "all_unowned":
        assert bool(((c.owner if c.source == "owner" else c.tab_row[:, 0]) < 0).all())
    if cls == "all_owned":
        assert bool(((c.owner if c.source == "owner" else c.tab_row[:, 0]) >= 0).all())
    check_outputs(g, form, g.run(form), _what(C, FF, count, cls))


def _guard_refs(g, W1=None):
    c = g.case
    return dict(C=c.C, FF=c.FF, W1=g.W1 if W1 is None else W1, b1=g.b1, W2=g.W2, b2=g.b2, lnw=g.ln_w, lnb=g.ln_b)


@pytest.mark.parametrize("C,FF,cls,form", [
    pytest.param(C, FF, cls, f, id="%dx%d-%s-%s" % (C, FF, cls, f)) for C, FF in SHAPES for cls in TOP_CLASSES
    for f in ("ws-plain-norm-packed", "ws-owner-nonorm-unpacked", "ws-table-norm-packed", "ws-table-nonorm-unpacked", "ws-table-noy")])
def test_split_fp16_form_near_the_top_of_the_fp16_range(C, FF, cls, form):
    from mssvt_amd import fused
    form = FORMS[form]
    g = on_gpu(C, FF, rows_of("ws", C, FF, "48G+5"), form.source, cls)
    check_top_window(g.case, g.stats)
    # the caller's guard bounds both quantities from the parameters alone: it accepts these, and declines W1 scaled so that
    # the hidden activations pass the limit
    assert fused._ffn_f16_weights(_guard_refs(g)) is not None
    beyond = g.W1 * (1.5 * F16_MAX / g.stats["hidden"])
    assert fused._ffn_f16_weights(_guard_refs(g, beyond)) is None
    check_outputs(g, form, g.run(form), _what(C, FF, "48G+5", cls))


# ---- tolerance-free properties ------------------------------------------------------------------------------------------------
CAP_PAIRS = {  # name -> (cap(G), n_dev(G))
    "16G+1,0": (lambda G: 16 * G + 1, lambda G: 0), "16G+1,1": (lambda G: 16 * G + 1, lambda G: 1),
    "16G+1,17": (lambda G: 16 * G + 1, lambda G: 17), "128G+40,48G+5": (lambda G: 128 * G + 40, lambda G: 48 * G + 5),
    "16G+1,16G+1": (lambda G: 16 * G + 1, lambda G: 16 * G + 1),
}


@pytest.mark.parametrize("C,FF,pair,form", [
    pytest.param(C, FF, pair, f, id="%dx%d-%s-%s" % (C, FF, pair, f)) for C, FF in SHAPES for pair in CAP_PAIRS
    for f in (WS_MAIN, "ws-table-noy", SPLIT_MAIN, WS_FRAME, "split-owner-nonorm")])
def test_device_row_count_leaves_the_rows_up_to_the_capacity_alone(C, FF, pair, form):
    """n_rows = capacity, num_rows_dev = n: rows [n, capacity + 32) of y, y_norm and hidden keep the sentinel bit for bit
    (the inputs there are NaN, their table / owner entries valid: a read would show), rows below n equal the launch
    with n_rows = n and no device count."""
    form = FORMS[form]
    G = grid_of(form.kernel, C, FF)
    cap, n = CAP_PAIRS[pair][0](G), CAP_PAIRS[pair][1](G)
    g = on_gpu(C, FF, n, form.source, cap=cap)
    assert g.case.cap == cap and g.case.n == n
    a = g.launch(form, n_rows=cap, n_dev=n)
    b = g.launch(form, n_rows=n)
    assert a.st == 0 and b.st == 0 and a.y.shape[0] == cap + 32
    for name, ta, tb in (("y", a.y, b.y), ("y_norm", a.yn, b.yn), ("hidden", a.hidden, b.hidden)):
        if ta is None:
            continue
        assert bool((ta[n:] == SENTINEL).all()), (name, "rows past the device count were written")
        assert torch.equal(ta[:n], tb[:n]), name
        written = (name == "y" and form.store_y) or (name == "y_norm" and form.norm) or name == "hidden"
        if written and n:
            assert bool(torch.isfinite(ta[:n]).all()) and not bool((ta[:n] == SENTINEL).all(1).any()), name
    check_outputs(g, form, b, "%dx%d cap %s" % (C, FF, pair))


@pytest.mark.parametrize("C,FF", SHAPES, ids=_ids)
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("norm", ["norm", "nonorm"])
def test_packed_fragments_equal_the_split_in_the_prologue(C, FF, source, norm):
    """k_ffn_pack and the in-kernel prologue call the same ffw_weight_frags: the same bits come out."""
    g = on_gpu(C, FF, rows_of("ws", C, FF, "48G+5"), source)
    a, b = g.run(FORMS["ws-%s-%s-packed" % (source, norm)]), g.run(FORMS["ws-%s-%s-unpacked" % (source, norm)])
    assert a.st == 0 and b.st == 0
    assert torch.equal(a.y, b.y) and torch.equal(a.yn, b.yn)


@pytest.mark.parametrize("C,FF", SHAPES, ids=_ids)
@pytest.mark.parametrize("form,count", [(WS_MAIN, "48G+5"), (WS_FRAME, "48G+5"), ("ws-table-noy", "48G+5"),
                                        (SPLIT_MAIN, "16*8G+17"), ("split-owner-nonorm", "16*8G+17")])
def test_two_launches_give_the_same_bits(C, FF, form, count):
    form = FORMS[form]
    g = on_gpu(C, FF, rows_of(form.kernel, C, FF, count), form.source)
    a, b = g.launch(form), g.launch(form)
    assert a.st == 0 and b.st == 0
    assert torch.equal(a.y, b.y) and torch.equal(a.yn, b.yn)
    assert a.hidden is None or torch.equal(a.hidden, b.hidden)


@pytest.mark.parametrize("C,FF", SHAPES, ids=_ids)
@pytest.mark.parametrize("form,count", [(WS_MAIN, "16(8G+13)+1"), (SPLIT_MAIN, "16*20G+5")])
def test_a_row_does_not_depend_on_its_neighbours_or_the_work_order(C, FF, form, count):
    """The largest launch (several tiles per workgroup / wave, pipelined, dealt XCD-contiguous) against launches over
    contiguous slices of 16 * grid rows, in which every workgroup (wave 0 of every workgroup) does exactly one tile and
    nothing is pipelined: equal bit for bit, row for row.  A row's result depends on that row alone -- MFMA columns are
    independent, LayerNorm reduces over the row's own lanes, GEMM2 sums its k-slices in a fixed order -- and slice starts
    are multiples of 16 rows, so a row keeps its lane."""
    form = FORMS[form]
    G = grid_of(form.kernel, C, FF)
    g = on_gpu(C, FF, rows_of(form.kernel, C, FF, count), "table")
    n = g.case.n
    whole = g.run(form)
    assert whole.st == 0
    out = g.buffers(form, n + 32)
    for r0 in range(0, n, 16 * G):
        rows = min(16 * G, n - r0)
        if form.kernel == "ws":
            assert ws_regime(rows, G)[1:] == (1, False)
        else:
            assert split_regime(rows, G)[1:] == (1, 1)
        assert g.launch(form, r0=r0, n_rows=rows, out=out).st == 0
    y, yn, hidden = out
    assert bool((y[n:] == SENTINEL).all()) and bool((yn[n:] == SENTINEL).all())
    for name, ta, tb in (("y", whole.y, y), ("y_norm", whole.yn, yn), ("hidden", whole.hidden, hidden)):
        if ta is None:
            continue
        diff = (ta[:n] != tb[:n]).any(1).nonzero()[:, 0]
        assert diff.numel() == 0, "%s: %d rows differ, first %s (tiles %s)" % (name, diff.numel(), diff[:8].tolist(),
                                                                             (diff[:8] // 16).tolist())


# ---- what the library declines ------------------------------------------------------------------------------------------------
def test_declined_calls_launch_nothing():
    """Shapes outside the three: MSSVT_E_TOOLARGE; phases 3 without the hidden scratch, y = NULL without y_norm or with
    phases 3: MSSVT_E_BADARG.  The outputs keep the sentinel."""
    def untouched(r):
        return all(t is None or bool((t == SENTINEL).all()) for t in (r.y, r.yn, r.hidden))

    for source in SOURCES:
        g = OnGpu(make_case(32, 64, 100, source))
        for kernel in ("ws", "split"):
            for C, FF in ((48, 96), (32, 96), (16, 32)):
                r = g.launch(FORMS["%s-%s-norm%s" % (kernel, source, "-packed" if kernel == "ws" else "")], C=C, FF=FF)
                assert r.st == E_TOOLARGE and untouched(r), (source, kernel, C, FF, r.st)
        r = g.launch(FORMS["split-%s-norm" % source], hidden_null=True)
        assert r.st == E_BADARG and untouched(r)
    g = OnGpu(make_case(32, 64, 100, "table"))
    r = g.launch(FORMS["ws-table-nonorm-packed"], y_null=True)  # y = NULL without y_norm
    assert r.st == E_BADARG and untouched(r)
    r = g.launch(FORMS["split-table-norm"], y_null=True)  # y = NULL with phases 3
    assert r.st == E_BADARG and untouched(r)
    g = OnGpu(make_case(32, 64, 100, "plain"))
    r = g.launch(FORMS["ws-plain-norm-packed"], y_null=True)  # mssvt_ffn_fused always stores y
    assert r.st == E_BADARG and untouched(r)
    from mssvt_amd import _lib
    assert int(_lib.lib().mssvt_ffn_packed_bytes(48, 96)) == 0
    junk = torch.full((64,), 7, dtype=torch.uint8, device=DEV)
    assert _lib.lib().mssvt_ffn_pack_weights(48, 96, g.W1.data_ptr(), g.W2.data_ptr(), junk.data_ptr(), _lib.stream()) == E_TOOLARGE
    torch.cuda.synchronize()
    assert bool((junk == 7).all())
