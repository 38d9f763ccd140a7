"""The float64 reference of tests/test_ffn_forms_gpu.py, checked without a GPU before it judges a kernel:

  restatement   `reference_f64` (vectorised) equals a deliberately naive restatement of the same formulas -- Python loops,
                one row, one hidden unit, one channel at a time -- to 1e-12 relative, on small cases of every residual
                source and input class, results and range figures alike;
  sensitivity   on every class of inputs the GPU tests use, a MUTATED reference (x_in instead of 2 x_in on unowned rows; the
                third table slot dropped; b2 dropped; no ReLU on the last 16 hidden units; the two LayerNorm eps swapped;
                y_norm taken of the branch alone) leaves every tolerance the kernels are held to by a factor >= 10 in at
                least one row -- in y AND in y_norm, since there are forms that store only one of them (`norm_of_branch`
                changes y_norm alone).  For the classes `mixed`, `nan_unreferenced`, `all_*` that is the per-row bound of
                phases 4 and the 4 x float32 rule of phases 3, whichever is wider; for `near_f16_top_*` the 8 x float32
                rule.  A mutation is tried on the sources whose formula has the mutated term (`drop_w3`: table;
                `unowned_once`: owner, table); where a CLASS removes the term (no unowned row, no owned row) the
                parametrisation says so and the test asserts that reason -- at most one such triple per mutation;
  range         the `near_f16_top` cases sit where they say by the reference's own report, at all three shapes, and the
                float32 evaluation of every class stays finite.
"""
import math

import pytest
import torch

from tests import test_ffn_forms_gpu as T


def naive_f64(c, mutate=None):
    C, FF = c.C, c.FF
    lst = lambda t: None if t is None else t.double().tolist()  # noqa: E731
    x_new, x_in, attn, tab_w = lst(c.x_new), lst(c.x_in), lst(c.attn), lst(c.tab_w)
    ln_w, ln_b, W1, b1, W2, b2, ln2_w, ln2_b = [lst(t) for t in (c.ln_w, c.ln_b, c.W1, c.b1, c.W2, c.b2, c.ln2_w, c.ln2_b)]
    eps, eps2 = (c.eps2, c.eps) if mutate == "swap_eps" else (c.eps, c.eps2)
    twice = 1.0 if mutate == "unowned_once" else 2.0

    def norm(v, w, b, e):
        mean = sum(v) / C
        var = sum((a - mean) ** 2 for a in v) / C
        return [(v[j] - mean) / math.sqrt(var + e) * w[j] + b[j] for j in range(C)]

    ys, yns, stats = [], [], dict(ln=0.0, hidden=0.0)
    for r in range(c.n):
        if c.source == "plain":
            x = list(x_new[r])
        elif c.source == "owner":
            x = list(x_new[r]) if int(c.owner[r]) >= 0 else [twice * a for a in x_in[r]]
        elif int(c.tab_row[r, 0]) < 0:
            x = [twice * a for a in x_in[r]]
        else:
            x = list(x_in[r])
            for i in range(2 if mutate == "drop_w3" else 3):
                src = attn[int(c.tab_row[r, i])]
                for j in range(C):
                    x[j] += tab_w[r][i] * src[j]
        h = norm(x, ln_w, ln_b, eps)
        u = []
        for k in range(FF):
            s = b1[k]
            for j in range(C):
                s += W1[k][j] * h[j]
            if not (mutate == "relu_skip_last_tile" and k >= FF - 16):
                s = max(s, 0.0)
            u.append(s)
        y = []
        for j in range(C):
            s = 0.0 if mutate == "drop_b2" else b2[j]
            for k in range(FF):
                s += W2[j][k] * u[k]
            y.append(x[j] + s)
        ys.append(y)
        yns.append(norm([y[j] - x[j] for j in range(C)] if mutate == "norm_of_branch" else y, ln2_w, ln2_b, eps2))
        stats["ln"] = max(stats["ln"], max(abs(a) for a in h))
        stats["hidden"] = max(stats["hidden"], max(abs(a) for a in u))
    shape = (c.n, C)
    return torch.tensor(ys, dtype=torch.float64).reshape(shape), torch.tensor(yns, dtype=torch.float64).reshape(shape), stats


def _applies(cls, source):
    return source == "table" or cls != "nan_unreferenced"


TINY = [pytest.param(C, FF, n, s, cls, id="%dx%d-n%d-%s-%s" % (C, FF, n, s, cls))
        for C, FF, n, classes in ((32, 64, 19, T.CLASSES[:4]), (32, 64, 45, T.TOP_CLASSES), (64, 128, 5, ("mixed",)), (128, 256, 2, ("mixed",)))
        for cls in classes for s in T.SOURCES if _applies(cls, s)]


@pytest.mark.parametrize("C,FF,n,source,cls", TINY)
def test_reference_equals_its_loop_restatement(C, FF, n, source, cls):
    case = T.make_case(C, FF, n, source, cls, seed=3)
    for mutate in (None,) + (T.MUTATIONS if (C, n) == (32, 19) else ()):
        y, yn, st = T.reference_f64(case, mutate=mutate, chunk=7)
        wy, wyn, wst = naive_f64(case, mutate=mutate)
        assert bool(torch.isfinite(wy).all()) and bool(torch.isfinite(wyn).all())
        for got, want in ((y, wy), (yn, wyn)):
            assert float(((got - want).abs() / T.row_scale(want)).max()) <= 1e-12, mutate
        for k in wst:
            assert abs(st[k] - wst[k]) <= 1e-12 * wst[k], (k, st[k], wst[k])


def test_capacity_rows_hold_nan_and_stay_out_of_the_reference():
    for source in T.SOURCES:
        c = T.make_case(32, 64, 21, source, cap=40, seed=5)
        y, yn, _ = T.reference_f64(c)
        assert y.shape == (21, 32) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(yn).all())
        c0 = T.make_case(32, 64, 0, source, cap=17, seed=5)
        assert T.reference_f64(c0)[0].shape == (0, 32)


# (class, source) pairs of the sensitivity test; the all_* classes are the `mixed` generator with one ownership for
# every row, represented by the source that has every term
SENS = [("mixed", s) for s in T.SOURCES] + [("nan_unreferenced", "table"), ("all_unowned", "table"), ("all_owned", "table")] + \
       [(cls, s) for cls in T.TOP_CLASSES for s in T.SOURCES]
SENS_SHAPE, SENS_ROWS = (64, 128), 700


def has_term(mutation, source):
    """Whether the formula of `source` has the term `mutation` changes."""
    if mutation == "drop_w3":
        return source == "table"
    if mutation == "unowned_once":
        return source != "plain"
    return True


def not_applicable(mutation, cls, source):
    """Why `mutation` cannot show on the inputs of class `cls` although the source has the term (None: it must show)."""
    if mutation == "unowned_once" and cls == "all_owned":
        return "no unowned row"
    if mutation == "drop_w3" and cls == "all_unowned":
        return "no owned row"
    return None


SENS_PARAMS = [(m, cls, s) for cls, s in SENS for m in T.MUTATIONS if has_term(m, s)]


def test_at_most_one_inapplicable_triple_per_mutation():
    for m in T.MUTATIONS:
        assert sum(1 for mm, cls, s in SENS_PARAMS if mm == m and not_applicable(mm, cls, s)) <= 1, m
    assert set(cls for _, cls, _ in SENS_PARAMS) == set(T.CLASSES)


_ref_cache = {}


def _class_ref(cls, source):
    key = (cls, source)
    if key not in _ref_cache:
        _ref_cache.clear()
        case = T.make_case(SENS_SHAPE[0], SENS_SHAPE[1], SENS_ROWS, source, cls, seed=11)
        y, yn, stats = T.reference_f64(case)
        y32, yn32, _ = T.reference(case, dtype=torch.float32)
        assert bool(torch.isfinite(y32).all()) and bool(torch.isfinite(yn32).all())
        e32 = ((y32.double() - y).abs() / T.row_scale(y), (yn32.double() - yn).abs() / T.row_scale(yn))
        _ref_cache[key] = (case, (y, yn), e32)
    return _ref_cache[key]


def _factor(cls, source, which, diff, want, e32):
    """By how much `diff` leaves the widest tolerance any form holds output `which` (0: y, 1: y_norm) of this class to."""
    scaled = diff / T.row_scale(want)
    if cls in T.TOP_CLASSES:
        return max(float(scaled.max()) / (T.TOP_RATIO * float(e32.max())), float(scaled.mean()) / (T.TOP_RATIO * float(e32.mean())))
    ty, tn = (6e-6, 3e-5) if source == "table" else (4e-6, 2e-5)
    f_ws = float(scaled.max()) / ty if which == 0 else float(diff.max()) / tn
    f_split = max(float(scaled.max()) / (T.SPLIT_RATIO * float(e32.max()) + 1e-6),
                  float(scaled.mean()) / (T.SPLIT_RATIO * float(e32.mean())))
    return min(f_ws, f_split)


@pytest.mark.parametrize("mutation,cls,source", [
    pytest.param(m, cls, s, id="%s-%s-%s%s" % (m, cls, s, "-cannot_apply_" + not_applicable(m, cls, s).replace(" ", "_")
                                             if not_applicable(m, cls, s) else "")) for m, cls, s in SENS_PARAMS])
def test_mutated_reference_leaves_the_tolerance(mutation, cls, source):
    case, ref, e32 = _class_ref(cls, source)
    mut = T.reference_f64(case, mutate=mutation)[:2]
    why = not_applicable(mutation, cls, source)
    if why == "no unowned row":
        assert bool((case.tab_row[:case.n, 0] >= 0).all())
    if why == "no owned row":
        assert bool((case.tab_row[:case.n, 0] < 0).all())
    if why:
        assert torch.equal(mut[0], ref[0]) and torch.equal(mut[1], ref[1])  # these inputs cannot show it
        return
    outputs = (1,) if mutation == "norm_of_branch" else (0, 1)
    if mutation == "norm_of_branch":
        assert torch.equal(mut[0], ref[0])
    for which in outputs:
        f = _factor(cls, source, which, (mut[which] - ref[which]).abs(), ref[which], e32[which])
        print("%s %s %s %s: mutated reference leaves the tolerance by a factor %.3g" % (mutation, cls, source, ("y", "y_norm")[which], f))
        assert f >= 10.0, (mutation, cls, source, which, f)


@pytest.mark.parametrize("C,FF", T.SHAPES, ids=["%dx%d" % s for s in T.SHAPES])
@pytest.mark.parametrize("cls", T.TOP_CLASSES)
@pytest.mark.parametrize("source", T.SOURCES)
def test_operands_of_the_fp16_range_cases_sit_where_the_case_says(C, FF, cls, source):
    case = T.make_case(C, FF, 500, source, cls, seed=13)
    stats = T.reference_f64(case)[2]
    print("%dx%d %s %s: max|LN(x)| %.5g, max|hidden| %.5g" % (C, FF, cls, source, stats["ln"], stats["hidden"]))
    T.check_top_window(case, stats)
    top = stats["ln" if cls == "near_f16_top_ln" else "hidden"]
    assert abs(top / (T.TOP_TARGET * T.F16_MAX) - 1.0) < 0.02
    # the caller's guard (fused._ffn_f16_weights) bounds both operands from the parameters alone; its bound, restated, must
    # accept these parameters -- the GPU test asserts that on the function itself
    xmax = math.sqrt(C) * float(case.ln_w.abs().max()) + float(case.ln_b.abs().max())
    x2 = math.sqrt(C) * float(case.ln_w.abs().max()) + float(case.ln_b.norm())
    hmax = float((torch.minimum(case.W1.abs().sum(1) * xmax, case.W1.norm(dim=1) * x2) + case.b1.abs()).max())
    print("    guard bounds: LN %.5g, hidden %.5g" % (xmax, hmax))
    assert stats["ln"] <= xmax * (1 + 1e-6) and stats["hidden"] <= hmax * (1 + 1e-6)  # they ARE bounds
    assert max(xmax, hmax) < 6.0e4


@pytest.mark.parametrize("cls,source", SENS)
def test_float32_evaluation_stays_finite(cls, source):
    _class_ref(cls, source)  # asserts it
