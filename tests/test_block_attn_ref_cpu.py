"""The float64 reference of tests/test_block_attn_gpu.py, checked without a GPU before it judges a kernel:

  restatement   `reference_f64` (vectorised) equals a deliberately naive restatement of the same formulas -- Python loops,
                one window, one query, one head at a time -- to 1e-12 relative, results and range figures alike;
  sensitivity   on every class of inputs the GPU tests use, a MUTATED reference (the last live slot of each window masked;
                heads h and h + 1 swapped in the V product; bv dropped; scores scaled by ln 2; the centre part of the
                positional term dropped) leaves the tolerance the kernels are held to by a factor >= 10 in at least one
                row: 1e-5 max|ref| + 1e-4 |ref| for cases a-d, 8 x the float32 evaluation's own error for case e.  So the
                inputs can tell a subtly wrong kernel from a right one.  Where a mutation cannot apply (one head; one live
                key; no row at all) the parametrisation says so, and the test asserts that reason;
  range         the operands of case (e) sit where the case says: the scaled quantity within [0.5, 0.9] x 65504 and the
                other four below it, as the float64 reference reports them.
"""
import math

import pytest
import torch

from tests import test_block_attn_gpu as T


def naive_f64(case):
    c = case
    out = torch.full((c.cap * c.nq + 1, c.C), float("nan"), dtype=torch.float64)
    stats = dict(tokens=0.0, qp=0.0, qt=0.0, xbar=0.0, v=0.0, score=0.0)

    def bump(name, t):
        stats[name] = max(stats[name], float(torch.as_tensor(t).abs().max()))

    d = lambda t: t.double()  # noqa: E731
    for gi, (c0, cg, heads) in enumerate(c.groups):
        Wq, bq, Wo, bo = d(c.Wq[gi]), d(c.bq[gi]), d(c.Wo[gi]), d(c.bo[gi])
        Wk, bk, Wv, bv = d(c.Wkv[gi][:cg]), d(c.bkv[gi][:cg]), d(c.Wkv[gi][cg:]), d(c.bkv[gi][cg:])
        Wp, bp = d(c.Wpos[c0:c0 + cg]), d(c.bpos[c0:c0 + cg])
        for w in range(c.nw):
            centre = d(c.wcentre[w, :3])

            def token(meta):
                row = int(T.row_bits(meta))
                return d(c.xhat[row, c0:c0 + cg]) + torch.relu(Wp @ torch.cat([d(meta[:3]), centre]) + bp)

            keys = [token(c.kmeta[gi][w, k]) for k in range(c.K) if int(T.row_bits(c.kmeta[gi][w, k])) >= 0]
            for tk in keys:
                bump("tokens", tk)
                bump("v", Wv @ tk + bv)
            for s in range(c.nq):
                if int(T.row_bits(c.qmeta[w, s])) < 0:
                    continue
                tq = token(c.qmeta[w, s])
                qp = Wq @ tq + bq
                bump("tokens", tq)
                bump("qp", qp)
                o = torch.zeros(cg, dtype=torch.float64)
                for h in range(heads):
                    sl = slice(h * c.hd, (h + 1) * c.hd)
                    sc = [float(((qp[sl] * c.scale) * (Wk[sl] @ tk + bk[sl])).sum()) for tk in keys]
                    bump("score", torch.tensor(sc, dtype=torch.float64))
                    m = max(sc)
                    e = [math.exp(x - m) for x in sc]
                    z = sum(e)
                    xbar = torch.zeros(cg, dtype=torch.float64)
                    for ek, tk in zip(e, keys):
                        o[sl] += ek / z * (Wv[sl] @ tk + bv[sl])
                        xbar += ek / z * tk
                    bump("xbar", xbar)
                    bump("qt", c.scale * T.LOG2E * (Wk[sl].T @ qp[sl]))
                out[w * c.nq + s, c0:c0 + cg] = Wo @ o + bo
    return out, stats


TINY = {
    "two_groups_16x8_8x8_K17": lambda: T.make_case(28, [(0, 16, 2), (16, 8, 1)], 8, 3, 17, 5, N=40, seed=1),
    "one_group_32x16_K33_at_c0_4": lambda: T.make_case(40, [(4, 32, 2)], 16, 4, 33, 4, N=30, seed=2, keys="tile1_empty"),
}


@pytest.mark.parametrize("name", sorted(TINY))
def test_reference_equals_its_loop_restatement(name):
    case = TINY[name]()
    got, gs = T.reference_f64(case)
    want, ws = naive_f64(case)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool((~torch.isnan(want)).any())
    m = ~torch.isnan(want)
    assert float((got[m] - want[m]).abs().max()) <= 1e-12 * float(want[m].abs().max())
    for k in ws:
        assert abs(gs[k] - ws[k]) <= 1e-12 * ws[k], (k, gs[k], ws[k])


# one representative of every case class of the GPU file: name -> (builder, tolerance class)
CLASSES = {}
for _cg, _hd, _K in ((64, 16, 33), (24, 8, 8), (48, 16, 64), (32, 32, 17), (8, 8, 1)):
    CLASSES["a-%dx%d-K%d" % (_cg, _hd, _K)] = (lambda cg=_cg, hd=_hd, K=_K: T.case_a(cg, hd, K), "abcd")
for _name in T.LAYOUTS:
    CLASSES["b-" + _name] = (lambda name=_name: T.case_b(name, 32), "abcd")
for _name in T.STRUCTURES:
    CLASSES["c-" + _name] = (lambda name=_name: T.case_c(name, 64, 64), "abcd")
CLASSES["d"] = (lambda: T.case_d(32, 4), "abcd")  # the generator of (d) at the grid of a 4-CU device
for _sub in T.E_SUBCASES:
    CLASSES["e-" + _sub] = (lambda sub=_sub: T.case_e(32, 32, sub), "e")


def not_applicable(name, mutation):
    """Why `mutation` cannot show on the inputs of class `name` (None: it must show)."""
    if name == "c-no_active_window":
        return "no row is written"
    if mutation == "swap_heads_v" and name in ("a-32x32-K17", "a-8x8-K1"):
        return "one head"
    if mutation in ("mask_last_live", "scores_ln2") and name in ("a-8x8-K1", "c-one_live_key"):
        return "one live key"  # nothing to mask, and a softmax over one key is 1 at any scale
    return None


_ref_cache = {}


def _class_ref(name):
    if name not in _ref_cache:
        _ref_cache.clear()
        case = CLASSES[name][0]()
        ref, stats = T.reference_f64(case)
        bound = None
        if CLASSES[name][1] == "e":
            m = ~torch.isnan(ref)
            e32 = (T.reference(case, dtype=torch.float32)[0].double() - ref)[m].abs()
            bound = (T.MAX_RATIO * float(e32.max()), T.MAX_RATIO * float(e32.mean()))
        _ref_cache[name] = (case, ref, stats, bound)
    return _ref_cache[name]


@pytest.mark.parametrize("name,mutation", [
    pytest.param(n, m, id="%s-%s%s" % (n, m, "-cannot_apply_" + not_applicable(n, m).replace(" ", "_") if not_applicable(n, m) else ""))
    for n in CLASSES for m in T.MUTATIONS])
def test_mutated_reference_leaves_the_tolerance(name, mutation):
    case, ref, stats, bound = _class_ref(name)
    mut = T.reference_f64(case, mutate=mutation)[0]
    m = ~torch.isnan(ref)
    assert torch.equal(m, ~torch.isnan(mut))
    why = not_applicable(name, mutation)
    if why == "no row is written":
        assert not bool(m.any())
        return
    if why in ("one head", "one live key"):
        assert torch.equal(mut[m], ref[m])  # the mutation changes nothing here: these inputs cannot show it
        return
    diff = (mut - ref)[m].abs()
    if CLASSES[name][1] == "e":
        factor = max(float(diff.max()) / bound[0], float(diff.mean()) / bound[1])
    else:
        factor = float((diff / (1e-5 * ref[m].abs().max() + 1e-4 * ref[m].abs())).max())
    print("%s %s: mutated reference leaves the tolerance by a factor %.3g" % (name, mutation, factor))
    assert factor >= 10.0, (name, mutation, factor)


@pytest.mark.parametrize("cg,K", T.E_SHAPES)
@pytest.mark.parametrize("sub", T.E_SUBCASES)
def test_operands_of_the_fp16_range_cases_sit_where_the_case_says(cg, K, sub):
    case = T.case_e(cg, K, sub)
    T.check_invariants(case)
    stats = T.reference_f64(case)[1]
    print("e %dx16 K%d %s: %s" % (cg, K, sub, ", ".join("%s %.4g" % kv for kv in sorted(stats.items()))))
    T.check_e_window(case, stats, sub)
