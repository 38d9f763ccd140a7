"""The float64 reference of tests/test_compress_forms_gpu.py, checked without a GPU before it judges a kernel:

  restatement   `reference` (vectorised) equals a deliberately naive restatement of the header's formula -- Python loops, one
                window, one list slot, one channel at a time -- to 1e-12 relative, on tiny levels of every structural kind, on
                lists that are no runs (interleaved, shuffled, one empty) and under every mutation;
  sensitivity   on every class of inputs the GPU tests use, a MUTATED reference leaves every tolerance the kernels are held
                to (4 x / 8 x the float32 evaluation's error, per window row, max or mean) by a factor >= 10: the zero
                padding dropped from the max / always included; the window centre taken at the voxel's z instead of the
                slab's; the relative coordinate masked with the mask inverted (see below); the scale dropped; weights 2^s
                instead of e^s; two heads swapped in V; bv dropped; the second ReLU of pos_proj dropped; the last row of every window that crosses a 16-row
                boundary left out; every window that opens a group of 16 given its predecessor's query.  Every mutation
                shows on every class; none is set aside as inapplicable.  (There is no "bk dropped" mutation: bk adds q . bk, the same constant, to every
                score of a window and head, and the softmax cannot see it.  The relative coordinate masked the way the
                Block masks it -- times zero on the slots that are NOT listed -- is invisible for the same kind of reason:
                with the softmax over the listed slots only, no output reads a padded slot.  `mask_rel` states that
                and a test asserts the mutated reference EQUAL on every class; what is held to the factor 10 is
                `mask_rel_inverted`, the same mask with the wrong polarity, which zeroes the listed slots.)
  placement     `edge100` puts between 25 % and 75 % of the 16-row pieces over |score log2 e| = 100 with windows that go from a
                plain piece to a merge piece and back; each `top_*` operand sits at 0.6 x 65504 and the others below 0.5 x;
  arithmetic    the z_magic identity of k_cmp_ws and the LDS limit of launch_compress for every shape.
"""
import math

import numpy as np
import pytest
import torch

from tests import test_compress_forms_gpu as T


def naive_f64(c, mutate=None):
    L, C, hd, ns = c.L, c.C, c.hd, c.L.ns
    lst = lambda t: t.double().tolist()  # noqa: E731
    xhat = lst(c.xhat[:L.n])
    Wp1, bp1, Wp2, bp2, Wq, bq, Wkv, bkv, Wo, bo = [lst(getattr(c, k)) for k in T.Case.NAMES[1:]]
    f32 = np.float32

    def centre(i, cell, lo):  # fp32, ((i + 0.5) cell) + lo
        return float(f32(f32(f32(i) + f32(0.5)) * f32(cell)) + f32(lo))

    queries, slots_of = [], []
    for w in range(L.nw):
        cnt = int(L.win_cnt[w])
        slots = [int(L.win_vstart[w] + L.k_ind[w, s]) for s in range(cnt)]
        if mutate == "drop_cross16_last" and cnt and min(slots) // 16 != max(slots) // 16:
            slots.remove(max(slots))
        slots_of.append(slots)
        padded = {"pad_never": False, "pad_always": True}.get(mutate, cnt < ns)
        q_tok = []
        for ch in range(C):
            vals = [xhat[r][ch] for r in slots] + ([0.0] if padded or not slots else [])
            q_tok.append(max(vals))
        q = []
        for o in range(C):
            s = bq[o]
            for ch in range(C):
                s += Wq[o][ch] * q_tok[ch]
            q.append(s if mutate == "no_scale" else s * c.scale)
        queries.append(q)
    if mutate == "group_first_pred_query":
        queries = [queries[w - 1] if w % 16 == 0 and w > 0 else queries[w] for w in range(L.nw)]
    out = []
    for w in range(L.nw):
        b_, wz, wy, wx = [int(v) for v in L.win_ind[w]]
        wc = [centre(wx, L.win_size[0], T.MN[0]), centre(wy, L.win_size[1], T.MN[1]), centre(wz, L.win_size[2], T.MN[2])]
        scores, vals = [], []
        for r in slots_of[w]:
            _, z, y, x = [int(v) for v in L.indices[r]]
            vc = [centre(x, T.VS[0], T.MN[0]), centre(y, T.VS[1], T.MN[1]), centre(z, T.VS[2], T.MN[2])]
            wcr = [wc[0], wc[1], vc[2]] if mutate == "centre_voxel_z" else wc
            geo = [0.0 if mutate == "mask_rel_inverted" else vc[i] - wcr[i] for i in range(3)] + wcr
            h = [max(0.0, bp1[o] + sum(Wp1[o][i] * geo[i] for i in range(6))) for o in range(C)]
            k_tok = []
            for o in range(C):
                s = bp2[o]
                for ch in range(C):
                    s += Wp2[o][ch] * h[ch]
                k_tok.append(xhat[r][o] + (s if mutate == "no_relu2" else max(0.0, s)))
            kv = []
            for o in range(2 * C):
                s = 0.0 if (mutate == "no_bv" and o >= C) else bkv[o]
                for ch in range(C):
                    s += Wkv[o][ch] * k_tok[ch]
                kv.append(s)
            K, V = kv[:C], kv[C:]
            if mutate == "swap_heads":
                V = V[hd:2 * hd] + V[:hd] + V[2 * hd:]
            sc = [sum(queries[w][hh * hd + i] * K[hh * hd + i] for i in range(hd)) for hh in range(C // hd)]
            scores.append([s * math.log(2.0) for s in sc] if mutate == "pow2" else sc)
            vals.append(V)
        o_ = [0.0] * C
        for hh in range(C // hd):
            if not scores:
                break
            m = max(s[hh] for s in scores)
            e = [math.exp(s[hh] - m) for s in scores]
            tot = sum(e)
            for i in range(hd):
                o_[hh * hd + i] = sum(e[j] * vals[j][hh * hd + i] for j in range(len(e))) / tot
        out.append([bo[o] + sum(Wo[o][ch] * o_[ch] for ch in range(C)) for o in range(C)])
    return torch.tensor(out, dtype=torch.float64).reshape(L.nw, C)


TINY_KINDS = ("ones", "full32", "never_full", "mixed8", "odd5", "odd3_ns32", "unlisted", "nw1", "n1", "two_samples")


@pytest.mark.parametrize("kind", TINY_KINDS + ("lists",))
def test_reference_equals_its_loop_restatement(kind):
    L = T.fused_level(17, 12, 3) if kind == "lists" else T.structural_level(kind, small=True)
    if kind == "lists":
        assert int((L.win_cnt == 0).sum()) == 1
    case = T.make_case(L, "negative" if kind in ("never_full", "lists") else "ln", C=32, hd=8, seed=3)
    for mutate in (None,) + (T.MUTATIONS if kind in ("two_samples", "lists", "full32") else ()):
        if mutate == "mask_rel":
            continue  # (changes padded slots only, which the loop restatement never forms: module docstring)
        got, want = T.reference(case, mutate=mutate)[0], naive_f64(case, mutate)
        assert bool(torch.isfinite(want).all())
        assert float(((got - want).abs() / T.row_scale(want)).max()) <= 1e-12, (kind, mutate)
    if kind == "lists":
        w = int(np.nonzero(L.win_cnt == 0)[0][0])
        assert torch.equal(T.reference(case)[0][w], case.bo.double())  # an empty list gives bo


def test_reference_at_the_kernels_own_shape():
    L = T.structural_level("mixed8", small=True)
    case = T.make_case(L, "scaled", C=128, hd=16, seed=4)
    got, want = T.reference(case, chunk=4)[0], naive_f64(case)
    assert float(((got - want).abs() / T.row_scale(want)).max()) <= 1e-12


def test_rows_behind_the_level_hold_nan_and_stay_out_of_the_reference():
    case = T.make_case(T.structural_level("unlisted", small=True), "ln", C=32, hd=8)
    assert bool(torch.isnan(case.xhat[case.L.n:]).all()) and case.xhat.shape[0] == case.L.n + 32
    out = T.reference(case)[0]
    assert out.shape == (case.L.nw, 32) and bool(torch.isfinite(out).all())


# ---- sensitivity -----------------------------------------------------------------------------------------------------------------
# the level a mutation is tried on: mixed8, except `pad_always`, which changes only FULL lists with a channel whose maximum is
# negative -- 2^-8 per channel on mixed8 (a handful of channels of the level, lost in the one-hot softmax of `scaled`), 2^-3
# on odd3, whose full lists hold three rows
SENS_LEVEL = {"pad_always": "odd3"}


_ref_cache = {}


def _class_ref(cls, level=T.CLASS_LEVELS[0]):
    if (cls, level) not in _ref_cache:
        case = T.make_case(T.structural_level(level), cls, seed=11)
        want = T.reference(case)[0]
        o32 = T.reference(case, dtype=torch.float32)[0]
        assert bool(torch.isfinite(o32).all())
        e16 = (T.reference(case, split=True)[0] - want).abs() / T.row_scale(want)
        _ref_cache[(cls, level)] = (case, want, (o32.double() - want).abs() / T.row_scale(want), e16)
    return _ref_cache[(cls, level)]


SENS_PARAMS = [(m, cls) for m in T.MUTATIONS if m != "mask_rel" for cls in T.CLASSES]


def test_every_mutation_is_tried_on_every_class():
    """No (mutation, class) pair is set aside as inapplicable: all of them must show."""
    assert set(SENS_PARAMS) == set((m, cls) for m in T.MUTATIONS if m != "mask_rel" for cls in T.CLASSES)
    assert len(T.MUTATIONS) == 12 and len(T.CLASSES) == 9


@pytest.mark.parametrize("mutation,cls", [pytest.param(m, cls, id="%s-%s" % (m, cls)) for m, cls in SENS_PARAMS])
def test_mutated_reference_leaves_the_tolerance(mutation, cls):
    case, want, e32, e16 = _class_ref(cls, SENS_LEVEL.get(mutation, T.CLASS_LEVELS[0]))
    mut = T.reference(case, mutate=mutation)[0]
    # the widest tolerance any form is held to: the split forms' (the caps are not counted: the e32 / e16 rules alone)
    r_max, r_mean, _ = T.tolerance_ratios(cls, mut, want, e32, None if cls in T.LOOSE else e16)
    f = max(r_max, r_mean)
    print("%s %s: mutated reference leaves the tolerance by a factor %.3g" % (mutation, cls, f))
    assert f >= 10.0, (mutation, cls, f)


def test_masking_the_relative_coordinate_shows_only_where_padded_slots_are_read():
    """`mask_rel` multiplies the relative coordinate of the slots that are NOT listed by zero.  With the softmax over the
    listed slots only, no output reads those slots: the mutation is invisible to this formula on every class, which is
    why a kernel may skip them (compress_fused.hip) or never form them (compress_ws.hip)."""
    for cls in T.CLASSES:
        case, want = _class_ref(cls)[:2]
        assert torch.equal(T.reference(case, mutate="mask_rel")[0], want)


# ---- placement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in T.CLASS_LEVELS if n != "unlisted"])
def test_edge100_puts_half_of_the_pieces_over_the_limit(name):
    case = T.make_case(T.structural_level(name), "edge100")
    frac, up, down = T.check_edge100(case)
    print("%s: %.2f of the pieces over the limit, %d plain->merge windows, %d merge->plain" % (name, frac, up, down))


@pytest.mark.parametrize("name", T.CLASS_LEVELS)
@pytest.mark.parametrize("cls", T.TOP_CLASSES)
def test_operands_of_the_fp16_range_cases_sit_where_the_case_says(name, cls):
    case = T.make_case(T.structural_level(name), cls)
    st = T.reference(case)[1]
    print("%s %s: " % (name, cls) + ", ".join("%s %.5g" % (k, st[k]) for k in T.OPERANDS + ("score_max",)))
    T.check_top(case, st)


@pytest.mark.parametrize("C,hd", [(128, 16), (64, 8)])
@pytest.mark.parametrize("cls", T.TOP_CLASSES)
def test_operands_of_the_fp16_range_cases_on_hand_built_lists(C, hd, cls):
    case = T.make_case(T.fused_level(33, 12, 545), cls, C, hd)
    T.check_top(case, T.reference(case)[1])


def test_split_model_keeps_22_bits_toward_zero():
    g = torch.Generator().manual_seed(5)
    v = torch.cat([torch.randn(4000, generator=g).double() * 10.0 ** (torch.rand(4000, generator=g).double() * 12 - 8),
                   torch.tensor([0.0, 1.0, -1.0, 65504.0, 39302.4, 2.0 ** -14, 2.0 ** -24, 1e-9], dtype=torch.float64)])
    hi, lo = T.split22(v)
    assert torch.equal(hi.half().double(), hi) and torch.equal((lo * 2048.0).half().double(), lo * 2048.0)  # fp16 values
    assert bool((hi.abs() <= v.abs()).all()) and bool(((hi + lo).abs() <= v.abs()).all())               # toward zero
    big = v.abs() >= 2.0 ** -3                                                                             # both halves normal
    assert float(((v - hi - lo).abs() / v.abs().clamp(min=1e-300))[big].max()) <= 2.0 ** -21
    x, W = torch.randn(7, 32, generator=g).double(), torch.randn(5, 32, generator=g).double()
    assert float((T._product(x, W, True) - x @ W.T).abs().max()) <= 32 * 9.0 * 2.0 ** -20
    for cls in ("ln", "negative"):
        case, want, e32, e16 = _class_ref(cls)
        print("%s: e16 max %.2e mean %.2e, e32 max %.2e mean %.2e" % (cls, e16.max(), e16.mean(), e32.max(), e32.mean()))
        assert 0.0 < float(e16.mean()) < 20.0 * float(e32.mean())  # the same order as fp32's own error, not a loophole


# ---- arithmetic -----------------------------------------------------------------------------------------------------------------------
def test_z_magic_divides_every_cell_below_64():
    for z_ws in range(1, 33):
        assert T.z_magic_holds(z_ws), z_ws
        for z in range(64):
            assert (z * (65536 // z_ws + 1)) >> 16 == z // z_ws


def test_lds_limit_of_the_three_launch_form():
    want = {128: 93, 64: 142, 32: 155}
    for C in (128, 64, 32):
        ns = T.fused_ns_limit(C)
        assert ns == want[C]
        assert max(T.fused_lds(C, ns)) <= 160 * 1024 < max(T.fused_lds(C, ns + 1))
        assert T.fused_lds(C, ns)[1] >= T.fused_lds(C, ns)[0]  # the output launch (16 waves of lists) sets the limit
    assert T.fused_lds(128, 93)[1] == 68096 + 16 * 16 * 4 * 93


def test_launch_arithmetic_of_the_cases():
    assert [T.ws_groups(c, 256) for c in (0, 1, 16, 17, 48, 4096, 4097, 10 ** 6)] == [0, 1, 1, 2, 3, 256, 256, 256]
    L = T.structural_level("nw33")
    e = T.hand_made_ends(L, 8)
    assert e["all0"].tolist() == [[0, 0]] + [[L.nw, L.n]] * 8
    assert e["each"][:8, 0].tolist() == list(range(8)) and e["each"][8].tolist() == [L.nw, L.n]
    assert np.diff(e["sizes"][:, 0]).tolist()[:3] == [1, 15, 16]
    assert (np.diff(e["repeat"][:, 0]) == 0).sum() >= 3
    for v in e.values():
        assert all(int(L.win_vstart[w]) == r for w, r in v if w < L.nw)
    # the three grid regimes of k_cmp_query_keys exist on 256 compute units
    n = T.fused_level(33, 12, 545).n
    vt = (n + 15) // 16
    for C in (128, 64, 32):
        for split in (0, 1):
            assert T.fused_grids(C, 12, n, 33, split, 256)[0] < T.fused_grids(C, 12, n, 33, split, 256)[1]
            assert len(set(T.fused_grids(C, 12, n, 16 * vt, split, 256))) == 1
            g_w, g_v = T.fused_grids(C, 12, n, 16 * (vt + 9), split, 256)
            assert g_w > g_v
