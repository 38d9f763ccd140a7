"""tests/train_matrix_ref.py held to torch on the CPU: the float64 statements equal torch (autograd where there is a
gradient) to 1e-12 relative, a plain float32 evaluation of the same statements stays inside every bound, and the
integer operands of the exact cases give integers below 2^24."""
import pytest
import torch

from tests import train_matrix_ref as ref


def _close64(a, b, what):
    scale = max(1.0, float(b.abs().max())) if b.numel() else 1.0
    assert float((a - b).abs().max() if b.numel() else 0.0) <= 1e-12 * scale, what


def _inside(got, want, lim, what):
    err = (got.double() - want).abs()
    ratio = float((err / lim.clamp(min=1e-300)).max())
    print("%s: float32 evaluation, worst |err| / bound = %.3f" % (what, ratio))
    assert bool((err <= lim).all()), (what, ratio)
    return ratio


SMALL = [(a, b) for a in (0, 1, 8, 9, 17) for b in (0, 1, 4, 5, 17)]


def _rows(M, K, g):
    return torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-8, 9, (M, 1), generator=g).float())


@pytest.mark.parametrize("K,N", [(64, 64), (64, 128), (128, 64), (128, 128), (128, 256), (256, 128)])
@pytest.mark.parametrize("transpose_w,bias,relu,scale", [(0, True, False, 1.0), (1, False, False, 0.25), (0, True, True, 0.25)])
def test_linear_statement_and_bounds(K, N, transpose_w, bias, relu, scale):
    g = torch.Generator().manual_seed(K * 7 + N)
    M = 129
    x = _rows(M, K, g)
    w = torch.randn((K, N) if transpose_w else (N, K), generator=g) / K ** 0.5
    b = torch.randn(N, generator=g) if bias else None
    y, mag = ref.linear_ref(x, w, transpose_w, b, relu, scale)
    xd = x.double().requires_grad_(True)
    t = torch.nn.functional.linear(xd, w.double().t() if transpose_w else w.double(), None if b is None else b.double())
    t = (t.relu() if relu else t) * scale
    _close64(y, t.detach(), "Y")
    if not relu:  # the input gradient IS the transposed form of the same statement
        dy = torch.randn(M, N, generator=g)
        t.backward(dy.double())
        wt = w.t().contiguous() if transpose_w else w  # (N, K)
        dx, _ = ref.linear_ref(dy, wt, 1, None, False, scale)
        _close64(dx, xd.grad, "dX")
    y32, _ = ref.linear_ref(x, w, transpose_w, b, relu, scale, dtype=torch.float32)
    lim, lim_h = ref.linear_bound(K, mag, scale), ref.linear_h_bound(x, w, transpose_w, mag, scale)
    assert _inside(y32, y, lim, "linear") < 1.0
    assert bool((lim_h >= lim).all())  # the split-fp16 bound is the fp32 bound plus the operands' terms


@pytest.mark.parametrize("M", [1, 17, 65, 577])
@pytest.mark.parametrize("cout,cin", [(64, 64), (20, 36), (256, 144)])
def test_wgrad_statement_and_bounds(M, cout, cin):
    g = torch.Generator().manual_seed(M + cout)
    x, dy = _rows(M, cin, g), _rows(M, cout, g)
    dw, db, mw, mb = ref.wgrad_ref(x, dy)
    w = torch.zeros(cout, cin, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.linear(x.double(), w, b).backward(dy.double())
    _close64(dw, w.grad, "dW")
    _close64(db, b.grad, "db")
    dw32, db32, _, _ = ref.wgrad_ref(x, dy, dtype=torch.float32)
    _inside(dw32, dw, ref.wgrad_bound(M, mw), "dW")
    _inside(db32, db, ref.wgrad_bound(M, mb), "db")


def test_exact_operands_stay_below_2_24():
    """The exact cases' operands (|x| <= 3, |w| <= 2, |b| <= 3; weight gradient: |x|, |dY| <= 3 over 2048 x 256 rows)
    give integer results below 2^24 at the largest shapes used: every partial sum in any order is an integer float32."""
    assert 3 * 2 * 256 + 3 < 2 ** 24
    assert 3 * 3 * 2048 * 256 < 2 ** 24
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-3, 4, (257, 256), generator=g).float()
    w = torch.randint(-2, 3, (128, 256), generator=g).float()
    b = torch.randint(-3, 4, (128,), generator=g).float()
    y, mag = ref.linear_ref(x, w, 0, b, False, 1.0)
    assert bool((y == y.round()).all()) and float(mag.max()) < 2 ** 24
    assert torch.equal(ref.linear_ref(x, w, 0, b, False, 1.0, dtype=torch.float32)[0].double(), y)
    dy = torch.randint(-3, 4, (257, 64), generator=g).float()
    dw, db, mw, mb = ref.wgrad_ref(x, dy)
    assert bool((dw == dw.round()).all()) and float(mw.max()) < 2 ** 24 and float(mb.max()) < 2 ** 24


@pytest.mark.parametrize("heads,hd,kind", [(2, 4, "grid"), (4, 16, "hot"), (1, 64, "hot"), (3, 8, "same"), (2, 32, "dominant"),
                                           (17, 4, "hot")])
def test_attention_statement_and_bounds(heads, hd, kind):
    wins, q, kv, dO = ref.attn_operands(heads * 100 + hd, heads, hd, kind, None if kind == "grid" else SMALL)
    cg = heads * hd
    r = ref.attn_ref(wins, q, kv, dO, heads, hd)
    # torch autograd, float64, window by window
    qd, kvd = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    O = torch.zeros(q.shape[0], cg, dtype=torch.float64)
    lse = torch.zeros(q.shape[0], heads, dtype=torch.float64)
    parts = []
    for qo, nq, ko, nk in zip(*[a.tolist() for a in wins]):
        if nq == 0 or nk == 0:
            continue
        qi = qd[qo:qo + nq].view(nq, heads, hd)
        k, v = kvd[ko:ko + nk, :cg].view(nk, heads, hd), kvd[ko:ko + nk, cg:].view(nk, heads, hd)
        s = torch.einsum("ihd,jhd->hij", qi, k)
        o = torch.einsum("hij,jhd->ihd", torch.softmax(s, -1), v).reshape(nq, cg)
        parts.append((o * dO[qo:qo + nq].double()).sum())
        O[qo:qo + nq] = o.detach()
        lse[qo:qo + nq] = torch.log(torch.exp(s.detach()).sum(-1)).t()
    torch.stack(parts).sum().backward()
    _close64(r["O"], O, "O")
    _close64(r["lse"], lse, "lse")
    _close64(r["dq"], qd.grad, "dq")
    _close64(r["dkv"], kvd.grad, "dkv")
    if kind == "hot":
        s_abs = max(float(torch.einsum("ihd,jhd->hij", q[a:a + b].view(b, heads, hd).double(),
                                       kv[c:c + d, :cg].view(d, heads, hd).double()).abs().max())
                    for a, b, c, d in zip(*[x.tolist() for x in wins]) if b and d)
        assert s_abs > 30.0
    if kind == "dominant":
        assert float(r["dkv"][:, cg:].abs()[r["dkv"][:, cg:] != 0].min()) < 1e-40  # probabilities below float32's range
    # a plain float32 evaluation of the statement (its backward fed the float32-rounded O and lse, as a kernel's is)
    O32, lse32 = r["O"].float(), r["lse"].float()
    want = ref.attn_ref(wins, q, kv, dO, heads, hd, O_in=O32, lse_in=lse32)
    got = ref.attn_ref(wins, q, kv, dO, heads, hd, O_in=O32, lse_in=lse32, dtype=torch.float32)
    for name in ("O", "lse", "dq", "dkv"):
        assert _inside(got[name], want[name], want["b" + name], "%s (%s)" % (name, kind)) < 1.0
        assert bool(torch.isfinite(want["b" + name]).all())


def test_window_grid_holds_every_pair_out_of_order():
    q_off, q_cnt, k_off, k_cnt, R, Kn = ref.window_grid(3)
    nw = q_cnt.numel()
    assert nw % 4 != 0
    assert {(a, b) for a in ref.NQS for b in ref.NKS} <= set(zip(q_cnt.tolist(), k_cnt.tolist()))
    for off, cnt, total in ((q_off, q_cnt, R), (k_off, k_cnt, Kn)):
        rows = torch.cat([torch.arange(o, o + c) for o, c in zip(off.tolist(), cnt.tolist())])
        assert torch.equal(rows.sort().values, torch.arange(total))  # a partition: every row in exactly one window
        owners = off[cnt > 0]
        assert bool((owners[1:] < owners[:-1]).any()) and bool((owners[1:] > owners[:-1]).any())
    assert not torch.equal(q_off.argsort(), k_off.argsort())
