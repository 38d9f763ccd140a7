"""csrc/head_conv.hip (CenterHead's shared layer, trunk and finals on split-fp16 matrix instructions, their packs and exponent
words) against the float64 statement of tests/head_conv_ref.py, under the error bound derived in tests/test_bev_conv_gpu.py:

    |got - ref| <= (3 2^-22 + S 2^-24) (|x| conv |w|) + 2^-24 max|x| sum|w|,   S = 9 Cin / 32 + 2

per output element; for the finals per branch, with max|x| over that branch's slice of the trunk tensor (the kernel normalises
every branch on its own exponent words).  With a BatchNorm fold or a bias the bound is |scale| bound + 2^-23 (|scale| A +
|shift|): scale and shift are the float64 fold rounded once to fp32."""
import numpy as np
import pytest
import torch
from torch import nn

from mssvt_amd import _lib, head_conv
from mssvt_amd._lib import MssvtHipError
from tests import head_conv_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (B, H, W): the smallest grids, odd sizes, pixel counts either side of the 32-pixel wave tile and the 256-pixel workgroup
# tile, and batches whose sample boundary falls inside a tile
GRIDS = [(1, 1, 1), (1, 2, 3), (3, 5, 7), (1, 1, 31), (1, 1, 32), (1, 1, 33), (1, 15, 17), (1, 16, 16), (1, 1, 257), (3, 9, 10)]
SHARED = [(64, 32), (512, 64)]  # golden and product channel counts
KS = {5: (3, 2, 1, 3, 2), 6: (16, 2, 1, 3, 2, 2), 11: (1, 2, 1, 3, 2, 2, 1, 1, 3, 2, 16)}  # maps per branch


def make_conv(cin, cout, seed, bias=False, wscale=1.0):
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(cin, cout, 3, stride=1, padding=1, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * wscale)
        if bias:
            conv.bias.copy_(torch.randn(cout, generator=g))
    return conv.to(DEV).eval()


def make_bn(c, seed, gain=1.0):
    g = torch.Generator().manual_seed(seed)
    bn = nn.BatchNorm2d(c, eps=1e-3)
    with torch.no_grad():
        bn.weight.copy_((torch.rand(c, generator=g) + 0.5) * gain)
        bn.bias.copy_(torch.randn(c, generator=g) * 0.3 * gain)
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.5)
        bn.running_var.copy_(torch.rand(c, generator=g) * 1.7 + 0.3)
    return bn.to(DEV).eval()


def activations(shape, seed):
    """Non-negative, half of them zero (what a ReLU leaves)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g).clamp_(min=0.0) * 3.0).contiguous()


def w_of(conv):
    return conv.weight.detach().cpu().numpy()


def b_of(conv):
    return None if conv.bias is None else conv.bias.detach().cpu().numpy()


def ratio(got, want, bound):
    return float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())


def library(x_rows, conv, bn, relu):
    with torch.no_grad():
        y = conv(x_rows.to(DEV).permute(0, 3, 1, 2))
        y = y if bn is None else bn(y)
        y = torch.relu(y) if relu else y
    return y.permute(0, 2, 3, 1).cpu().numpy()


def trunk_layers(s, nb, seed, plain=False, gains=None):
    convs = [make_conv(s, s, seed + 10 * b, bias=not plain, wscale=0.2) for b in range(nb)]
    bns = [None if plain else make_bn(s, seed + 10 * b + 1, 1.0 if gains is None else gains[b]) for b in range(nb)]
    return list(zip(convs, bns))


def final_layers(s, ks, seed, zero_bias=False):
    convs = [make_conv(s, k, seed + 7 * b, bias=True, wscale=0.3) for b, k in enumerate(ks)]
    if zero_bias:
        with torch.no_grad():
            for c in convs:
                c.bias.zero_()
    return convs


def run_finals(packed, t_rows):
    t = t_rows.to(DEV)
    return head_conv.run_finals(packed, t, head_conv.expmap(t, packed.s))


# ---- the bound, every stage, every grid -----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bn", [False, True])
@pytest.mark.parametrize("cin,s", SHARED)
def test_shared_layer_stays_inside_the_bound_on_every_grid(cin, s, with_bn):
    conv = make_conv(cin, s, seed=cin + s, bias=with_bn, wscale=0.1)
    bn = make_bn(s, seed=3) if with_bn else None
    packed = head_conv.pack_shared(conv, bn)
    worst, worst_lib = 0.0, 0.0
    for i, (B, H, W) in enumerate(GRIDS):
        x = activations((B, H, W, cin), seed=i + cin)
        y, e = head_conv.run_shared(packed, x.to(DEV))
        want, bound = ref.stage(x.numpy(), w_of(conv), b_of(conv), ref.bn_dict(bn), relu=True)
        got = y.cpu().numpy()
        assert got.shape == want.shape == (B, H, W, s)
        r = ratio(got, want, bound)
        worst = max(worst, r)
        if i == len(GRIDS) - 1:  # the library's fp32 path under the same measure, for the record (not the limit)
            worst_lib = ratio(library(x, conv, bn, True), want, bound)
        assert r <= 1.0, ((B, H, W), r)
        np.testing.assert_array_equal(e.cpu().numpy(), ref.exp_words(got, s))  # the epilogue's exponent words
    print("shared %d->%d bn=%d: worst error / bound: kernel %.3f (all grids), library fp32 %.3f (last grid)" % (cin, s, with_bn, worst, worst_lib))


@pytest.mark.parametrize("s", head_conv.S)
@pytest.mark.parametrize("cin", head_conv.CIN)
def test_every_covered_channel_pair_of_the_shared_layer(cin, s):
    """All of Cin in {64, 256, 384, 512} x S in {32, 64} (one, two, three and four 128-channel chunks) on the grid whose
    sample boundaries fall inside a tile."""
    conv, bn = make_conv(cin, s, seed=cin + s, bias=True, wscale=0.1), make_bn(s, seed=5)
    x = activations((3, 9, 10, cin), seed=cin)
    y, _ = head_conv.run_shared(head_conv.pack_shared(conv, bn), x.to(DEV))
    want, bound = ref.stage(x.numpy(), w_of(conv), b_of(conv), ref.bn_dict(bn), relu=True)
    assert ratio(y.cpu().numpy(), want, bound) <= 1.0


@pytest.mark.parametrize("nb", [5, 6, 11])
@pytest.mark.parametrize("s", [32, 64])
def test_trunk_stays_inside_the_bound_on_every_grid(s, nb):
    pairs = trunk_layers(s, nb, seed=s + nb)
    packed = head_conv.pack_trunk(pairs)
    branches = [(w_of(c), b_of(c), ref.bn_dict(bn)) for c, bn in pairs]
    worst, worst_lib = 0.0, 0.0
    for i, (B, H, W) in enumerate(GRIDS):
        x = activations((B, H, W, s), seed=i + nb)
        xd = x.to(DEV)
        t, e2 = head_conv.run_trunk(packed, xd, head_conv.expmap(xd, s))
        want, bound = ref.trunk(x.numpy(), branches)
        got = t.cpu().numpy()
        assert got.shape == want.shape == (B, H, W, nb * s)
        r = ratio(got, want, bound)
        worst = max(worst, r)
        if i == len(GRIDS) - 1:
            lib = np.concatenate([library(x, c, bn, True) for c, bn in pairs], axis=3)
            worst_lib = ratio(lib, want, bound)
        assert r <= 1.0, ((B, H, W), r)
        np.testing.assert_array_equal(e2.cpu().numpy(), ref.exp_words(got, s))  # one word per pixel AND branch
    print("trunk %d->%dx%d: worst error / bound: kernel %.3f (all grids), library fp32 %.3f (last grid)" % (s, nb, s, worst, worst_lib))


@pytest.mark.parametrize("nb", [5, 6, 11])
@pytest.mark.parametrize("s", [32, 64])
def test_finals_stay_inside_the_bound_per_branch_on_every_grid(s, nb):
    """k = 1, 2, 3 and 16 maps per branch; the output is ONE planar buffer [branch][B][k][H][W] of contiguous views."""
    ks = KS[nb]
    convs = final_layers(s, ks, seed=s + nb)
    packed = head_conv.pack_finals(convs)
    assert packed.ks == ks and packed.kbase == tuple(int(v) for v in np.cumsum((0,) + ks[:-1]))
    branches = [(w_of(c), b_of(c)) for c in convs]
    worst, worst_lib = 0.0, 0.0
    for i, (B, H, W) in enumerate(GRIDS):
        t = activations((B, H, W, nb * s), seed=i + 3 * nb)
        maps = run_finals(packed, t)
        want = ref.finals(t.numpy(), branches)
        base = maps[0].data_ptr()
        for b, (m, (w, bound)) in enumerate(zip(maps, want)):
            assert tuple(m.shape) == (B, ks[b], H, W) and m.is_contiguous()
            assert m.data_ptr() == base + 4 * B * H * W * packed.kbase[b]  # views of one buffer, in branch order
            r = ratio(m.cpu().numpy(), w, bound)
            worst = max(worst, r)
            assert r <= 1.0, ((B, H, W), b, r)
            if i == len(GRIDS) - 1:
                lib = library(t[..., b * s:(b + 1) * s].contiguous(), convs[b], None, False).transpose(0, 3, 1, 2)
                worst_lib = max(worst_lib, ratio(lib, w, bound))
    print("finals %d->%s: worst error / bound: kernel %.3f (all grids), library fp32 %.3f (last grid)" % (s, list(ks), worst, worst_lib))


def test_branches_planted_2_pow_20_apart_keep_their_own_bound():
    """The BatchNorm weight of branch 0 is 2^10 times, of branch 1 2^-10 times the others': their trunk outputs lie 2^20
    apart.  Every branch's finals stay inside THEIR OWN bound (max|x| over the branch's slice) against the statement on the
    trunk tensor the kernel produced.  One exponent word per pixel over all branches would leave branch 1's operands in
    fp16's denormal range: errors of 2^-25 of the LARGEST branch, far outside branch 1's bound."""
    s, ks = 64, (2, 3, 1, 2)
    gains = [2.0 ** 10, 2.0 ** -10, 1.0, 1.0]
    pairs = trunk_layers(s, len(ks), seed=40, gains=gains)
    convs = final_layers(s, ks, seed=41)
    x = activations((2, 9, 11, s), seed=42).to(DEV)
    t, e2 = head_conv.run_trunk(head_conv.pack_trunk(pairs), x, head_conv.expmap(x, s))
    maps = head_conv.run_finals(head_conv.pack_finals(convs), t, e2)
    tn = t.cpu().numpy()
    top = [float(np.abs(tn[..., b * s:(b + 1) * s]).max()) for b in range(len(ks))]
    assert top[0] / top[1] > 2.0 ** 18 and top[1] > 0.0
    for b, (m, (want, bound)) in enumerate(zip(maps, ref.finals(tn, [(w_of(c), b_of(c)) for c in convs]))):
        r = ratio(m.cpu().numpy(), want, bound)
        print("planted ranges: branch %d max|x| %.3g, worst error / bound %.3f" % (b, top[b], r))
        assert r <= 1.0, (b, r)


# ---- one kernel for two families -------------------------------------------------------------------------------------------
# 70 pixels: a wave's tile straddles two samples and the last tile is partial; 969: four workgroups, the last one partial
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (3, 17, 19)])
@pytest.mark.parametrize("stage,c", [("shared", 64), ("trunk", 32), ("trunk", 64)])
def test_the_heads_stages_are_the_bev_layer_bit_for_bit(stage, c, B, H, W):
    """A Conv 3x3 (stride 1, padding 1) c -> c + BatchNorm + ReLU through ``mssvt_bev_conv`` (run-time taps, one header
    record) and through the head's shared layer / its one-branch trunk (folded taps, sliced input, a record per slice): the
    same outputs, the same blob past the first record (which differs in k alone), and the head's epilogue words are the
    stand-alone exponent pass over the output."""
    from mssvt_amd import bev_conv
    conv, bn = make_conv(c, c, seed=c + B, bias=True, wscale=0.1), make_bn(c, seed=c + H)
    x = torch.randn((B, H, W, c), generator=torch.Generator().manual_seed(W + c)).mul_(3.0).to(DEV)
    layer = bev_conv.pack(conv, bn)
    want = bev_conv.conv_bn_act(x.permute(0, 3, 1, 2), layer, relu=True).permute(0, 2, 3, 1)
    if stage == "shared":
        packed = head_conv.pack_shared(conv, bn)
        y, e = head_conv.run_shared(packed, x)
    else:
        packed = head_conv.pack_trunk([(conv, bn)])
        y, e = head_conv.run_trunk(packed, x, head_conv.expmap(x, c))
    assert y.shape == want.shape and torch.equal(y, want)
    assert packed.blob.numel() == layer.blob.numel() and torch.equal(packed.blob[16:], layer.blob[16:])
    assert torch.equal(packed.blob[:8], layer.blob[:8])  # (and of the first record, the two powers of two)
    assert torch.equal(e, head_conv.expmap(y, c))


# ---- geometry ----------------------------------------------------------------------------------------------------------
def impulses(cin, H=5, W=7):
    """Sample b holds one element 1 + 2^-12 (hi = 1, lo = 2^-12) at position b of the grid: every border and corner."""
    x = torch.zeros(H * W, H, W, cin)
    for b in range(H * W):
        x[b, b // W, b % W, (7 * b) % cin] = 1.0 + 2.0 ** -12
    return x


def check_impulse(got, want):
    assert set(np.unique(want)) <= {0.0, (1.0 + 2.0 ** -12) * (1.0 + 2.0 ** -13)}
    assert (want != 0.0).sum() > 0
    assert (got[want == 0.0] == 0.0).all()  # non-zero only where the statement is
    assert (np.abs(got - want)[want != 0.0] <= 2.0 ** -23).all()  # 1 ulp of a float32 in [1, 2)


@pytest.mark.parametrize("cin,s", SHARED)
def test_impulse_pins_the_shared_layers_taps_and_both_cross_terms(cin, s):
    """Every weight 1 + 2^-13: each output the impulse reaches is the float32 product within 1 ulp, every other one exactly
    0.  A dropped hi lo or lo hi term is 2^-12 or 2^-13 off: 2048 / 1024 ulp."""
    conv = make_conv(cin, s, seed=1)
    with torch.no_grad():
        conv.weight.fill_(1.0 + 2.0 ** -13)
    x = impulses(cin)
    y, _ = head_conv.run_shared(head_conv.pack_shared(conv, None), x.to(DEV))
    check_impulse(y.cpu().numpy(), ref.stage(x.numpy(), w_of(conv))[0])


@pytest.mark.parametrize("s,nb", [(32, 5), (64, 6)])
def test_impulse_pins_the_trunks_and_the_finals_taps_slices_and_planar_layout(s, nb):
    pairs = trunk_layers(s, nb, seed=2, plain=True)
    convs = final_layers(s, KS[nb], seed=3, zero_bias=True)
    with torch.no_grad():
        for c in [p[0] for p in pairs] + convs:
            c.weight.fill_(1.0 + 2.0 ** -13)
    x = impulses(s)
    xd = x.to(DEV)
    t, _ = head_conv.run_trunk(head_conv.pack_trunk(pairs), xd, head_conv.expmap(xd, s))
    check_impulse(t.cpu().numpy(), ref.trunk(x.numpy(), [(w_of(c), None, None) for c, _ in pairs])[0])
    # the finals: the impulse in ONE branch's slice (branch = position mod nb) must reach that branch's maps only
    tx = impulses(nb * s)
    maps = run_finals(head_conv.pack_finals(convs), tx)
    want = ref.finals(tx.numpy(), [(w_of(c), None) for c in convs])
    hit = 0
    for m, (w, _) in zip(maps, want):
        got = m.cpu().numpy()
        assert (got[w == 0.0] == 0.0).all() and (np.abs(got - w)[w != 0.0] <= 2.0 ** -23).all()
        hit += int((w != 0.0).sum())
    assert hit > 0


@pytest.mark.parametrize("stage", head_conv.STAGES)
def test_power_of_two_scaling_is_exact(stage):
    """Input x 2^k -> output x 2^k, bit for bit (no shift: no BatchNorm, zero bias)."""
    s, nb = 64, 5
    if stage == "shared":
        packed = head_conv.pack_shared(make_conv(256, s, seed=9), None)
        x = (activations((2, 11, 13, 256), seed=4) + 2.0 ** -6).to(DEV)  # (no zeros: every element really scales)
        run = lambda v: head_conv.run_shared(packed, v)[0]  # noqa: E731
    elif stage == "trunk":
        packed = head_conv.pack_trunk(trunk_layers(s, nb, seed=9, plain=True))
        x = (activations((2, 11, 13, s), seed=4) + 2.0 ** -6).to(DEV)
        run = lambda v: head_conv.run_trunk(packed, v, head_conv.expmap(v, s))[0]  # noqa: E731
    else:
        packed = head_conv.pack_finals(final_layers(s, KS[nb], seed=9, zero_bias=True))
        x = (activations((2, 11, 13, nb * s), seed=4) + 2.0 ** -6).to(DEV)
        run = lambda v: torch.cat([m.reshape(-1) for m in head_conv.run_finals(packed, v, head_conv.expmap(v, s))])  # noqa: E731
    base = run(x)
    assert float(base.abs().max()) > 0
    for p in (18, -20):
        assert torch.equal(run(x * 2.0 ** p), base * 2.0 ** p), p


def test_non_finite_inputs_never_come_out_finite():
    s, ks = 32, (3, 2, 1)
    conv, bn = make_conv(64, s, seed=2, bias=True, wscale=0.1), make_bn(s, seed=3)
    x = activations((2, 6, 9, 64), seed=8)
    x[0, 2, 3, 5] = float("nan")
    x[1, 4, 8, 63] = float("inf")
    x[1, 0, 0, 0] = float("-inf")
    y, _ = head_conv.run_shared(head_conv.pack_shared(conv, bn), x.to(DEV))
    want, _ = ref.stage(x.numpy(), w_of(conv), b_of(conv), ref.bn_dict(bn), relu=True)
    got = y.cpu().numpy()
    bad = ~np.isfinite(want)
    assert bad.sum() > 0 and not np.isfinite(got[bad]).any()
    clean = np.isfinite(want).all(axis=3)
    assert np.isfinite(got[clean]).all()  # pixels out of their reach are untouched
    # trunk and finals on a tensor with the same three elements planted
    pairs, convs = trunk_layers(s, len(ks), seed=5), final_layers(s, ks, seed=6)
    xs = activations((2, 6, 9, s), seed=9)
    xs[0, 2, 3, 5], xs[1, 4, 8, 31], xs[1, 0, 0, 0] = float("nan"), float("inf"), float("-inf")
    xd = xs.to(DEV)
    t, e2 = head_conv.run_trunk(head_conv.pack_trunk(pairs), xd, head_conv.expmap(xd, s))
    want_t, _ = ref.trunk(xs.numpy(), [(w_of(c), b_of(c), ref.bn_dict(b)) for c, b in pairs])
    got_t = t.cpu().numpy()
    bad = ~np.isfinite(want_t)
    assert bad.sum() > 0 and not np.isfinite(got_t[bad]).any()
    maps = head_conv.run_finals(head_conv.pack_finals(convs), t, e2)
    for m, (w, _) in zip(maps, ref.finals(got_t, [(w_of(c), b_of(c)) for c in convs])):
        bad = ~np.isfinite(w)
        assert bad.sum() > 0 and not np.isfinite(m.cpu().numpy()[bad]).any()
        clean = np.broadcast_to(np.isfinite(w).all(axis=1, keepdims=True), w.shape)
        assert np.isfinite(m.cpu().numpy()[clean]).all()


# ---- memory --------------------------------------------------------------------------------------------------------------
GUARD = 4096


def guarded(n, dtype=torch.float32, fill=float("nan"), data=None):
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    if data is not None:
        big[GUARD:GUARD + n] = data.to(DEV).reshape(-1)
    return big, big[GUARD:GUARD + n]


def untouched(big, n):
    lo, hi = big[:GUARD], big[GUARD + n:]
    if big.dtype == torch.float32:
        return bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all())
    return bool((lo == -1).all()) and bool((hi == -1).all())


@pytest.mark.parametrize("cin,s,nb,B,H,W", [(64, 32, 5, 2, 17, 19), (384, 64, 6, 3, 3, 5)])
def test_reads_stay_inside_the_inputs_and_every_output_element_is_written(cin, s, nb, B, H, W):
    """Input, both exponent workspaces, the shared tensor, the trunk tensor, its words and the planar output all sit inside
    NaN / -1 filled allocations: a read outside poisons the result, a write outside changes a guard word, an element left
    unwritten stays NaN / -1.  The results are the bits of the tight allocations."""
    ks = KS[nb]
    conv, bn = make_conv(cin, s, seed=3, bias=True, wscale=0.1), make_bn(s, seed=4)
    pairs, convs = trunk_layers(s, nb, seed=5), final_layers(s, ks, seed=6)
    ps, pt, pf = head_conv.pack_shared(conv, bn), head_conv.pack_trunk(pairs), head_conv.pack_finals(convs)
    xs = activations((B, H, W, cin), seed=6)
    n = B * H * W
    xbig, x = guarded(n * cin, data=xs)
    wbig, ws = guarded(n, torch.int32, -1)
    ybig, y = guarded(n * s)
    e1big, e1 = guarded(n, torch.int32, -1)
    tbig, t = guarded(n * nb * s)
    e2big, e2 = guarded(n * nb, torch.int32, -1)
    obig, o = guarded(n * sum(ks))
    st = _lib.stream()
    _lib.call("mssvt_head_conv_shared", x.data_ptr(), B, H, W, cin, s, ps.blob.data_ptr(), ws.data_ptr(), y.data_ptr(),
              e1.data_ptr(), st)
    _lib.call("mssvt_head_conv_trunk", y.data_ptr(), B, H, W, s, nb, pt.blob.data_ptr(), e1.data_ptr(), t.data_ptr(),
              e2.data_ptr(), st)
    _lib.call("mssvt_head_conv_finals", t.data_ptr(), B, H, W, s, nb, pf.blob.data_ptr(), e2.data_ptr(), o.data_ptr(), st)
    for big, inner in ((xbig, x), (wbig, ws), (ybig, y), (e1big, e1), (tbig, t), (e2big, e2), (obig, o)):
        assert untouched(big, inner.numel())
    for inner in (y, t, o):
        assert bool(torch.isfinite(inner).all())
    for inner in (ws, e1, e2):
        assert bool((inner >= 0).all())
    yy, ee = head_conv.run_shared(ps, xs.to(DEV))
    tt, ee2 = head_conv.run_trunk(pt, yy, ee)
    maps = head_conv.run_finals(pf, tt, ee2)
    assert torch.equal(yy.reshape(-1), y) and torch.equal(ee, e1) and torch.equal(tt.reshape(-1), t) and torch.equal(ee2, e2)
    assert torch.equal(torch.cat([m.reshape(-1) for m in maps]), o)
    # the stand-alone exponent pass writes every word, nothing else, and the words of the producing stage's epilogue
    ebig, e = guarded(n * nb, torch.int32, -1)
    _lib.call("mssvt_head_conv_expmap", t.data_ptr(), n * nb, s, e.data_ptr(), st)
    assert untouched(ebig, n * nb) and torch.equal(e, e2)


def small_head(cin=64, shared=32, seed=0, **kw):
    return ref.build_head(cin, seed=seed, shared=shared, **kw).to(DEV)


def flat(pred_dicts):
    return torch.cat([v.reshape(-1) for pd in pred_dicts for v in pd.values()])


def test_bit_identical_across_calls_and_streams():
    head = small_head(seed=12)
    x = activations((3, 64, 21, 23), seed=13).to(DEV).contiguous(memory_format=torch.channels_last)
    first = flat(head_conv.forward(head, x))
    again = flat(head_conv.forward(head, x))
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(flat(head_conv.forward(head, x)))
        s.synchronize()
    for o in [again] + outs:
        assert torch.equal(first, o)


def test_pack_and_forward_never_synchronise_the_host():
    head = small_head(seed=14)
    x = activations((2, 64, 9, 9), seed=15).to(DEV).contiguous(memory_format=torch.channels_last)
    warm = flat(head_conv.forward(head, x))
    torch.cuda.synchronize()
    with torch.no_grad():
        head.shared_conv[0].weight.mul_(1.0)  # a new version: the pack below really runs
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        probe = torch.ones(1, device=DEV)
        try:
            probe.item()
            live = False
        except RuntimeError:
            live = True
        if live:
            before = head_conv._cache[head][1]
            packs = head_conv.pack(head)
            out = flat(head_conv.forward(head, x))
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    assert packs is not before and torch.equal(warm, out)


def test_every_status_code_is_reached_and_nothing_is_launched():
    lib = _lib.lib()
    assert lib.mssvt_head_conv_supported(512, 64, 5, 3) == 1 and lib.mssvt_head_conv_supported(64, 32, 11, 16) == 1
    for bad in [(128, 64, 5, 3), (512, 48, 5, 3), (512, 64, 0, 3), (512, 64, 65, 3), (512, 64, 5, 17), (512, 64, 5, 0)]:
        assert lib.mssvt_head_conv_supported(*bad) == 0, bad
    assert lib.mssvt_head_conv_shared_pack_bytes(512, 64) == 64 + 8 * 64 + 36 * 512 * 64
    assert lib.mssvt_head_conv_trunk_pack_bytes(64, 5) == 128 + 8 * 320 + 36 * 64 * 320
    assert lib.mssvt_head_conv_finals_pack_bytes(32, 11) == 192 + 8 * 176 + 36 * 32 * 176
    assert lib.mssvt_head_conv_shared_pack_bytes(128, 64) == 0 and lib.mssvt_head_conv_trunk_pack_bytes(48, 5) == 0
    assert lib.mssvt_head_conv_finals_pack_bytes(64, 0) == 0
    s, nb, ks = 32, 3, (3, 2, 1)
    conv = make_conv(64, s, seed=1)
    pairs, convs = trunk_layers(s, nb, seed=2), final_layers(s, ks, seed=3)
    ps, pt, pf = head_conv.pack_shared(conv, None), head_conv.pack_trunk(pairs), head_conv.pack_finals(convs)
    before = [p.blob.clone() for p in (ps, pt, pf)]
    n = 16
    x = torch.zeros(1, 4, 4, 64, device=DEV)
    y = torch.full((n * s,), 7.0, device=DEV)
    t = torch.full((n * nb * s,), 7.0, device=DEV)
    o = torch.full((n * sum(ks),), 7.0, device=DEV)
    e = torch.full((n * nb,), 7, dtype=torch.int32, device=DEV)
    st = _lib.stream()
    xp, yp, tp, op, ep = x.data_ptr(), y.data_ptr(), t.data_ptr(), o.data_ptr(), e.data_ptr()
    sp, tpk, fp, wp = ps.blob.data_ptr(), pt.blob.data_ptr(), pf.blob.data_ptr(), conv.weight.data_ptr()
    BAD, BIG = -1, -2
    assert lib.mssvt_head_conv_shared(None, 1, 4, 4, 64, s, sp, ep, yp, ep, st) == BAD
    assert lib.mssvt_head_conv_shared(xp, 0, 4, 4, 64, s, sp, ep, yp, ep, st) == BAD
    assert lib.mssvt_head_conv_shared(xp, 1, 4, 4, 64, s, sp, None, yp, ep, st) == BAD
    assert lib.mssvt_head_conv_shared(xp + 4, 1, 4, 4, 64, s, sp, ep, yp, ep, st) == BAD  # unaligned
    assert lib.mssvt_head_conv_shared(xp, 1, 4, 4, 128, s, sp, ep, yp, ep, st) == BIG
    assert lib.mssvt_head_conv_shared(xp, 1, 4, 4, 64, 48, sp, ep, yp, ep, st) == BIG
    assert lib.mssvt_head_conv_shared(xp, 1 << 15, 1 << 8, 1 << 8, 64, s, sp, ep, yp, ep, st) == BIG  # 2^31 pixels
    assert lib.mssvt_head_conv_trunk(yp, 1, 4, 4, s, nb, tpk, None, tp, ep, st) == BAD
    assert lib.mssvt_head_conv_trunk(yp, 1, 4, 0, s, nb, tpk, ep, tp, ep, st) == BAD
    assert lib.mssvt_head_conv_trunk(yp, 1, 4, 4, s, nb, tpk, ep, tp + 8, ep, st) == BAD
    assert lib.mssvt_head_conv_trunk(yp, 1, 4, 4, 16, nb, tpk, ep, tp, ep, st) == BIG
    assert lib.mssvt_head_conv_trunk(yp, 1, 4, 4, s, 65, tpk, ep, tp, ep, st) == BIG
    assert lib.mssvt_head_conv_finals(tp, 1, 4, 4, s, nb, fp, ep, None, st) == BAD
    assert lib.mssvt_head_conv_finals(tp, 1, 4, 4, s, 0, fp, ep, op, st) == BAD
    assert lib.mssvt_head_conv_finals(tp, 1, 4, 4, s, nb, fp + 4, ep, op, st) == BAD
    assert lib.mssvt_head_conv_finals(tp, 1, 4, 4, 128, nb, fp, ep, op, st) == BIG
    assert lib.mssvt_head_conv_finals(tp, 1 << 15, 1 << 8, 1 << 8, s, nb, fp, ep, op, st) == BIG
    assert lib.mssvt_head_conv_expmap(None, 16, s, ep, st) == BAD and lib.mssvt_head_conv_expmap(tp, 0, s, ep, st) == BAD
    assert lib.mssvt_head_conv_expmap(tp, 16, 48, ep, st) == BIG
    assert lib.mssvt_head_conv_shared_pack(None, None, None, None, None, None, 0.0, 64, s, sp, st) == BAD
    assert lib.mssvt_head_conv_shared_pack(wp, None, wp, None, None, None, 0.0, 64, s, sp, st) == BAD  # affine without statistics
    assert lib.mssvt_head_conv_shared_pack(wp, None, None, None, wp, None, 0.0, 64, s, sp, st) == BAD  # mean without variance
    assert lib.mssvt_head_conv_shared_pack(wp, None, None, None, None, None, 0.0, 128, s, sp, st) == BIG
    assert lib.mssvt_head_conv_trunk_pack(wp, None, None, None, None, None, 0.0, s, nb, nb, tpk, st) == BAD  # branch outside
    assert lib.mssvt_head_conv_trunk_pack(wp, None, None, None, None, None, 0.0, s, nb, 0, tpk + 4, st) == BAD
    assert lib.mssvt_head_conv_trunk_pack(wp, None, None, None, None, None, 0.0, 48, nb, 0, tpk, st) == BIG
    assert lib.mssvt_head_conv_finals_pack(wp, None, s, nb, -1, 3, 0, fp, st) == BAD
    assert lib.mssvt_head_conv_finals_pack(wp, None, s, nb, 0, 0, 0, fp, st) == BAD
    assert lib.mssvt_head_conv_finals_pack(wp, None, s, nb, 0, 17, 0, fp, st) == BIG
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((t == 7.0).all()) and bool((o == 7.0).all()) and bool((e == 7).all())
    for p, b in zip((ps, pt, pf), before):
        assert torch.equal(p.blob, b)
    # the Python layer: no CPU path, contiguous channels-last rows of the right width only
    for wrong in (x.cpu(), x.double(), x[:, :, :, :32], x[0], x.permute(0, 3, 1, 2)):
        with pytest.raises(MssvtHipError):
            head_conv.run_shared(ps, wrong)
    with pytest.raises(MssvtHipError):
        head_conv.pack_shared(make_conv(64, s, seed=1).cpu(), None)
    with pytest.raises(MssvtHipError):
        head_conv.pack(small_head(num_conv={"dim": 1}))


def test_cache_is_rebuilt_after_load_state_dict_and_in_place_changes():
    head = small_head(seed=21)
    x = activations((1, 64, 8, 8), seed=22).to(DEV).contiguous(memory_format=torch.channels_last)
    p0 = head_conv.pack(head)
    assert head_conv.pack(head) is p0
    out0 = flat(head_conv.forward(head, x))
    with torch.no_grad():
        head.heads_list[0].dim[0][1].running_var.add_(0.25)  # a running statistic of one branch's trunk layer
    p1 = head_conv.pack(head)
    assert p1 is not p0 and not torch.equal(p1["trunk"].blob, p0["trunk"].blob) and torch.equal(p1["shared"].blob, p0["shared"].blob)
    with torch.no_grad():
        head.heads_list[0].hm[1].weight.mul_(2.0)  # what an optimizer step does
    p2 = head_conv.pack(head)
    assert p2 is not p1 and head_conv.pack(head) is p2 and not torch.equal(p2["finals"].blob, p1["finals"].blob)
    sd = {k: v.clone() for k, v in head.state_dict().items()}
    sd["shared_conv.0.weight"] *= -0.5
    head.load_state_dict(sd)
    p3 = head_conv.pack(head)
    assert p3 is not p2 and not torch.equal(p3["shared"].blob, p2["shared"].blob)
    out3 = flat(head_conv.forward(head, x))
    assert not torch.equal(out3, out0)
    with torch.no_grad():  # and the new blobs are the new layers: against the library
        want = [hd(head.shared_conv(x)) for hd in head.heads_list]
    got = head_conv.forward(head, x)
    for g, w in zip(got, want):
        for k in w:
            np.testing.assert_allclose(g[k].cpu().numpy(), w[k].cpu().numpy(), rtol=1e-4, atol=1e-4 * max(1.0, float(w[k].abs().max())))
