"""tests/head_conv_ref.py (the float64 statement the GPU tests hold csrc/head_conv.hip to) against torch's float64 conv2d /
batch_norm on the CPU for a whole small head, its error bound against the formula written out, and the configuration side
of the switch: the yaml key sets the attribute, ``head_conv.supported`` is the coverage rule."""
import numpy as np
import torch
import torch.nn.functional as F

from mssvt_amd import head_conv
from tests import bev_conv_ref, head_conv_ref as ref


def test_statement_is_torch_in_float64_for_a_whole_small_head():
    """Two heads, one with three classes' worth of branches, `vel` included: 12 branches on a 9 x 11 map."""
    head = ref.build_head(64, seed=3, shared=32, heads=[["Vehicle"], ["Pedestrian", "Cyclist"]], vel=True).double()
    x = torch.randn(2, 64, 9, 11, generator=torch.Generator().manual_seed(1)).clamp_(min=0).double()
    with torch.no_grad():
        y = head.shared_conv(x)
        want = [sep(y) for sep in head.heads_list]
    sd = {k: v.numpy() for k, v in head.state_dict().items()}
    sd["eps"] = head.shared_conv[1].eps
    names = [list(sep.sep_head_dict) for sep in head.heads_list]
    assert names[0] == ["center", "center_z", "dim", "rot", "vel", "hm"] and sum(len(n) for n in names) == 12
    got = ref.head_forward(sd, x.permute(0, 2, 3, 1).numpy(), names)
    assert len(got) == 12
    for i, w in enumerate(want):
        for k, v in w.items():
            assert got[(i, k)].shape == tuple(v.shape)
            np.testing.assert_allclose(got[(i, k)], v.numpy(), rtol=1e-12, atol=1e-12)


def test_stages_against_conv2d_and_batch_norm_one_by_one():
    g = torch.Generator().manual_seed(2)
    s, ks = 32, (3, 1, 16)
    x = torch.randn(2, 5, 7, s, generator=g).double()
    ws = [torch.randn(s, s, 3, 3, generator=g).double() for _ in ks]
    bns = [dict(mean=torch.randn(s, generator=g).double().numpy(), var=(torch.rand(s, generator=g) + 0.5).double().numpy(),
                eps=1e-3, weight=torch.randn(s, generator=g).double().numpy(), bias=torch.randn(s, generator=g).double().numpy())
           for _ in ks]
    t, bound = ref.trunk(x.numpy(), [(w.numpy(), None, bn) for w, bn in zip(ws, bns)])
    assert t.shape == bound.shape == (2, 5, 7, len(ks) * s) and (bound > 0).all()
    for b, (w, bn) in enumerate(zip(ws, bns)):
        y = F.conv2d(x.permute(0, 3, 1, 2), w, padding=1)
        y = F.batch_norm(y, torch.from_numpy(bn["mean"]), torch.from_numpy(bn["var"]), torch.from_numpy(bn["weight"]),
                         torch.from_numpy(bn["bias"]), False, 0.0, 1e-3).relu()
        np.testing.assert_allclose(t[..., b * s:(b + 1) * s], y.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=1e-12)
    fw = [(torch.randn(k, s, 3, 3, generator=g).double(), torch.randn(k, generator=g).double()) for k in ks]
    maps = ref.finals(t, [(w.numpy(), b.numpy()) for w, b in fw])
    tt = torch.from_numpy(t).permute(0, 3, 1, 2)
    for b, ((m, bd), (w, bias)) in enumerate(zip(maps, fw)):
        want = F.conv2d(tt[:, b * s:(b + 1) * s], w, bias, padding=1)
        assert m.shape == bd.shape == tuple(want.shape) == (2, ks[b], 5, 7)
        np.testing.assert_allclose(m, want.numpy(), rtol=1e-12, atol=1e-12)
    buf = ref.planar([m for m, _ in maps])
    assert buf.shape == (2 * 5 * 7 * sum(ks),)
    np.testing.assert_array_equal(buf[2 * 35 * 3:2 * 35 * 4].reshape(2, 1, 5, 7), maps[1][0])  # [branch][B][k][H][W]


def test_error_bound_is_the_formula_and_the_finals_bound_is_per_branch_slice():
    g = np.random.default_rng(3)
    s = 64
    x = np.abs(g.standard_normal((1, 4, 5, s)))
    w = g.standard_normal((3, s, 3, 3))
    y, a, scale, shift = ref.conv(x, w)
    steps = 9 * s // 32 + 2
    assert bev_conv_ref.steps(3, s) == steps
    want = (3 * 2.0 ** -22 + steps * 2.0 ** -24) * a + 2.0 ** -24 * x.max() * np.abs(w).sum(axis=(1, 2, 3))
    np.testing.assert_allclose(ref.error_bound(a, x, w), want, rtol=1e-15)
    _, plain = ref.stage(x, w)
    np.testing.assert_allclose(plain, want, rtol=1e-15)
    bias = g.standard_normal(3)
    _, folded = ref.stage(x, w, bias)
    np.testing.assert_allclose(folded, want + 2.0 ** -23 * (a + np.abs(bias)), rtol=1e-15)
    # two branches: raising the OTHER branch's slice by 2^20 leaves this branch's value and bound untouched
    t = np.abs(g.standard_normal((1, 4, 5, 2 * s)))
    branches = [(g.standard_normal((2, s, 3, 3)), None), (g.standard_normal((3, s, 3, 3)), None)]
    base = ref.finals(t, branches)
    t2 = t.copy()
    t2[..., :s] *= 2.0 ** 20
    moved = ref.finals(t2, branches)
    np.testing.assert_array_equal(moved[1][0], base[1][0])
    np.testing.assert_array_equal(moved[1][1], base[1][1])
    np.testing.assert_allclose(moved[0][1], base[0][1] * 2.0 ** 20, rtol=1e-15)
    words = ref.exp_words(np.array([[0.0, -3.0, 2.0, 1.0], [0.5, 0.25, -0.125, 0.0]], np.float32), 4)
    np.testing.assert_array_equal(words, np.array([3.0, 0.5], np.float32).view(np.int32))


def test_yaml_key_sets_the_attribute_and_supported_is_the_coverage_rule():
    from mssvt_amd import centerpoint, config
    cfg = config.load_yaml(config.DEFAULT_CFG)
    torch.manual_seed(0)
    assert centerpoint.build_detector(cfg).dense_head.fused_convs is False  # off by default
    cfg.MODEL.DENSE_HEAD["FUSED_CONVS"] = True
    head = centerpoint.build_detector(cfg).dense_head
    assert head.fused_convs is True
    assert head_conv.supported(head)  # 512 -> 64, five branches with num_conv 2
    found = head_conv.layers(head)
    assert (found[0][0].in_channels, found[0][0].out_channels, len(found[1]), [c.out_channels for c in found[2]]) == \
        (512, 64, 5, [2, 1, 3, 2, 3])
    assert head_conv.supported(ref.build_head(64, shared=32, heads=[["Vehicle"], ["Pedestrian", "Cyclist"]], vel=True))
    assert ref.build_head(64, shared=32, fused=True).fused_convs is True and ref.build_head(64, shared=32).fused_convs is False
    for kw in (dict(num_conv={"dim": 1}), dict(num_conv={"hm": 3}), dict(num_conv={k: 1 for k in ("hm", "center", "center_z", "dim", "rot")}),
               dict(shared=48), dict(shared=128)):
        assert not head_conv.supported(ref.build_head(64, **dict(dict(shared=32), **kw))), kw
    assert not head_conv.supported(ref.build_head(128, shared=32))  # Cin outside the set
    odd = ref.build_head(64, shared=32)
    odd.shared_conv[1] = torch.nn.BatchNorm2d(32, track_running_stats=False)  # no running statistics
    assert not head_conv.supported(odd)
    odd = ref.build_head(64, shared=32)
    odd.heads_list[0].rot[0][1] = torch.nn.GroupNorm(4, 32)
    assert not head_conv.supported(odd)
