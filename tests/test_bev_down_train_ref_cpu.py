"""tests/bev_down_train_ref.py against torch's autograd in float64 (both spellings of the layer), its four-phase form of the
input gradient against the direct sum, its emulation of the weight-gradient kernel's arithmetic against its bound on every
input kind the GPU tests use, and ``bev_down_train``'s predicates on module objects."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests import bev_down_train_ref as ref

SIZES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (5, 4), (6, 6), (7, 7), (1, 6), (4, 1)]


@pytest.mark.parametrize("cin,cout", [(8, 12), (32, 64)])
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("zeropad", [False, True])
def test_statement_matches_autograd_in_float64(hw, cin, cout, zeropad):
    B, (H, W) = 2, hw
    xs, dys = ref.inputs("plain", B, H, W, cin, cout, seed=H + 10 * W + cin)
    ws = ref.weights(cin, cout, seed=cout)
    x = torch.from_numpy(xs).double().permute(0, 3, 1, 2).requires_grad_(True)
    w = torch.from_numpy(ws).double().requires_grad_(True)
    y = F.conv2d(nn.ZeroPad2d(1)(x), w, stride=2, padding=0) if zeropad else F.conv2d(x, w, stride=2, padding=1)
    assert tuple(y.shape[2:]) == ref.out_size(H, W) == tuple(dys.shape[1:3])
    y.backward(torch.from_numpy(dys).double().permute(0, 3, 1, 2))
    want_y, a_y, b_y = ref.y_ref(xs, ws)
    want_dx, a_dx, b_dx = ref.dx_phases(dys, ws, H, W)
    want_dw = ref.dw_ref(xs, dys)
    for got, want in ((y.detach().permute(0, 2, 3, 1), want_y), (x.grad.permute(0, 2, 3, 1), want_dx),
                      (x.grad.permute(0, 2, 3, 1), ref.dx_ref(dys, ws, H, W)), (w.grad, want_dw)):
        got = got.numpy()
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-13 * max(np.abs(want).max(), 1e-300)
    assert (a_y >= np.abs(want_y) * (1 - 1e-12)).all() and (a_dx >= np.abs(want_dx) * (1 - 1e-12)).all()
    assert (ref.dw_abs(xs, dys) >= np.abs(want_dw) * (1 - 1e-12)).all()
    assert (b_y > 0).all() and (b_dx > 0).all()
    # never looser than the 3 x 3 bound on the rotated weights
    assert (b_dx <= ref.dx_bound_3x3(a_dx, dys, ws)).all()


def test_the_phase_taps_are_the_nine_taps_each_used_once():
    assert [len(ref.PHASE_TAPS[p]) for p in ref.PHASES] == [1, 2, 2, 4]
    assert sorted((ky, kx) for p in ref.PHASES for ky, kx, _, _ in ref.PHASE_TAPS[p]) == ref.TAPS
    for (py, px), taps in ref.PHASE_TAPS.items():
        for ky, kx, oy, ox in taps:
            # pixel (2 j + py, 2 i + px) is read by output pixel (j + oy, i + ox) through tap (ky, kx)
            assert 2 * oy + ky - 1 == py and 2 * ox + kx - 1 == px
    for H in range(1, 8):
        assert sum(ref.phase_size(H, 3, py, 0)[0] for py in range(2)) == H
        assert ref.phase_size(H, 3, 0, 0)[0] == ref.out_size(H, 3)[0]


@pytest.mark.parametrize("hw", SIZES)
def test_four_phases_against_the_direct_sum_on_integers(hw):
    """On small integers both forms are exact: equal bit for bit, and the absent ky = 0 / kx = 0 tap of the last row / column of
    an even-sized input adds nothing."""
    H, W = hw
    Ho, Wo = ref.out_size(H, W)
    rng = np.random.default_rng(H * 8 + W)
    dy = rng.integers(-4, 5, (2, Ho, Wo, 5)).astype(np.float64)
    w = rng.integers(-4, 5, (5, 3, 3, 3)).astype(np.float64)
    np.testing.assert_array_equal(ref.dx_phases(dy, w, H, W)[0], ref.dx_ref(dy, w, H, W))


def test_tap_rows_follow_the_output_pixels():
    x = np.arange(2 * 4 * 5, dtype=np.float64).reshape(2, 4, 5, 1) + 1.0
    Ho, Wo = ref.out_size(4, 5)
    for ky, kx in ref.TAPS:
        rows, mask = ref.tap_rows(x, ky, kx)
        assert rows.shape == (2 * Ho * Wo, 1) and mask.shape == (2 * Ho * Wo,)
        for b in range(2):
            for oy in range(Ho):
                for ox in range(Wo):
                    iy, ix, m = 2 * oy + ky - 1, 2 * ox + kx - 1, (b * Ho + oy) * Wo + ox
                    inside = 0 <= iy < 4 and 0 <= ix < 5
                    assert bool(mask[m]) == inside and rows[m, 0] == (x[b, iy, ix, 0] if inside else 0.0)


def test_the_published_slice_lengths_cover_the_shapes():
    assert sorted(ref.SLICE_PIXELS) == sorted(ref.SHAPES)
    assert all(v % 32 == 0 for v in ref.SLICE_PIXELS.values())


def emulation_ratio(kind, B, H, W, cin, cout, seed):
    sl = ref.SLICE_PIXELS[(cin, cout)]
    x, dy = ref.inputs(kind, B, H, W, cin, cout, seed)
    err = np.abs(ref.dw_emulated(x, dy, sl).astype(np.float64) - ref.dw_ref(x, dy))
    bound = ref.dw_bound(x, dy, sl)
    assert (err <= bound).all(), (kind, (B, H, W), float((err / np.maximum(bound, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("kind", ["plain", "tail", "spike"])
def test_emulation_stays_inside_the_bound_narrow(kind):
    sl = ref.SLICE_PIXELS[(32, 64)]
    worst = 0.0
    # (the output grids: 1, 6, 12, 31 / 32 pixels, sl - 1, sl + 1, 2 sl + 1 and three samples of ~0.75 slices)
    for i, (B, H, W) in enumerate([(1, 1, 1), (3, 3, 4), (3, 4, 3), (1, 2, 61), (1, 1, 64), (1, 33, 29), (1, 1, 2 * sl + 1),
                                   (1, 5, 2 * (2 * sl + 1) // 3), (3, 17, 2 * (sl // 12))]):
        worst = max(worst, emulation_ratio(kind, B, H, W, 32, 64, seed=10 * i))
    print("emulation, %s, (32, 64): worst error / bound %.3f" % (kind, worst))
    assert worst < 1.0


@pytest.mark.parametrize("kind", ["plain", "tail", "spike"])
def test_emulation_stays_inside_the_bound_product(kind):
    sl = ref.SLICE_PIXELS[(128, 256)]
    worst = max(emulation_ratio(kind, 1, 2, 66, 128, 256, seed=1), emulation_ratio(kind, 1, 1, 2 * sl + 1, 128, 256, seed=2))
    print("emulation, %s, (128, 256): worst error / bound %.3f" % (kind, worst))
    assert worst < 1.0


# ---- the predicates on module objects ------------------------------------------------------------------------------------
def test_down_shape_on_module_objects():
    from mssvt_amd import bev_down_train as bdn
    assert bdn.SHAPES == ref.SHAPES and bdn.NARROW_SHAPES == {(32, 64)}
    assert bdn.ROUTED_DOWN_TRAIN <= {(128, 256)}
    assert bdn.down_shape(nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False)) == (32, 64)
    assert bdn.down_shape(nn.Conv2d(128, 256, 3, stride=2, padding=0, bias=False), 1) == (128, 256)
    assert bdn.down_shape(nn.Conv2d(5, 7, 3, stride=2, padding=1, bias=False)) == (5, 7)  # (the shape alone: coverage is the library's)
    for no, pad in ((nn.Conv2d(32, 64, 3, stride=2, padding=0, bias=False), None), (nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False), 0),
                    (nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=True), None), (nn.Conv2d(32, 64, 3, stride=1, padding=1, bias=False), None),
                    (nn.Conv2d(32, 64, 3, stride=2, padding=2, dilation=2, bias=False), None),
                    (nn.Conv2d(32, 64, 3, stride=2, padding=1, dilation=2, bias=False), None),
                    (nn.Conv2d(32, 64, 3, stride=(2, 1), padding=1, bias=False), None),
                    (nn.Conv2d(32, 64, 3, stride=2, padding=(1, 0), bias=False), None),
                    (nn.Conv2d(32, 64, 3, stride=2, padding=1, groups=2, bias=False), None),
                    (nn.Conv2d(32, 64, 3, stride=2, padding=1, padding_mode="reflect", bias=False), None),
                    (nn.Conv2d(32, 64, 1, stride=2, bias=False), None), (nn.Conv2d(32, 64, 2, stride=2, bias=False), None),
                    (nn.ConvTranspose2d(32, 64, 3, stride=2, padding=1, bias=False), None), (nn.ReLU(), None)):
        assert bdn.down_shape(no, pad) is None, (no, pad)
    # parameters on the CPU: never supported, never routed
    cpu = nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False)
    assert not bdn.down_train_supported(cpu) and not bdn.down_train_routed(cpu)


def test_routing_follows_the_sets_and_run_layers_train_sends_the_layer_to_down(monkeypatch):
    """With the library's side of the predicate replaced (the shape alone decides), routing is membership of ROUTED_DOWN_TRAIN or
    NARROW_SHAPES, and ``run_layers_train(..., fused_down=True)`` sends both spellings to ``bev_down_train.down`` -- never to
    ``conv3x3`` -- and neither without the argument."""
    from mssvt_amd import bev_conv_train, bev_down_train as bdn
    monkeypatch.setattr(bdn, "down_train_supported", lambda conv, pad=None: bdn.down_shape(conv, pad) in bdn.SHAPES)
    narrow = nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False)
    wide = nn.Conv2d(128, 256, 3, stride=2, padding=0, bias=False)
    other = nn.Conv2d(64, 64, 3, stride=2, padding=1, bias=False)
    assert bdn.down_train_routed(narrow) and not bdn.down_train_routed(other)
    monkeypatch.setattr(bdn, "ROUTED_DOWN_TRAIN", frozenset())
    assert not bdn.down_train_routed(wide, 1)
    monkeypatch.setattr(bdn, "ROUTED_DOWN_TRAIN", frozenset({(128, 256)}))
    assert bdn.down_train_routed(wide, 1) and not bdn.down_train_routed(wide)  # (padding 0 without the ZeroPad2d is another layer)
    calls = []

    def fake_down(conv, x):
        calls.append(conv)
        return F.conv2d(x, conv.weight, stride=2, padding=1)

    def never(conv, x):
        raise AssertionError("the stride-2 layer must not go through conv3x3")

    monkeypatch.setattr(bdn, "down", fake_down)
    monkeypatch.setattr(bev_conv_train, "conv3x3", never)
    x = torch.randn(1, 32, 5, 6)
    paired = nn.Conv2d(32, 64, 3, stride=2, padding=0, bias=False)
    for layers, conv in (([narrow, nn.ReLU()], narrow), ([nn.ZeroPad2d(1), paired, nn.ReLU()], paired)):
        want = nn.Sequential(*layers)(x)
        del calls[:]
        got = bev_conv_train.run_layers_train(layers, x, fused_down=True)
        assert calls == [conv] and torch.equal(got, want)
        del calls[:]
        assert torch.equal(bev_conv_train.run_layers_train(layers, x), want) and calls == []
    # a ZeroPad2d(1) in front of a padding-1 convolution: the pad stays a module, the convolution is routed on its own
    del calls[:]
    layers = [nn.ZeroPad2d(1), narrow]
    assert torch.equal(bev_conv_train.run_layers_train(layers, x, fused_down=True), nn.Sequential(*layers)(x)) and calls == [narrow]
