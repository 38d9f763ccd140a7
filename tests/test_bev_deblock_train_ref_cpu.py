"""tests/bev_deblock_train_ref.py against torch's autograd in float64, and its emulation of the weight-gradient kernel's
arithmetic against its bound on every input kind the GPU tests use."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bev_deblock_train_ref as ref


@pytest.mark.parametrize("s,cin,cout", [(1, 8, 12), (2, 12, 8), (1, 32, 64), (2, 64, 32)])
def test_statement_matches_autograd_in_float64(s, cin, cout):
    B, H, W = 2, 5, 7
    xs, dys = ref.inputs("plain", B, H, W, s, cin, cout, seed=s + cin)
    ws = ref.weights(s, cin, cout, seed=cout)
    x = torch.from_numpy(xs).double().permute(0, 3, 1, 2).requires_grad_(True)
    w = torch.from_numpy(ws).double().requires_grad_(True)
    y = F.conv_transpose2d(x, w, stride=s)
    y.backward(torch.from_numpy(dys).double().permute(0, 3, 1, 2))
    want_y, a_y, b_y = ref.y_ref(xs, ws, s)
    want_dx, a_dx, b_dx = ref.dx_ref(dys, ws, s)
    want_dw = ref.dw_ref(xs, dys, s)
    for got, want in ((y.detach().permute(0, 2, 3, 1), want_y), (x.grad.permute(0, 2, 3, 1), want_dx), (w.grad, want_dw)):
        got = got.numpy()
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()
    assert (a_y >= np.abs(want_y) * (1 - 1e-12)).all() and (a_dx >= np.abs(want_dx) * (1 - 1e-12)).all()
    assert (ref.dw_abs(xs, dys, s) >= np.abs(want_dw) * (1 - 1e-12)).all()
    assert (b_y > 0).all() and (b_dx > 0).all()


def test_phase_rows_follow_the_input_pixels():
    dy = np.arange(2 * 4 * 6 * 1, dtype=np.float64).reshape(2, 4, 6, 1)
    rows = ref.phase_rows(dy, 2, 1, 0)
    assert rows.shape == (12, 1)
    for b in range(2):
        for iy in range(2):
            for ix in range(3):
                assert rows[(b * 2 + iy) * 3 + ix, 0] == dy[b, 2 * iy + 1, 2 * ix, 0]


def test_the_published_slice_lengths_cover_the_shapes():
    assert sorted(ref.SLICE_PIXELS) == sorted(ref.SHAPES)
    assert all(v % 32 == 0 for v in ref.SLICE_PIXELS.values())


def emulation_ratio(kind, B, H, W, s, cin, cout, seed):
    sl = ref.SLICE_PIXELS[(s, cin, cout)]
    x, dy = ref.inputs(kind, B, H, W, s, cin, cout, seed)
    err = np.abs(ref.dw_emulated(x, dy, s, sl).astype(np.float64) - ref.dw_ref(x, dy, s))
    bound = ref.dw_bound(x, dy, s, sl)
    assert (err <= bound).all(), (kind, (B, H, W), float((err / np.maximum(bound, 1e-300)).max()))
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("s,cin,cout", [(1, 32, 64), (2, 64, 32)])
@pytest.mark.parametrize("kind", ["plain", "tail", "spike"])
def test_emulation_stays_inside_the_bound_narrow(kind, s, cin, cout):
    sl = ref.SLICE_PIXELS[(s, cin, cout)]
    worst = 0.0
    for i, (B, H, W) in enumerate([(1, 1, 1), (3, 5, 7), (1, 1, 31), (1, 1, 33), (1, 1, sl - 1), (1, 1, sl + 1), (1, 3, (2 * sl + 1) // 3),
                                   (3, 9, sl // 12)]):
        worst = max(worst, emulation_ratio(kind, B, H, W, s, cin, cout, seed=10 * i + s))
    print("emulation, %s, (%d, %d, %d): worst error / bound %.3f" % (kind, s, cin, cout, worst))
    assert worst < 1.0


@pytest.mark.parametrize("s,cin,cout", [(1, 128, 256), (2, 256, 256)])
@pytest.mark.parametrize("kind", ["plain", "tail", "spike"])
def test_emulation_stays_inside_the_bound_product(kind, s, cin, cout):
    sl = ref.SLICE_PIXELS[(s, cin, cout)]
    worst = max(emulation_ratio(kind, 1, 1, 33, s, cin, cout, seed=1), emulation_ratio(kind, 1, 1, sl + 1, s, cin, cout, seed=2))
    print("emulation, %s, (%d, %d, %d): worst error / bound %.3f" % (kind, s, cin, cout, worst))
    assert worst < 1.0
