"""tests/bev_conv_train_ref.py held to torch autograd in float64 on the CPU, and a numpy emulation of the kernel's split
arithmetic (fp16 halves rounded to nearest, fp32 accumulation per 32-pixel step, per-slice powers of two, ordered slice sums)
kept inside the bound the GPU tests hold the kernel to."""
import numpy as np
import pytest
import torch

from tests import bev_conv_train_ref as ref


@pytest.mark.parametrize("d", [1, 2])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 2, 3), (3, 5, 7), (2, 4, 9)])
def test_statement_is_autograd_of_conv2d_in_float64(B, H, W, d):
    rng = np.random.default_rng(B * H * W + d)
    cin, cout = 5, 6
    x = rng.standard_normal((B, H, W, cin))
    w = rng.standard_normal((cout, cin, 3, 3))
    dy = rng.standard_normal((B, H, W, cout))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w).requires_grad_(True)
    y = torch.nn.functional.conv2d(xt, wt, padding=d, dilation=d)
    y.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    np.testing.assert_allclose(ref.dw_ref(x, dy, d), wt.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.dx_ref(dy, w, d), xt.grad.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.dw_abs(x, dy, d), ref.dw_ref(np.abs(x), np.abs(dy), d), rtol=0, atol=0)
    assert (np.abs(ref.dw_ref(x, dy, d)) <= ref.dw_abs(x, dy, d) + 1e-12).all()


def test_tap_rows_zero_fill_and_mask():
    x = np.arange(1, 1 + 2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4, 1)
    rows, mask = ref.tap_rows(x, 0, 2, 1)  # reads (y - 1, x + 1)
    rows, mask = rows.reshape(2, 3, 4), mask.reshape(2, 3, 4)
    assert not mask[:, 0].any() and not mask[:, :, 3].any() and mask[:, 1:, :3].all()
    assert (rows[~mask] == 0).all() and rows[1, 2, 0] == x[1, 1, 1, 0]
    rows, mask = ref.tap_rows(x, 2, 1, 4)  # a dilation past the image: nothing inside
    assert not mask.any() and not rows.any()


@pytest.mark.parametrize("kind", ["plain", "tail", "spike"])
@pytest.mark.parametrize("B,H,W,sl,d", [(1, 16, 64, 256, 1), (2, 25, 50, 512, 2), (1, 1, 257, 256, 1)])
def test_emulated_split_arithmetic_stays_inside_the_bound(kind, B, H, W, sl, d):
    x, dy = ref.inputs(kind, B, H, W, 16, 24, seed=H + W)
    got = ref.dw_emulated(x, dy, d, sl)
    err = np.abs(got.astype(np.float64) - ref.dw_ref(x, dy, d))
    bound = ref.dw_bound(x, dy, d, sl)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s %s slices of %d: worst error / bound %.3f" % (kind, (B, H, W), sl, ratio))
    assert (err <= bound).all(), ratio
    assert ratio > 1e-4  # (the bound is not vacuous: the arithmetic's error shows on its scale)


def test_emulation_scales_exactly_by_powers_of_two():
    x, dy = ref.inputs("plain", 1, 9, 40, 16, 16, seed=1)
    base = ref.dw_emulated(x, dy, 1, 256)
    assert np.array_equal(ref.dw_emulated(x * np.float32(2.0 ** 18), dy, 1, 256), base * np.float32(2.0 ** 18))
    assert np.array_equal(ref.dw_emulated(x, dy * np.float32(2.0 ** -20), 1, 256), base * np.float32(2.0 ** -20))


def test_routed_train_is_what_the_recorded_runs_cleared():
    """ROUTED_TRAIN against profiles/bev_conv_train_times.json, the rule recomputed from the recorded runs: a shape is routed
    only where the Function's slowest run beat the library's fastest (over both layouts) at every batch size."""
    import json
    import os
    from mssvt_amd import bev_conv_train
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bev_conv_train_times.json")
    with open(path) as f:
        prof = json.load(f)
    cleared = {}
    for r in prof["layers"]:
        key = (r["ksize"], r["cin"], r["cout"], r["stride"], r["dilation"])
        ok = max(r["ms"]["hip"]) < min(r["ms"]["library_nchw"] + r["ms"]["library_nhwc"])
        assert ok == r["cleared"] and len(r["ms"]["hip"]) >= 5
        cleared[key] = cleared.get(key, True) and ok
    assert {r["B"] for r in prof["layers"]} == {1, 4}
    assert bev_conv_train.ROUTED_TRAIN == frozenset(k for k, ok in cleared.items() if ok)
    assert sorted(tuple(s) for s in prof["routed"]) == sorted(bev_conv_train.ROUTED_TRAIN)
    assert sorted(tuple(s) for s in prof["routed_in_package"]) == sorted(bev_conv_train.ROUTED_TRAIN)
