"""tests/bev_up2_ref.py (the float64 statement the GPU tests hold mssvt_bev_up2 to) against
torch.nn.functional.conv_transpose2d + BatchNorm2d.eval() in float64 on the CPU; what ``bev_conv.up2_shape`` accepts; the
``fused_deblocks`` switch of BaseBEVBackbone on the CPU."""
import numpy as np
import pytest
import torch
from torch import nn

from tests import bev_up2_ref as ref


@pytest.mark.parametrize("cin,cout", [(64, 32), (256, 256)])
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 7)])
def test_statement_matches_torch_in_float64(cin, cout, hw):
    rng = np.random.default_rng(cin + 10 * hw[0] + hw[1])
    B = 3
    x = rng.normal(size=(B,) + hw + (cin,))
    w = rng.normal(size=(cin, cout, 2, 2))
    bias = rng.normal(size=cout) if hw[0] % 2 else None
    bn = dict(mean=rng.normal(0, 0.5, cout), var=rng.uniform(0.3, 2.0, cout), eps=1e-3, weight=rng.uniform(0.5, 1.5, cout),
              bias=rng.normal(0, 0.3, cout))
    scale, shift = ref.fold(cout, bias, bn)
    m = nn.BatchNorm2d(cout, eps=bn["eps"]).double().eval()
    with torch.no_grad():
        m.running_mean.copy_(torch.from_numpy(bn["mean"]))
        m.running_var.copy_(torch.from_numpy(bn["var"]))
        m.weight.copy_(torch.from_numpy(bn["weight"]))
        m.bias.copy_(torch.from_numpy(bn["bias"]))
    for relu in (False, True):
        got, a = ref.up2(x, w, scale, shift, relu)
        with torch.no_grad():
            t = torch.nn.functional.conv_transpose2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w),
                                                     None if bias is None else torch.from_numpy(bias), stride=2)
            t = m(t)
            t = torch.relu(t) if relu else t
            ta = torch.nn.functional.conv_transpose2d(torch.from_numpy(np.abs(x)).permute(0, 3, 1, 2), torch.from_numpy(np.abs(w)),
                                                      None, stride=2)
        want = t.permute(0, 2, 3, 1).numpy()
        assert got.shape == want.shape == (B, 2 * hw[0], 2 * hw[1], cout)
        tol = 1e-12 * max(1.0, float(np.abs(want).max()))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=tol)
        np.testing.assert_allclose(a, ta.permute(0, 2, 3, 1).numpy(), rtol=1e-12, atol=tol)
    bound = ref.error_bound(a, x, w)
    assert bound.shape == a.shape and (bound > 0).all() and ref.steps(cin) == cin // 32 + 2


def test_up2_shape_accepts_exactly_kernel_2_stride_2():
    from mssvt_amd import bev_conv
    assert bev_conv.up2_shape(nn.ConvTranspose2d(256, 256, 2, stride=2, bias=False)) == (256, 256)
    assert bev_conv.up2_shape(nn.ConvTranspose2d(64, 32, 2, stride=2)) == (64, 32)
    assert bev_conv.up2_shape(nn.ConvTranspose2d(48, 40, 2, stride=2)) == (48, 40)  # (the shape; `up2_supported` asks the library)
    for other in (nn.ConvTranspose2d(256, 256, 2, stride=1), nn.ConvTranspose2d(256, 256, 1, stride=1),
                  nn.ConvTranspose2d(256, 256, 4, stride=4), nn.ConvTranspose2d(256, 256, 3, stride=2),
                  nn.ConvTranspose2d(256, 256, 2, stride=2, padding=1), nn.ConvTranspose2d(256, 256, 2, stride=2, output_padding=1),
                  nn.ConvTranspose2d(256, 256, 2, stride=2, dilation=2), nn.ConvTranspose2d(256, 256, 2, stride=2, groups=2),
                  nn.ConvTranspose2d(256, 256, (2, 1), stride=(2, 1)), nn.Conv2d(256, 256, 2, stride=2), nn.ReLU()):
        assert bev_conv.up2_shape(other) is None, other
    # the 1 x 1 family keeps its meaning
    assert bev_conv.layer_shape(nn.ConvTranspose2d(256, 256, 2, stride=2, bias=False)) is None
    assert not bev_conv.up2_supported(nn.ConvTranspose2d(256, 256, 2, stride=2, bias=False))  # parameters on the CPU
    assert isinstance(bev_conv.ROUTED_UP2, frozenset) and bev_conv.ROUTED_UP2 <= {(256, 256)}
    assert bev_conv.GOLDEN_UP2 == frozenset({(64, 32)})
    from mssvt_amd import _lib
    assert set(bev_conv.UP2_CHANNEL_SHAPES) == {(256, 256), (64, 32)} >= bev_conv.ROUTED_UP2 | bev_conv.GOLDEN_UP2
    for cin, cout in bev_conv.UP2_CHANNEL_SHAPES:
        assert _lib.lib().mssvt_bev_up2_supported(cin, cout) == 1
        assert _lib.lib().mssvt_bev_up2_pack_bytes(cin, cout) == 64 + 32 * cout + 16 * cin * cout
    assert _lib.lib().mssvt_bev_up2_supported(128, 256) == 0 and _lib.lib().mssvt_bev_up2_pack_bytes(128, 256) == 0


def _backbone(**keys):
    from mssvt_amd.base_bev_backbone import BaseBEVBackbone
    from mssvt_amd.config import Config
    torch.manual_seed(2)
    cfg = dict(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=[32, 64], UPSAMPLE_STRIDES=[1, 2], NUM_UPSAMPLE_FILTERS=[32, 32])
    cfg.update(keys)
    return BaseBEVBackbone(Config.wrap(cfg), 32).eval()


def test_yaml_key_sets_the_switch_and_it_is_off_by_default():
    assert _backbone().fused_deblocks is False and _backbone(FUSED_CONVS=True).fused_deblocks is False
    on = _backbone(FUSED_CONVS=True, FUSED_DEBLOCKS=True)
    assert on.fused_deblocks is True and on.fused_convs is True
    assert _backbone(FUSED_DEBLOCKS=True).fused_convs is False
    from mssvt_amd import config
    cfg = config.load_yaml(config.DEFAULT_CFG)
    assert not cfg.MODEL.BACKBONE_2D.get("FUSED_DEBLOCKS", False)  # the product configuration does not turn it on by itself


def test_on_the_cpu_the_switch_has_no_effect_bit_for_bit():
    off, on = _backbone(), _backbone(FUSED_CONVS=True, FUSED_DEBLOCKS=True)
    on.load_state_dict(off.state_dict())
    x = torch.randn(2, 32, 12, 10, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        a, b = off(dict(spatial_features=x)), on(dict(spatial_features=x))
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]) and a[k].stride() == b[k].stride(), k
    assert tuple(b["spatial_features_2d"].shape) == (2, 64, 12, 10)
