"""HeightCompression / BaseBEVBackbone / the whole CenterPoint detector with ``fused_convs`` on: against the reference-run
goldens (the tolerance the existing golden tests apply to the library path), against the switch-off run, and the
conditions under which the switch must have no effect."""
import os

import numpy as np
import pytest
import torch

from mssvt_amd import bev_conv, synthetic
from mssvt_amd.base_bev_backbone import BaseBEVBackbone
from mssvt_amd.config import Config
from mssvt_amd.height_compression import HeightCompression
from mssvt_amd.mssvt_utils import SparseTensor

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture
def kernel_calls(monkeypatch):
    """Counts the layers that really run on the kernel."""
    calls = []
    real = bev_conv.conv_bn_act

    def counted(x, packed, relu=True):
        calls.append((packed.ksize, packed.cin, packed.cout, packed.stride, packed.dilation))
        return real(x, packed, relu)

    monkeypatch.setattr(bev_conv, "conv_bn_act", counted)
    return calls


def close(got, want, rtol=1e-4, atol_rel=1e-4):
    got, want = got.float().cpu().numpy(), want.float().cpu().numpy()
    assert got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol_rel * max(1.0, float(np.abs(want).max())))


def sparse_grid(grid, B, C, seed, fill=0.3):
    g = torch.Generator().manual_seed(seed)
    X, Y, Z = grid
    rows = []
    for b in range(B):
        cells = torch.randperm(X * Y * Z, generator=g)[:max(1, int(fill * X * Y * Z))].sort().values
        x, y, z = cells // (Y * Z), (cells // Z) % Y, cells % Z
        rows.append(torch.stack([torch.full_like(x, b), z, y, x], dim=1))
    vc = torch.cat(rows).int()
    feats = torch.randn(vc.shape[0], C, generator=g).to(DEV)
    return SparseTensor(features=feats, indices=vc.to(DEV), spatial_shape=grid, voxel_size=[0.3, 0.3, 0.2],
                        point_cloud_range=[0, 0, 0, 0.3 * X, 0.3 * Y, 0.2 * Z], batch_size=B, hash_size=100003)


def randomise_batch_norms(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return module


# ---- against the reference-run goldens ---------------------------------------------------------------------------------
def golden_height_compression(golden_dir):
    d = np.load(os.path.join(golden_dir, "height_compression_convs.npz"))
    hc = HeightCompression(dict(NUM_BEV_FEATURES=int(d["num_bev_features"]), COMPRESS_LAYER_NUMS=int(d["layers"]),
                                LAYER_STRIDES=[1, 1], LAYER_DIALATIONS=[1, 2], LAYER_PADDINGS=[1, 2])).eval()
    hc.load_state_dict({k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd.")}, strict=True)
    sp = SparseTensor(features=torch.from_numpy(d["features"]).to(DEV), indices=torch.from_numpy(d["indices"]).to(DEV),
                      spatial_shape=d["spatial_shape"].tolist(), voxel_size=[1.0, 1.0, 1.0],
                      point_cloud_range=[0, 0, 0, 1, 1, 1], batch_size=int(d["batch_size"]), hash_size=int(d["hash_size"]))
    return d, hc.to(DEV), sp


def test_height_compression_switch_on_matches_the_reference_run(golden_dir):
    """The golden's layers have 48 channels: the grid arrives channels-last from mssvt_dense_bev_nhwc and both layers run
    through the library on it; tolerance of tests/test_module_gpu.py::test_height_compression_matches_the_reference_run."""
    d, hc, sp = golden_height_compression(golden_dir)
    assert hc.fused_convs is False
    hc.fused_convs = True
    with torch.no_grad():
        out = hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1))
    got, want = out["spatial_features"], d["spatial_features"]
    assert bev_conv.is_channels_last(got) and out["spatial_features_stride"] == int(d["stride"]) and tuple(got.shape) == want.shape
    assert np.abs(got.cpu().numpy() - want).max() <= 1e-4 * max(1.0, np.abs(want).max())


def test_bev_backbone_switch_on_matches_the_reference_run(golden_dir, kernel_calls):
    """det_bev_head.npz: the 48 -> 32 first layer and the 2 x 2 stride-2 transposed deblock go through the library, the other
    six layers (32 -> 32, 32 -> 64 at stride 2, 64 -> 64, the 1 x 1 deblock) through the kernel; tolerance of
    tests/test_detector_gpu.py::test_center_head_with_the_hip_nms_matches_the_reference_run."""
    from tests.test_detector_cpu import build_from_golden
    d, bev, _ = build_from_golden(golden_dir)
    bev = bev.to(DEV)
    bev.fused_convs = True
    with torch.no_grad():
        out = bev(dict(spatial_features=torch.from_numpy(d["spatial_features"]).to(DEV)))
    assert sorted(kernel_calls) == sorted([(3, 32, 32, 1, 1)] * 2 + [(3, 32, 64, 2, 1)] + [(3, 64, 64, 1, 1)] * 2 + [(1, 32, 32, 1, 1)])
    f2d = out["spatial_features_2d"]
    assert bev_conv.is_channels_last(f2d) and f2d.dtype == torch.float32
    np.testing.assert_allclose(f2d.cpu().numpy(), d["spatial_features_2d"], rtol=1e-4, atol=5e-5)
    assert set(out) == {"spatial_features", "spatial_features_1x", "spatial_features_2x", "spatial_features_2d"}


# ---- switch on against switch off --------------------------------------------------------------------------------------
def test_golden_sized_modules_on_random_inputs_on_versus_off(golden_dir, kernel_calls):
    from tests.test_detector_cpu import build_from_golden
    d, bev, _ = build_from_golden(golden_dir)
    bev = randomise_batch_norms(bev, 3).to(DEV)
    x = torch.randn(2, 48, 64, 64, generator=torch.Generator().manual_seed(1)).clamp_(min=0).to(DEV)
    with torch.no_grad():
        off = bev(dict(spatial_features=x))
        bev.fused_convs = True
        on = bev(dict(spatial_features=x))
    assert len(kernel_calls) == 6 and off["spatial_features_2d"].is_contiguous()
    for k in ("spatial_features_1x", "spatial_features_2x", "spatial_features_2d"):
        close(on[k], off[k])
    _, hc, sp = golden_height_compression(golden_dir)
    sp.features = torch.randn(sp.features.shape, generator=torch.Generator().manual_seed(2)).to(DEV)
    with torch.no_grad():
        off = hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1))["spatial_features"]
        hc.fused_convs = True
        on = hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1))["spatial_features"]
    close(on, off)


def product_modules(plain=False):
    """mssvt.yaml's channel counts with one layer per block; `plain`: only undilated stride-1 128 -> 128 layers."""
    torch.manual_seed(4)
    d3 = 1 if plain else 2
    hc = HeightCompression(Config.wrap(dict(NUM_BEV_FEATURES=128, COMPRESS_LAYER_NUMS=3, LAYER_STRIDES=[1, 1, 1],
                                            LAYER_DIALATIONS=[1, 1, d3], LAYER_PADDINGS=[1, 1, d3], FUSED_CONVS=True)))
    if plain:
        bev = BaseBEVBackbone(Config.wrap(dict(LAYER_NUMS=[1], LAYER_STRIDES=[1], NUM_FILTERS=[128], FUSED_CONVS=True)), 128)
    else:
        bev = BaseBEVBackbone(Config.wrap(dict(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=[128, 256],
                                               UPSAMPLE_STRIDES=[1, 2], NUM_UPSAMPLE_FILTERS=[256, 256], FUSED_CONVS=True)), 128)
    assert hc.fused_convs is True and bev.fused_convs is True  # the yaml key
    return randomise_batch_norms(hc, 5).to(DEV).eval(), randomise_batch_norms(bev, 6).to(DEV).eval()


def test_product_channel_counts_on_a_40_grid_on_versus_off(kernel_calls):
    """128 / 256 channels as in mssvt.yaml on a 40 x 40 grid: the layers ROUTED names run on the kernel, the rest through the
    library; both modules agree with their switch-off runs."""
    hc, bev = product_modules()
    sp = sparse_grid([40, 40, 1], 2, 128, seed=7)
    layers = [(3, 128, 128, 1, 1), (3, 128, 128, 1, 1), (3, 128, 128, 1, 2),  # HeightCompression
              (3, 128, 128, 1, 1), (3, 128, 128, 1, 1), (3, 128, 256, 2, 1), (3, 256, 256, 1, 1), (1, 128, 256, 1, 1)]
    with torch.no_grad():
        on = bev(hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1)))
        assert sorted(kernel_calls) == sorted(s for s in layers if s in bev_conv.ROUTED)
        hc.fused_convs = bev.fused_convs = False
        off = bev(hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1)))
    assert tuple(on["spatial_features_2d"].shape) == (2, 512, 40, 40)
    for k in ("spatial_features", "spatial_features_1x", "spatial_features_2x", "spatial_features_2d"):
        close(on[k], off[k])
        assert off[k].is_contiguous() and bev_conv.is_channels_last(on[k])


@pytest.mark.parametrize("why", ["train", "autograd", "amp"])
def test_switch_has_no_effect_in_train_mode_with_autograd_or_amp(why, kernel_calls):
    """Today's path runs: the output is the switch-off run's, bit for bit and stride for stride, and no layer reaches the kernel.
    The modules hold undilated stride-1 128 -> 128 layers only: identity can show something only where the library itself
    repeats its bits from call to call, which it does for these and does NOT for the dilated layer at this size (measured on
    an MI355X, switch off both times, train and eval mode alike: the third compression layer's output moved by up to 1.4e-6
    between calls, the two before it not at all).  That premise is asserted too."""
    hc, bev = product_modules(plain=True)
    sp = sparse_grid([24, 24, 1], 2, 128, seed=8)

    def forward():
        if why == "train":
            hc.train(), bev.train()
        if why == "amp":
            hc.use_amp = bev.use_amp = True
        ctx = torch.enable_grad() if why == "autograd" else torch.no_grad()
        with ctx:
            return bev(hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1)))

    state = [{k: v.clone() for k, v in m.state_dict().items()} for m in (hc, bev)]

    def restore():  # (train mode moves the running statistics)
        hc.load_state_dict(state[0]), bev.load_state_dict(state[1])

    forward()  # the library settles on its algorithms for these shapes during a first call
    restore()
    on = forward()
    assert kernel_calls == []
    restore()
    hc.fused_convs = bev.fused_convs = False
    off = forward()
    restore()
    off2 = forward()
    for k in ("spatial_features", "spatial_features_2d"):
        assert torch.equal(off[k], off2[k]), "the library path does not repeat itself: " + k
        assert torch.equal(on[k], off[k]) and on[k].stride() == off[k].stride() and on[k].is_contiguous()


def test_packed_cache_follows_load_state_dict_and_in_place_changes(kernel_calls):
    hc, _ = product_modules()
    sp = sparse_grid([16, 16, 1], 1, 128, seed=9)
    conv, norm = hc.compress_layers[0], hc.compress_layers[1]

    def first_layer():
        with torch.no_grad():
            return bev_conv.conv_bn_act(sp.dense_nhwc(), bev_conv.pack(conv, norm), True), torch.relu(norm(conv(sp.dense()[:, :, 0])))

    p0 = bev_conv.pack(conv, norm)
    got, want = first_layer()
    close(got, want)
    assert bev_conv.pack(conv, norm) is p0
    sd = {k: v.clone() for k, v in hc.state_dict().items()}
    sd["compress_layers.0.weight"] *= -0.5
    sd["compress_layers.1.running_mean"] += 1.0
    hc.load_state_dict(sd)
    assert bev_conv.pack(conv, norm) is not p0
    got2, want2 = first_layer()
    close(got2, want2)
    assert not torch.equal(got2, got)
    with torch.no_grad():
        norm.weight.mul_(3.0)  # what an optimizer step does
    got3, want3 = first_layer()
    close(got3, want3)
    assert not torch.equal(got3, got2)


# ---- the whole detector ------------------------------------------------------------------------------------------------
def test_detector_from_points_to_boxes_with_the_switch_on():
    """mssvt.yaml with FUSED_CONVS on both dense modules: the boxes of the switch-off run, within the tolerance the detector
    tests use for box lists (tests/test_detector_cpu.py::check_against_golden)."""
    from mssvt_amd import centerpoint, config
    cfg = config.load_yaml(config.DEFAULT_CFG)
    cfg.MODEL.MAP_TO_BEV["FUSED_CONVS"] = True
    cfg.MODEL.BACKBONE_2D["FUSED_CONVS"] = True
    torch.manual_seed(0)
    det = centerpoint.build_detector(cfg).to(DEV).eval()
    assert det.map_to_bev_module.fused_convs and det.backbone_2d.fused_convs
    with torch.no_grad():
        for h in det.dense_head.heads_list:  # random init: lift the heat map above the score threshold
            h.hm[-1].bias.fill_(0.5)
    B = 2
    pts = torch.from_numpy(synthetic.make_batch_points(40000, B, 123)).to(DEV)
    with torch.no_grad():
        on, _ = det(dict(points=pts, batch_size=B))
        det.map_to_bev_module.fused_convs = det.backbone_2d.fused_convs = False
        off, _ = det(dict(points=pts, batch_size=B))
    rows = lambda p: np.concatenate([p["pred_boxes"].cpu().numpy(), p["pred_labels"].cpu().numpy()[:, None].astype(np.float32)], 1)  # noqa: E731
    for p, q in zip(on, off):
        assert 0 < q["pred_boxes"].shape[0] and p["pred_boxes"].shape == q["pred_boxes"].shape
        np.testing.assert_allclose(p["pred_scores"].cpu().numpy(), q["pred_scores"].cpu().numpy(), rtol=1e-4, atol=5e-5)
        g, w = rows(p), rows(q)
        g, w = g[np.lexsort((g[:, 1], g[:, 0]))], w[np.lexsort((w[:, 1], w[:, 0]))]
        np.testing.assert_allclose(g, w, rtol=1e-4, atol=1e-4)
