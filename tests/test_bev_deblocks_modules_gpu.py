"""BaseBEVBackbone with ``fused_deblocks`` on (every deblock writes its channel slice of the concatenated tensor, the 2 x 2
stride-2 transposed one on the split-fp16 kernel, no torch.cat): against the reference-run golden, against the switch-off
run, the conditions under which the switch must have no effect, and the whole detector."""
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
def calls(monkeypatch):
    """What really runs: ("conv", shape, channel or None), ("up2", (cin, cout), channel or None), ("cat",)."""
    seen = []
    conv, up2, cat = bev_conv.conv_bn_act, bev_conv.up2_bn_act, torch.cat

    def conv_(x, packed, relu=True, out=None, channel=0):
        seen.append(("conv", (packed.ksize, packed.cin, packed.cout, packed.stride, packed.dilation), None if out is None else channel))
        return conv(x, packed, relu, out=out, channel=channel)

    def up2_(x, packed, relu=True, out=None, channel=0):
        seen.append(("up2", (packed.cin, packed.cout), None if out is None else channel))
        return up2(x, packed, relu, out=out, channel=channel)

    def cat_(*a, **k):
        seen.append(("cat",))
        return cat(*a, **k)

    monkeypatch.setattr(bev_conv, "conv_bn_act", conv_)
    monkeypatch.setattr(bev_conv, "up2_bn_act", up2_)
    monkeypatch.setattr(torch, "cat", cat_)
    return seen


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


def product_modules(**keys):
    """mssvt.yaml's channel counts with one layer per block."""
    torch.manual_seed(4)
    d3 = 2
    hc = HeightCompression(Config.wrap(dict(NUM_BEV_FEATURES=128, COMPRESS_LAYER_NUMS=3, LAYER_STRIDES=[1, 1, 1],
                                            LAYER_DIALATIONS=[1, 1, d3], LAYER_PADDINGS=[1, 1, d3], FUSED_CONVS=True)))
    bev = BaseBEVBackbone(Config.wrap(dict(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=[128, 256], UPSAMPLE_STRIDES=[1, 2],
                                           NUM_UPSAMPLE_FILTERS=[256, 256], FUSED_CONVS=True, FUSED_DEBLOCKS=True, **keys)), 128)
    assert bev.fused_convs is True and bev.fused_deblocks is True  # the yaml keys
    return randomise_batch_norms(hc, 5).to(DEV).eval(), randomise_batch_norms(bev, 6).to(DEV).eval()


def test_golden_backbone_with_both_switches_on_matches_the_reference_run(golden_dir, calls):
    """det_bev_head.npz: the 1 x 1 32 -> 32 deblock writes channels [0, 32), the 2 x 2 stride-2 64 -> 32 one channels [32, 64) on
    the up-2 kernel; tolerance of tests/test_bev_conv_modules_gpu.py::test_bev_backbone_switch_on_matches_the_reference_run."""
    from tests.test_detector_cpu import build_from_golden
    d, bev, _ = build_from_golden(golden_dir)
    bev = bev.to(DEV)
    assert bev.fused_deblocks is False
    bev.fused_convs = bev.fused_deblocks = True
    with torch.no_grad():
        out = bev(dict(spatial_features=torch.from_numpy(d["spatial_features"]).to(DEV)))
    assert ("conv", (1, 32, 32, 1, 1), 0) in calls and ("up2", (64, 32), 32) in calls and ("cat",) not in calls
    assert sorted(c[1] for c in calls if c[0] == "conv" and c[2] is None) == \
        sorted([(3, 32, 32, 1, 1)] * 2 + [(3, 32, 64, 2, 1)] + [(3, 64, 64, 1, 1)] * 2)
    f2d = out["spatial_features_2d"]
    assert bev_conv.is_channels_last(f2d) and f2d.dtype == torch.float32
    np.testing.assert_allclose(f2d.cpu().numpy(), d["spatial_features_2d"], rtol=1e-4, atol=5e-5)
    assert set(out) == {"spatial_features", "spatial_features_1x", "spatial_features_2x", "spatial_features_2d"}


@pytest.mark.parametrize("routed_up2", [True, False])
def test_product_channel_counts_on_a_40_grid_on_versus_off(routed_up2, calls, monkeypatch):
    """128 / 256 channels as in mssvt.yaml on a 40 x 40 grid, B = 2: with the 2 x 2 deblock on the kernel, and with it taken out
    of ROUTED_UP2 (the library's result copied into its slice) -- both agree with the switch-off run, neither calls torch.cat."""
    monkeypatch.setattr(bev_conv, "ROUTED_UP2", frozenset({(256, 256)}) if routed_up2 else frozenset())
    hc, bev = product_modules()
    sp = sparse_grid([40, 40, 1], 2, 128, seed=7)
    with torch.no_grad():
        feats = hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1))
        del calls[:]
        on = bev(dict(feats))
        seen = list(calls)
        bev.fused_deblocks = False
        convs = bev(dict(feats))
        assert ("cat",) in calls  # (the premise: today's fused path concatenates)
        hc.fused_convs = bev.fused_convs = False
        off = bev(hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1)))
    assert ("cat",) not in seen and ("conv", (1, 128, 256, 1, 1), 0) in seen
    assert (("up2", (256, 256), 256) in seen) == routed_up2 and len([c for c in seen if c[0] == "up2"]) == int(routed_up2)
    assert tuple(on["spatial_features_2d"].shape) == (2, 512, 40, 40) and set(on) == set(off) == set(convs)
    for k in ("spatial_features_1x", "spatial_features_2x", "spatial_features_2d"):
        close(on[k], off[k])
        assert off[k].is_contiguous() and bev_conv.is_channels_last(on[k]) and on[k].stride() == convs[k].stride()
    # the 1 x 1 deblock's half is the fused_convs run bit for bit (the into-form has the allocating form's bits)
    assert torch.equal(on["spatial_features_2d"][:, :256], convs["spatial_features_2d"][:, :256])
    close(on["spatial_features_2d"][:, 256:], convs["spatial_features_2d"][:, 256:])


@pytest.mark.parametrize("why", ["no_fused_convs", "train", "autograd", "amp"])
def test_switch_has_no_effect_without_fused_convs_in_train_mode_with_autograd_or_amp(why, calls):
    """The switch-off run, bit for bit and stride for stride; nothing reaches the kernels and torch.cat runs as it does today.
    The module has the golden's channel counts (32 / 64, a 1 x 1 and a 2 x 2 stride-2 deblock): identity can show something
    only where the library itself repeats its bits from call to call, which on an MI355X at this grid it does for every layer
    of these widths and does NOT for the 3 x 3 stride-2 128 -> 256, the 3 x 3 256 -> 256 and the 2 x 2 256 -> 256 layers of the
    product widths (six calls each, eval and train mode alike).  That premise is asserted too."""
    torch.manual_seed(4)
    bev = BaseBEVBackbone(Config.wrap(dict(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=[32, 64], UPSAMPLE_STRIDES=[1, 2],
                                           NUM_UPSAMPLE_FILTERS=[32, 32], FUSED_CONVS=why != "no_fused_convs", FUSED_DEBLOCKS=True)), 32)
    bev = randomise_batch_norms(bev, 6).to(DEV).eval()
    assert bev.fused_deblocks is True and bev.fused_convs is (why != "no_fused_convs")
    x = torch.randn(2, 32, 24, 24, generator=torch.Generator().manual_seed(8)).clamp_(min=0).to(DEV)

    def forward():
        if why == "train":
            bev.train()
        if why == "amp":
            bev.use_amp = True
        ctx = torch.enable_grad() if why == "autograd" else torch.no_grad()
        with ctx:
            return bev(dict(spatial_features=x))

    state = {k: v.clone() for k, v in bev.state_dict().items()}  # (train mode moves the running statistics)
    forward()  # the library settles on its algorithms for these shapes during a first call
    bev.load_state_dict(state)
    del calls[:]
    on = forward()
    assert calls == [("cat",)]
    bev.load_state_dict(state)
    bev.fused_convs = bev.fused_deblocks = False
    off = forward()
    bev.load_state_dict(state)
    off2 = forward()
    assert set(on) == set(off)
    for k in ("spatial_features_1x", "spatial_features_2x", "spatial_features_2d"):
        assert torch.equal(off[k], off2[k]), "the library path does not repeat itself: " + k
        assert torch.equal(on[k], off[k]) and on[k].stride() == off[k].stride() and on[k].is_contiguous() and on[k].dtype == off[k].dtype


def test_a_single_block_module_keeps_the_fused_convs_path(calls):
    """One block: nothing to concatenate, the switch changes nothing."""
    torch.manual_seed(3)
    bev = BaseBEVBackbone(Config.wrap(dict(LAYER_NUMS=[1], LAYER_STRIDES=[1], NUM_FILTERS=[32], UPSAMPLE_STRIDES=[1],
                                           NUM_UPSAMPLE_FILTERS=[32], FUSED_CONVS=True, FUSED_DEBLOCKS=True)), 32)
    bev = randomise_batch_norms(bev, 7).to(DEV).eval()
    x = torch.randn(2, 32, 12, 10, generator=torch.Generator().manual_seed(1)).clamp_(min=0).to(DEV)
    with torch.no_grad():
        on = bev(dict(spatial_features=x))
        seen = list(calls)
        bev.fused_deblocks = False
        off = bev(dict(spatial_features=x))
    assert seen == calls[len(seen):] and all(c[0] == "conv" and c[2] is None for c in seen) and len(seen) == 3
    for k in off:
        assert torch.equal(on[k], off[k]) and on[k].stride() == off[k].stride()


def test_detector_from_points_to_boxes_with_all_switches_on():
    """mssvt.yaml with FUSED_CONVS on the three dense modules: FUSED_DEBLOCKS on top gives the boxes of the run without it,
    within the tolerance the detector tests use for box lists (tests/test_detector_cpu.py::check_against_golden)."""
    from mssvt_amd import centerpoint, config
    cfg = config.load_yaml(config.DEFAULT_CFG)
    cfg.MODEL.MAP_TO_BEV["FUSED_CONVS"] = True
    cfg.MODEL.BACKBONE_2D["FUSED_CONVS"] = True
    cfg.MODEL.BACKBONE_2D["FUSED_DEBLOCKS"] = True
    cfg.MODEL.DENSE_HEAD["FUSED_CONVS"] = True
    torch.manual_seed(0)
    det = centerpoint.build_detector(cfg).to(DEV).eval()
    assert det.backbone_2d.fused_convs and det.backbone_2d.fused_deblocks and det.dense_head.fused_convs
    with torch.no_grad():
        for h in det.dense_head.heads_list:  # random init: lift the heat map above the score threshold
            h.hm[-1].bias.fill_(0.5)
    B = 2
    pts = torch.from_numpy(synthetic.make_batch_points(40000, B, 123)).to(DEV)
    keep = bev_conv.ROUTED_UP2
    bev_conv.ROUTED_UP2 = frozenset({(256, 256)})  # the kernel, whatever the routing table holds
    try:
        with torch.no_grad():
            on, _ = det(dict(points=pts, batch_size=B))
            det.backbone_2d.fused_deblocks = False
            off, _ = det(dict(points=pts, batch_size=B))
    finally:
        bev_conv.ROUTED_UP2 = keep
    rows = lambda p: np.concatenate([p["pred_boxes"].cpu().numpy(), p["pred_labels"].cpu().numpy()[:, None].astype(np.float32)], 1)  # noqa: E731
    for p, q in zip(on, off):
        assert 0 < q["pred_boxes"].shape[0] and p["pred_boxes"].shape == q["pred_boxes"].shape
        np.testing.assert_allclose(p["pred_scores"].cpu().numpy(), q["pred_scores"].cpu().numpy(), rtol=1e-4, atol=5e-5)
        g, w = rows(p), rows(q)
        g, w = g[np.lexsort((g[:, 1], g[:, 0]))], w[np.lexsort((w[:, 1], w[:, 0]))]
        np.testing.assert_allclose(g, w, rtol=1e-4, atol=1e-4)
