"""``CenterHead`` with ``fused_convs`` on (mssvt_amd/head_conv.py, csrc/head_conv.hip): against the reference-run golden at the
tolerance the detector tests apply to the library path, against the switch-off run at product sizes and in other head
configurations, the conditions under which the switch must have no effect, the padded path without a host synchronisation,
and the whole detector from points to boxes."""
import numpy as np
import pytest
import torch

from mssvt_amd import center_head, head_conv, synthetic
from tests import head_conv_ref as ref
from tests.test_bev_conv_modules_gpu import close

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture
def stage_calls(monkeypatch):
    """The stages that really run on the kernels, in call order."""
    calls = []
    for name in ("run_shared", "run_trunk", "run_finals"):
        real = getattr(head_conv, name)

        def counted(packed, *args, _real=real):
            calls.append(packed.stage)
            return _real(packed, *args)

        monkeypatch.setattr(head_conv, name, counted)
    return calls


def routed_stages(channels_last=False):
    """The stages of ``head_conv.ROUTED`` in call order; the shared layer is taken for features that arrive channels-last, for
    NCHW features only with ``head_conv.SHARED_FROM_NCHW``."""
    return [s for s in head_conv.STAGES if s in head_conv.ROUTED and (s != "shared" or channels_last or head_conv.SHARED_FROM_NCHW)]


def features(shape, seed, channels_last=False):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed)).clamp_(min=0).to(DEV)
    return x.contiguous(memory_format=torch.channels_last) if channels_last else x


def run(head, x, on):
    head.fused_convs = on
    with torch.no_grad():
        out = head(dict(spatial_features_2d=x, batch_size=x.shape[0]))
    return head.forward_ret_dict["pred_dicts"], out


def rows(p):
    r = np.concatenate([p["pred_boxes"].cpu().numpy(), p["pred_labels"].cpu().numpy()[:, None].astype(np.float32)], 1)
    return r[np.lexsort((r[:, 1], r[:, 0]))]


def same_boxes(on, off):
    """Box lists as tests/test_detector_cpu.py::check_against_golden compares them."""
    for p, q in zip(on, off):
        assert p["pred_boxes"].shape == q["pred_boxes"].shape
        np.testing.assert_allclose(p["pred_scores"].cpu().numpy(), q["pred_scores"].cpu().numpy(), rtol=1e-4, atol=5e-5)
        np.testing.assert_allclose(rows(p), rows(q), rtol=1e-4, atol=1e-4)


def check_maps(head, on, off, B, H, W):
    assert len(on) == len(off) == len(head.heads_list)
    for sep, p, q in zip(head.heads_list, on, off):
        assert list(p) == list(q) == list(sep.sep_head_dict)  # keys in sep_head_dict order
        for k in q:
            assert tuple(p[k].shape) == (B, sep.sep_head_dict[k]["out_channels"], H, W) and p[k].is_contiguous()
            assert p[k].dtype == torch.float32
            close(p[k], q[k])


def test_golden_head_with_the_switch_on_matches_the_reference_run(golden_dir, stage_calls):
    """det_bev_head.npz (64 -> 32, five branches): all five raw maps and the box lists, at the tolerance of
    tests/test_detector_gpu.py::test_center_head_with_the_hip_nms_matches_the_reference_run."""
    from tests.test_detector_cpu import build_from_golden, check_against_golden
    d, bev, head = build_from_golden(golden_dir)
    assert head.fused_convs is False
    head.fused_convs = True
    check_against_golden(d, bev.to(DEV), head.to(DEV), dev=DEV, tol=5e-5)
    assert stage_calls == routed_stages()  # (the golden's features are NCHW)
    # and on the same features channels-last, as the backbone hands them over with its own switch on
    del stage_calls[:]
    x = torch.from_numpy(d["spatial_features_2d"]).to(DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        head(dict(spatial_features_2d=x, batch_size=int(d["batch_size"])))
    assert stage_calls == routed_stages(True)
    raw = head.forward_ret_dict["pred_dicts"][0]
    for k in ("hm", "center", "center_z", "dim", "rot"):
        np.testing.assert_allclose(raw[k].cpu().numpy(), d["raw." + k], rtol=1e-4, atol=5e-5)


@pytest.mark.parametrize("channels_last", [False, True])
def test_product_channel_counts_on_a_40_grid_on_versus_off(channels_last, stage_calls):
    """512 -> 64 with five branches as in mssvt.yaml, B = 2, random BatchNorm statistics; the features arrive NCHW (backbone
    switch off) or channels-last (backbone switch on)."""
    head = ref.build_head(512, seed=3, shared=64, fused=True).to(DEV)
    assert head.fused_convs is True and head_conv.supported(head)
    x = features((2, 512, 40, 40), seed=1, channels_last=channels_last)
    on, out_on = run(head, x, True)
    assert stage_calls == routed_stages(channels_last)
    off, out_off = run(head, x, False)
    assert stage_calls == routed_stages(channels_last)
    check_maps(head, on, off, 2, 40, 40)
    assert sum(p["pred_boxes"].shape[0] for p in out_off["final_box_dicts"]) > 0
    same_boxes(out_on["final_box_dicts"], out_off["final_box_dicts"])


def test_nchw_features_are_converted_once_where_the_shared_layer_is_routed_for_them(stage_calls, monkeypatch):
    """``SHARED_FROM_NCHW`` on (the setting for a device where the kernel wins behind the conversion too): NCHW features are
    made channels-last once and all routed stages run on the kernels; the caller's tensor is left as it was."""
    monkeypatch.setattr(head_conv, "SHARED_FROM_NCHW", True)
    head = ref.build_head(256, seed=4, shared=64).to(DEV)
    x = features((2, 256, 13, 15), seed=6)
    keep = x.clone()
    on, _ = run(head, x, True)
    assert stage_calls == routed_stages(True) and torch.equal(x, keep) and x.is_contiguous()
    off, _ = run(head, x, False)
    check_maps(head, on, off, 2, 13, 15)


@pytest.mark.parametrize("why", ["train", "autograd", "amp", "autocast", "uncovered"])
def test_switch_has_no_effect(why, stage_calls):
    """Train mode, autograd, AMP (the module's flag or an autocast region) and a head the kernels do not cover (one branch
    with num_conv 1): today's path runs, no stage reaches the kernels and the maps are the switch-off run's bit for bit.
    Identity can show something only where the library itself repeats its bits from call to call: asserted first."""
    kw = dict(num_conv={"dim": 1}) if why == "uncovered" else {}
    head = ref.build_head(64, seed=5, shared=32, score_thresh=0.9999, **kw).to(DEV)  # (no peak passes: the maps are the subject)
    assert head_conv.supported(head) == (why != "uncovered")
    x = features((2, 64, 24, 24), seed=8)
    if why == "train":
        head.train()
    if why == "amp":
        head.use_amp = True

    def forward(on):
        head.fused_convs = on
        ctx = torch.enable_grad() if why in ("train", "autograd") else torch.no_grad()
        with ctx, torch.autocast("cuda", enabled=why == "autocast"):
            head(dict(spatial_features_2d=x, batch_size=2, gt_boxes=torch.zeros(2, 1, 8, device=DEV)))
        return [{k: v.detach() for k, v in pd.items()} for pd in head.forward_ret_dict["pred_dicts"]]

    forward(False)  # the library settles on its algorithms for these shapes during a first call
    off = forward(False)
    off2 = forward(False)
    on = forward(True)
    assert stage_calls == []
    for p, q, r in zip(on, off, off2):
        for k in q:
            assert torch.equal(q[k], r[k]), "the library path does not repeat itself: " + k
            assert torch.equal(p[k], q[k]) and p[k].stride() == q[k].stride() and p[k].dtype == q[k].dtype


@pytest.mark.parametrize("config", ["two_heads", "vel"])
def test_other_head_configurations_on_versus_off(config, stage_calls):
    kw = dict(heads=[["Vehicle"], ["Pedestrian", "Cyclist"]]) if config == "two_heads" else dict(vel=True)
    head = ref.build_head(64, seed=7, shared=32, **kw).to(DEV)
    nb = sum(len(sep.sep_head_dict) for sep in head.heads_list)
    assert nb == (10 if config == "two_heads" else 6) and head_conv.supported(head)
    x = features((3, 64, 17, 19), seed=2)
    on, out_on = run(head, x, True)
    assert stage_calls == routed_stages()
    off, out_off = run(head, x, False)
    check_maps(head, on, off, 3, 17, 19)
    same_boxes(out_on["final_box_dicts"], out_off["final_box_dicts"])
    assert all(p["pred_boxes"].shape[1] == (9 if config == "vel" else 7) for p in out_on["final_box_dicts"])


def test_padded_path_with_the_switch_on_never_synchronises_the_host(stage_calls):
    head = ref.build_head(64, seed=9, shared=32).to(DEV)
    head.padded_predictions = True
    x = features((2, 64, 30, 30), seed=4, channels_last=True)
    _, off = run(head, x, False)
    _, warm = run(head, x, True)  # packs the weights; the library has settled too
    torch.cuda.synchronize()
    del stage_calls[:]
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
            _, on = run(head, x, True)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    assert stage_calls == routed_stages(True)
    got, want = on["final_box_padded"], off["final_box_padded"]
    assert int(want["num"].sum()) > 0 and torch.equal(got["num"], want["num"])
    same_boxes(center_head.unpad(got), center_head.unpad(want))
    for k in got:
        assert torch.equal(got[k], warm["final_box_padded"][k])


def test_detector_from_points_to_boxes_with_all_three_switches_on():
    """mssvt.yaml with FUSED_CONVS on map_to_bev, backbone_2d and dense_head: the boxes of the all-off run, as in
    tests/test_bev_conv_modules_gpu.py::test_detector_from_points_to_boxes_with_the_switch_on."""
    from mssvt_amd import centerpoint, config
    cfg = config.load_yaml(config.DEFAULT_CFG)
    cfg.MODEL.MAP_TO_BEV["FUSED_CONVS"] = True
    cfg.MODEL.BACKBONE_2D["FUSED_CONVS"] = True
    cfg.MODEL.DENSE_HEAD["FUSED_CONVS"] = True
    torch.manual_seed(0)
    det = centerpoint.build_detector(cfg).to(DEV).eval()
    assert det.map_to_bev_module.fused_convs and det.backbone_2d.fused_convs and det.dense_head.fused_convs
    assert head_conv.supported(det.dense_head)
    with torch.no_grad():
        for h in det.dense_head.heads_list:  # random init: lift the heat map above the score threshold
            h.hm[-1].bias.fill_(0.5)
    B = 2
    pts = torch.from_numpy(synthetic.make_batch_points(40000, B, 123)).to(DEV)
    with torch.no_grad():
        on, _ = det(dict(points=pts, batch_size=B))
        det.map_to_bev_module.fused_convs = det.backbone_2d.fused_convs = det.dense_head.fused_convs = False
        off, _ = det(dict(points=pts, batch_size=B))
    assert all(q["pred_boxes"].shape[0] > 0 for q in off)
    same_boxes(on, off)
