"""HeightCompression / BaseBEVBackbone / the whole CenterPoint detector in TRAINING mode with ``fused_train`` on: against a
float64 CPU copy of the same module (the project's 1e-3 relative parity tolerance), against the switch-off run, bit-identical
over two identical steps, and the layers the kernels do not cover on the library path.

The product channel shapes are routed here whatever ``bev_conv_train.ROUTED_TRAIN`` holds (the fixture sets it): the routing
rule is a question of speed, these tests are about values."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from mssvt_amd import bev_conv, bev_conv_train as bct, synthetic
from mssvt_amd.base_bev_backbone import BaseBEVBackbone
from mssvt_amd.config import Config
from mssvt_amd.height_compression import HeightCompression
from tests.test_bev_conv_modules_gpu import randomise_batch_norms, sparse_grid

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRODUCT = frozenset({(3, 128, 128, 1, 1), (3, 128, 128, 1, 2), (3, 256, 256, 1, 1)})
TOL = 1e-3


@pytest.fixture
def function_calls(monkeypatch):
    """Routes the product shapes and counts the convolutions that really run through the Function."""
    monkeypatch.setattr(bct, "ROUTED_TRAIN", PRODUCT)
    calls = []
    real = bct.conv3x3

    def counted(conv, x):
        calls.append(conv)
        return real(conv, x)

    monkeypatch.setattr(bct, "conv3x3", counted)
    return calls


def close(got, want, what):
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    assert got.shape == want.shape, what
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    assert err <= TOL * max(scale, 1e-30), (what, err, scale)


def library_calls(module):
    """Forward hooks on every convolution module: (module, grad_fn name of its output) of those called AS MODULES."""
    seen, handles = [], []
    for m in module.modules():
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            handles.append(m.register_forward_hook(lambda mod, inp, out: seen.append((mod, type(out.grad_fn).__name__))))
    return seen, handles


def grads(module):
    return {k: v.grad.clone() for k, v in module.named_parameters()}


def height_compression():
    torch.manual_seed(4)
    hc = HeightCompression(Config.wrap(dict(NUM_BEV_FEATURES=128, COMPRESS_LAYER_NUMS=3, LAYER_STRIDES=[1, 1, 1],
                                            LAYER_DIALATIONS=[1, 1, 2], LAYER_PADDINGS=[1, 1, 2], FUSED_TRAIN=True)))
    assert hc.fused_train is True and hc.fused_convs is False  # the yaml key
    return randomise_batch_norms(hc, 5).to(DEV).train()


def backbone():
    torch.manual_seed(6)
    bev = BaseBEVBackbone(Config.wrap(dict(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=[128, 256],
                                           UPSAMPLE_STRIDES=[1, 2], NUM_UPSAMPLE_FILTERS=[256, 256], FUSED_TRAIN=True)), 128)
    assert bev.fused_train is True and bev.fused_convs is False
    return randomise_batch_norms(bev, 7).to(DEV).train()


def hc_step(hc, sp, feats, seed_grad):
    """One training step of HeightCompression on sparse features `feats` (a fresh leaf): output, feature gradient, parameter gradients."""
    hc.zero_grad(set_to_none=True)
    f = feats.clone().requires_grad_(True)
    sp.features = f
    out = hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1))["spatial_features"]
    out.backward(seed_grad)
    return out.detach(), f.grad.clone(), grads(hc)


def test_height_compression_training_step(function_calls):
    hc = height_compression()
    state = copy.deepcopy(hc.state_dict())
    sp = sparse_grid([13, 11, 1], 2, 128, seed=7)  # X = 13, Y = 11: (2, 128, 11, 13)
    feats = sp.features.detach().clone()
    seed_grad = torch.randn(2, 128, 11, 13, generator=torch.Generator().manual_seed(1)).to(DEV)
    seen, handles = library_calls(hc)
    on, on_df, on_g = hc_step(hc, sp, feats, seed_grad)
    assert len(function_calls) == 3 and seen == [] and bev_conv.is_channels_last(on)  # all three layers on the kernels
    # bit-identical over two identical steps
    hc.load_state_dict(state)
    on2, on2_df, on2_g = hc_step(hc, sp, feats, seed_grad)
    assert torch.equal(on, on2) and torch.equal(on_df, on2_df) and all(torch.equal(on_g[k], on2_g[k]) for k in on_g)
    # the switch-off run: every convolution a module call on the library path
    hc.load_state_dict(state)
    hc.fused_train = False
    off, off_df, off_g = hc_step(hc, sp, feats, seed_grad)
    assert len(function_calls) == 6 and len(seen) == 3 and all("Convolution" in name for _, name in seen)
    for h in handles:
        h.remove()
    # the float64 CPU copy, on the dense grid the GPU module saw
    sp.features = feats
    dense = sp.dense()[:, :, 0].detach().double().cpu().requires_grad_(True)
    ref = copy.deepcopy(hc)
    ref.load_state_dict(state)
    layers = nn.Sequential(*ref.compress_layers).double().cpu().train()
    want = layers(dense)
    want.backward(seed_grad.double().cpu())
    idx = sp.indices.long().cpu()
    want_df = dense.grad[idx[:, 0], :, idx[:, 2], idx[:, 3]]
    for got, got_df, got_g, what in ((on, on_df, on_g, "on"), (off, off_df, off_g, "off")):
        close(got, want, what + " output")
        close(got_df, want_df, what + " feature gradient")
        for k, v in layers.named_parameters():
            close(got_g["compress_layers." + k], v.grad, "%s d %s" % (what, k))
    close(on, off, "on vs off output")
    close(on_df, off_df, "on vs off feature gradient")
    for k in on_g:
        close(on_g[k], off_g[k], "on vs off d " + k)


def bev_step(bev, x0, seed_grad):
    bev.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    out = bev(dict(spatial_features=x))
    out["spatial_features_2d"].backward(seed_grad)
    return {k: v.detach() for k, v in out.items() if k != "spatial_features"}, x.grad.clone(), grads(bev)


def test_two_block_backbone_training_step(function_calls):
    bev = backbone()
    state = copy.deepcopy(bev.state_dict())
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(2, 128, 12, 10, generator=g).clamp_(min=0).to(DEV)
    seed_grad = torch.randn(2, 512, 12, 10, generator=g).to(DEV)
    bev_step(bev, x0, seed_grad)  # (the library settles on its algorithms for these shapes during a first call)
    bev.load_state_dict(state)
    function_calls.clear()
    seen, handles = library_calls(bev)
    on, on_dx, on_g = bev_step(bev, x0, seed_grad)
    # the two 128 -> 128 layers and the 256 -> 256 layer on the kernels; the stride-2 layer and both deblocks on the library
    assert [tuple(c.weight.shape[:2]) for c in function_calls] == [(128, 128), (128, 128), (256, 256)]
    want_lib = [bev.blocks[1][1], bev.deblocks[0][0], bev.deblocks[1][0]]
    assert sorted(id(m) for m, _ in seen) == sorted(id(m) for m in want_lib)
    assert all("Convolution" in name for _, name in seen), seen
    assert not any(bct.train_supported(m) for m in want_lib)
    assert tuple(on["spatial_features_2d"].shape) == (2, 512, 12, 10) and set(on) == {"spatial_features_1x", "spatial_features_2x", "spatial_features_2d"}
    for h in handles:
        h.remove()
    bev.load_state_dict(state)
    on2, on2_dx, on2_g = bev_step(bev, x0, seed_grad)
    # bit-identical over two identical steps: what only the kernels, BatchNorm and ReLU determine (block 0) without condition ...
    assert torch.equal(on["spatial_features_1x"], on2["spatial_features_1x"])
    bev.load_state_dict(state)
    bev.fused_train = False
    off, off_dx, off_g = bev_step(bev, x0, seed_grad)
    assert len(function_calls) == 6
    bev.load_state_dict(state)
    off2, off2_dx, off2_g = bev_step(bev, x0, seed_grad)
    # ... and everything else -- it passes through the library's stride-2 layer and deblocks, forward or backward -- where the
    # library itself repeats its bits from step to step at these shapes (its backward kernels may add with atomics)
    library_repeats = all(torch.equal(off[k], off2[k]) for k in off) and torch.equal(off_dx, off2_dx) \
        and all(torch.equal(off_g[k], off2_g[k]) for k in off_g)
    print("the library path repeats its bits over two identical steps: %s" % library_repeats)
    if library_repeats:
        assert all(torch.equal(on[k], on2[k]) for k in on) and torch.equal(on_dx, on2_dx)
        assert all(torch.equal(on_g[k], on2_g[k]) for k in on_g)
    ref = copy.deepcopy(bev)
    ref.load_state_dict(state)
    ref = ref.double().cpu().train()
    want, want_dx, want_g = bev_step(ref, x0.double().cpu(), seed_grad.double().cpu())
    assert sorted(want_g) == sorted(on_g) == sorted(k for k, _ in bev.named_parameters())  # state-dict keys unchanged
    for got, got_dx, got_g, what in ((on, on_dx, on_g, "on"), (off, off_dx, off_g, "off")):
        for k in want:
            close(got[k], want[k], "%s %s" % (what, k))
        close(got_dx, want_dx, what + " input gradient")
        for k in want_g:
            close(got_g[k], want_g[k], "%s d %s" % (what, k))
    for k in on:
        close(on[k], off[k], "on vs off " + k)
    close(on_dx, off_dx, "on vs off input gradient")
    for k in on_g:
        close(on_g[k], off_g[k], "on vs off d " + k)


@pytest.mark.parametrize("why", ["eval", "no_grad", "amp", "off"])
def test_switch_has_no_effect_outside_its_conditions(why, function_calls):
    bev = backbone()
    if why == "eval":
        bev.eval()
    if why == "amp":
        bev.use_amp = True
    if why == "off":
        bev.fused_train = False
    x = torch.randn(1, 128, 6, 6, generator=torch.Generator().manual_seed(3)).to(DEV)
    with (torch.no_grad() if why == "no_grad" else torch.enable_grad()):
        out = bev(dict(spatial_features=x.requires_grad_(why != "no_grad")))
    assert function_calls == [] and out["spatial_features_2d"].is_contiguous()


def test_detector_training_step_with_the_switches_on(function_calls):
    """mssvt.yaml with FUSED_TRAIN on both dense modules: one training step; every parameter the switch-off step gives a
    gradient gets a finite one, the loss is within 1e-3 relative of the switch-off step's."""
    from mssvt_amd import centerpoint, config
    B = 2
    pts = torch.from_numpy(synthetic.make_batch_points(20000, B, 77)).to(DEV)
    rng = np.random.default_rng(3)
    gt = np.zeros((B, 10, 8), np.float32)
    for b in range(B):
        n = 8 - 2 * b
        gt[b, :n, 0:2] = rng.uniform(-40, 40, (n, 2))
        gt[b, :n, 2] = rng.uniform(-1, 1, n)
        gt[b, :n, 3:6] = rng.uniform([1.5, 0.8, 1.0], [5.0, 2.5, 2.0], (n, 3))
        gt[b, :n, 6] = rng.uniform(-3.1, 3.1, n)
        gt[b, :n, 7] = rng.integers(1, 4, n)
    import time
    losses, with_grad = {}, {}
    for on in (True, False):
        t0 = time.time()
        cfg = config.load_yaml(config.DEFAULT_CFG)
        cfg.MODEL.MAP_TO_BEV["FUSED_TRAIN"] = on
        cfg.MODEL.BACKBONE_2D["FUSED_TRAIN"] = on
        torch.manual_seed(0)
        det = centerpoint.build_detector(cfg).to(DEV).train()
        assert det.map_to_bev_module.fused_train is on and det.backbone_2d.fused_train is on
        before = len(function_calls)
        ret, _, _ = det(dict(points=pts, batch_size=B, gt_boxes=torch.from_numpy(gt).to(DEV)))
        ret["loss"].backward()
        routed = len(function_calls) - before
        convs = [m for part in (det.map_to_bev_module, det.backbone_2d) for m in part.modules() if isinstance(m, nn.Conv2d)]
        assert routed == (sum(bct.train_routed(m) or bct.train_routed(m, 1) for m in convs) if on else 0)
        assert not on or routed >= 14
        for k, v in det.named_parameters():
            if v.grad is not None:
                assert bool(torch.isfinite(v.grad).all()), k
            if k.split(".")[0] in ("map_to_bev_module", "backbone_2d"):
                assert v.grad is not None and float(v.grad.abs().sum()) > 0, k
        with_grad[on] = sorted(k for k, v in det.named_parameters() if v.grad is not None)
        losses[on] = ret["loss"].item()
        print("detector training step, fused_train %s: loss %.6f, %.1f s" % (on, losses[on], time.time() - t0))
        assert np.isfinite(losses[on]) and losses[on] > 0
        del det, ret
    assert with_grad[True] == with_grad[False]
    assert abs(losses[True] - losses[False]) <= 1e-3 * abs(losses[False]), losses
