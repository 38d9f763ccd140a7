"""HeightCompression / BaseBEVBackbone / the whole CenterPoint detector in TRAINING mode with ``fused_train`` and ``fused_bn``
on: every routed BatchNorm + ReLU pair through ``bn_train.bn_relu`` (csrc/bn_train.hip), against a float64 CPU copy of the same
module and against the ``fused_train``-only run (the project's 1e-3 relative parity tolerance), bit-identical over two
identical steps, and without effect wherever ``fused_train`` has none.

The product widths are routed here whatever ``bn_train.ROUTED_BN`` holds (the fixture sets it): the routing rule is a question
of speed, these tests are about values."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from mssvt_amd import bev_conv, bev_conv_train as bct, bn_train, synthetic
from tests.test_bev_conv_modules_gpu import sparse_grid
from tests.test_bev_conv_train_modules_gpu import PRODUCT, backbone, bev_step, close, hc_step, height_compression

pytestmark = pytest.mark.gpu
DEV = "cuda"
BUFFERS = ("running_mean", "running_var", "num_batches_tracked")


@pytest.fixture
def bn_calls(monkeypatch):
    """Routes the product convolutions and the product BatchNorm widths; counts the layers that really run through bn_relu."""
    monkeypatch.setattr(bct, "ROUTED_TRAIN", PRODUCT)
    monkeypatch.setattr(bn_train, "ROUTED_BN", frozenset({128, 256}))
    calls = []
    real = bn_train.bn_relu

    def counted(bn, x, relu):
        calls.append((bn, relu))
        return real(bn, x, relu)

    monkeypatch.setattr(bn_train, "bn_relu", counted)
    return calls


def module_calls(module):
    """Forward hooks on every BatchNorm module: those called AS MODULES."""
    seen, handles = [], []
    for m in module.modules():
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            handles.append(m.register_forward_hook(lambda mod, inp, out: seen.append(mod)))
    return seen, handles


def buffers(module):
    return {k: v.clone() for k, v in module.state_dict().items() if k.rsplit(".", 1)[-1] in BUFFERS}


def close_buffers(got, want, what):
    assert sorted(got) == sorted(want) and len(got) > 0
    for k in got:
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(want[k]) == 1, (what, k)
        else:
            close(got[k], want[k], "%s %s" % (what, k))


def test_height_compression_training_step(bn_calls):
    hc = height_compression()
    hc.fused_bn = True
    state = copy.deepcopy(hc.state_dict())
    sp = sparse_grid([13, 11, 1], 2, 128, seed=7)  # X = 13, Y = 11: (2, 128, 11, 13)
    feats = sp.features.detach().clone()
    seed_grad = torch.randn(2, 128, 11, 13, generator=torch.Generator().manual_seed(1)).to(DEV)
    seen, handles = module_calls(hc)
    on, on_df, on_g = hc_step(hc, sp, feats, seed_grad)
    on_b = buffers(hc)
    assert [relu for _, relu in bn_calls] == [True, True, True] and seen == [] and bev_conv.is_channels_last(on)
    assert [bn for bn, _ in bn_calls] == [hc.compress_layers[1], hc.compress_layers[4], hc.compress_layers[7]]
    # bit-identical over two identical steps
    hc.load_state_dict(state)
    on2, on2_df, on2_g = hc_step(hc, sp, feats, seed_grad)
    on2_b = buffers(hc)
    assert torch.equal(on, on2) and torch.equal(on_df, on2_df) and all(torch.equal(on_g[k], on2_g[k]) for k in on_g)
    assert all(torch.equal(on_b[k], on2_b[k]) for k in on_b)
    # the fused_train-only run: every BatchNorm a module call
    hc.load_state_dict(state)
    hc.fused_bn = False
    off, off_df, off_g = hc_step(hc, sp, feats, seed_grad)
    off_b = buffers(hc)
    assert len(bn_calls) == 6 and len(seen) == 3
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
    want_b = {"compress_layers." + k: v for k, v in buffers(layers).items()}
    for got, got_df, got_g, got_b, what in ((on, on_df, on_g, on_b, "on"), (off, off_df, off_g, off_b, "off")):
        close(got, want, what + " output")
        close(got_df, want_df, what + " feature gradient")
        for k, v in layers.named_parameters():
            close(got_g["compress_layers." + k], v.grad, "%s d %s" % (what, k))
        close_buffers(got_b, want_b, what)
    close(on, off, "on vs off output")
    close(on_df, off_df, "on vs off feature gradient")
    for k in on_g:
        close(on_g[k], off_g[k], "on vs off d " + k)
    close_buffers(on_b, off_b, "on vs off")


def test_two_block_backbone_training_step(bn_calls):
    bev = backbone()
    bev.fused_bn = True
    state = copy.deepcopy(bev.state_dict())
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(2, 128, 12, 10, generator=g).clamp_(min=0).to(DEV)
    seed_grad = torch.randn(2, 512, 12, 10, generator=g).to(DEV)
    bev_step(bev, x0, seed_grad)  # (the library settles on its algorithms for these shapes during a first call)
    bev.load_state_dict(state)
    bn_calls.clear()
    seen, handles = module_calls(bev)
    on, on_dx, on_g = bev_step(bev, x0, seed_grad)
    on_b = buffers(bev)
    all_bn = [m for m in bev.modules() if isinstance(m, nn.BatchNorm2d)]
    assert len(all_bn) == 6 and sorted(id(bn) for bn, _ in bn_calls) == sorted(id(m) for m in all_bn)
    assert all(relu for _, relu in bn_calls) and seen == []  # none called as a module
    assert tuple(on["spatial_features_2d"].shape) == (2, 512, 12, 10)
    for h in handles:
        h.remove()
    bev.load_state_dict(state)
    on2, on2_dx, on2_g = bev_step(bev, x0, seed_grad)
    # what only the kernels determine (block 0: convolutions, BatchNorm, ReLU) repeats its bits without condition
    assert torch.equal(on["spatial_features_1x"], on2["spatial_features_1x"])
    bev.load_state_dict(state)
    bev.fused_bn = False
    off, off_dx, off_g = bev_step(bev, x0, seed_grad)
    off_b = buffers(bev)
    assert len(bn_calls) == 12
    ref = copy.deepcopy(bev)
    ref.load_state_dict(state)
    ref = ref.double().cpu().train()
    want, want_dx, want_g = bev_step(ref, x0.double().cpu(), seed_grad.double().cpu())
    want_b = buffers(ref)
    assert sorted(want_g) == sorted(on_g) == sorted(k for k, _ in bev.named_parameters())  # state-dict keys unchanged
    assert sorted(bev.state_dict()) == sorted(state)
    for got, got_dx, got_g, got_b, what in ((on, on_dx, on_g, on_b, "on"), (off, off_dx, off_g, off_b, "off")):
        for k in want:
            close(got[k], want[k], "%s %s" % (what, k))
        close(got_dx, want_dx, what + " input gradient")
        for k in want_g:
            close(got_g[k], want_g[k], "%s d %s" % (what, k))
        close_buffers(got_b, want_b, what)
    for k in on:
        close(on[k], off[k], "on vs off " + k)
    close(on_dx, off_dx, "on vs off input gradient")
    for k in on_g:
        close(on_g[k], off_g[k], "on vs off d " + k)
    close_buffers(on_b, off_b, "on vs off")


@pytest.mark.parametrize("why", ["fused_train_off", "eval", "no_grad", "amp", "sync_batchnorm"])
def test_switch_has_no_effect_outside_its_conditions(why, bn_calls):
    bev = backbone()
    bev.fused_bn = True
    if why == "fused_train_off":
        bev.fused_train = False
    if why == "eval":
        bev.eval()
    if why == "amp":
        bev.use_amp = True
    if why == "sync_batchnorm":
        bev = nn.SyncBatchNorm.convert_sync_batchnorm(bev)
        assert bev.fused_bn and bev.fused_train and not any(type(m) is nn.BatchNorm2d for m in bev.modules())
        bev.eval()  # (a SyncBatchNorm in training mode needs a process group; the routing question is settled before that)
        assert not any(bn_train.bn_supported(m) or bn_train.bn_routed(m) for m in bev.modules())
        layers = list(bev.blocks[0])
        assert isinstance(layers[2], nn.SyncBatchNorm)
        seen, handles = module_calls(bev)
        x = torch.randn(1, 128, 6, 6, generator=torch.Generator().manual_seed(3)).to(DEV).contiguous(memory_format=torch.channels_last)
        bct.run_layers_train(layers, x.requires_grad_(True), fused_bn=True)
        assert bn_calls == [] and len(seen) == 2  # both stayed torch modules
        for h in handles:
            h.remove()
        return
    x = torch.randn(1, 128, 6, 6, generator=torch.Generator().manual_seed(3)).to(DEV)
    with (torch.no_grad() if why == "no_grad" else torch.enable_grad()):
        out = bev(dict(spatial_features=x.requires_grad_(why != "no_grad")))
    assert bn_calls == [] and out["spatial_features_2d"].is_contiguous()


@pytest.mark.parametrize("why", ["momentum_none", "affine_false", "no_running_stats"])
def test_an_uncovered_batch_norm_stays_a_module(why, bn_calls):
    bev = backbone()
    bev.fused_bn = True
    odd = dict(momentum_none=nn.BatchNorm2d(128, eps=1e-3, momentum=None), affine_false=nn.BatchNorm2d(128, eps=1e-3, affine=False),
               no_running_stats=nn.BatchNorm2d(128, eps=1e-3, track_running_stats=False))[why].to(DEV).train()
    bev.blocks[0][2] = odd
    assert not bn_train.bn_supported(odd) and not bn_train.bn_routed(odd)
    seen, handles = module_calls(bev)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 128, 6, 6, generator=g).to(DEV).requires_grad_(True)
    out = bev(dict(spatial_features=x))["spatial_features_2d"]
    out.sum().backward()
    assert seen == [odd] and len(bn_calls) == 5 and odd not in [bn for bn, _ in bn_calls]
    assert bool(torch.isfinite(x.grad).all())
    for h in handles:
        h.remove()


def test_a_routed_batch_norm_without_a_relu_behind_it(bn_calls):
    torch.manual_seed(8)
    bn = nn.BatchNorm2d(128, eps=1e-3, momentum=0.01).to(DEV).train()
    layers = [bn, nn.Conv2d(128, 128, 1, bias=False).to(DEV), nn.ReLU()]
    x = torch.randn(2, 128, 5, 7, device=DEV).contiguous(memory_format=torch.channels_last)
    ref = copy.deepcopy(bn)
    got = bct.run_layers_train(layers, x.clone().requires_grad_(True), fused_bn=True)
    assert bn_calls == [(bn, False)]
    want = layers[2](layers[1](ref(x)))
    close(got, want, "BatchNorm without ReLU")
    assert bool((got >= 0).all()) and bool((bn_train.bn_relu(bn, x, False) < 0).any())


def test_without_the_keyword_nothing_is_routed(bn_calls):
    """``run_layers_train(layers, x)`` and ``fused_train`` alone keep today's path: no BatchNorm leaves the module path."""
    bev = backbone()
    assert bev.fused_bn is False and bev.fused_train is True
    seen, handles = module_calls(bev)
    x = torch.randn(2, 128, 6, 6, generator=torch.Generator().manual_seed(3)).to(DEV)
    bev(dict(spatial_features=x.requires_grad_(True)))
    assert bn_calls == [] and len(seen) == 6
    seen.clear()
    xl = x.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    bct.run_layers_train(bev.blocks[0], xl)
    assert bn_calls == [] and len(seen) == 2
    bct.run_layers_train(bev.blocks[0], xl, fused_bn=True)
    assert len(bn_calls) == 2 and len(seen) == 2
    for h in handles:
        h.remove()


def test_yaml_key_and_default():
    from mssvt_amd.base_bev_backbone import BaseBEVBackbone
    from mssvt_amd.config import Config
    from mssvt_amd.height_compression import HeightCompression
    for flag in (True, False, None):
        extra = {} if flag is None else dict(FUSED_BN=flag)
        hc = HeightCompression(Config.wrap(dict(NUM_BEV_FEATURES=32, COMPRESS_LAYER_NUMS=1, **extra)))
        bev = BaseBEVBackbone(Config.wrap(dict(LAYER_NUMS=[1], LAYER_STRIDES=[1], NUM_FILTERS=[32], UPSAMPLE_STRIDES=[1],
                                               NUM_UPSAMPLE_FILTERS=[32], **extra)), 32)
        assert hc.fused_bn is bool(flag) and bev.fused_bn is bool(flag)


def test_detector_training_step_with_the_switches_on(bn_calls):
    """mssvt.yaml with FUSED_TRAIN + FUSED_BN on both dense modules: one training step; every parameter the switch-off step
    gives a gradient gets a finite one, the loss is within 1e-3 relative of the switch-off step's.  (The same two detector
    steps as tests/test_bev_conv_train_modules_gpu.py: behind it in the suite this takes seconds; alone, the library's first
    search for its convolution algorithms at the 470 x 470 grid takes two minutes.)"""
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
    losses, with_grad = {}, {}
    for on in (True, False):
        cfg = config.load_yaml(config.DEFAULT_CFG)
        for node in (cfg.MODEL.MAP_TO_BEV, cfg.MODEL.BACKBONE_2D):
            node["FUSED_TRAIN"] = on
            node["FUSED_BN"] = on
        torch.manual_seed(0)
        det = centerpoint.build_detector(cfg).to(DEV).train()
        assert det.map_to_bev_module.fused_bn is on and det.backbone_2d.fused_bn is on
        before = len(bn_calls)
        ret, _, _ = det(dict(points=pts, batch_size=B, gt_boxes=torch.from_numpy(gt).to(DEV)))
        ret["loss"].backward()
        bns = [m for part in (det.map_to_bev_module, det.backbone_2d) for m in part.modules() if isinstance(m, nn.BatchNorm2d)]
        assert len(bns) == 17 and all(bn_train.bn_routed(m) for m in bns)
        assert len(bn_calls) - before == (17 if on else 0)
        assert all(int(m.num_batches_tracked) == 1 for m in bns)
        for k, v in det.named_parameters():
            if v.grad is not None:
                assert bool(torch.isfinite(v.grad).all()), k
            if k.split(".")[0] in ("map_to_bev_module", "backbone_2d"):
                assert v.grad is not None and float(v.grad.abs().sum()) > 0, k
        with_grad[on] = sorted(k for k, v in det.named_parameters() if v.grad is not None)
        losses[on] = ret["loss"].item()
        print("detector training step, fused_train + fused_bn %s: loss %.6f" % (on, losses[on]))
        assert np.isfinite(losses[on]) and losses[on] > 0
        del det, ret
    assert with_grad[True] == with_grad[False]
    assert abs(losses[True] - losses[False]) <= 1e-3 * abs(losses[False]), losses
