"""BaseBEVBackbone and the whole CenterPoint detector in TRAINING mode with ``fused_train`` + ``fused_train_down`` on, with and
without ``fused_bn`` / ``fused_train_deblocks``: against a float64 CPU copy of the same module (the project's 1e-3 relative
parity tolerance, as tests/test_bev_deblock_train_modules_gpu.py), against the run with the new switch off and the run with
``fused_train`` alone; the stride-2 layer really runs through ``bev_down_train.DownFunction``; the switch alone is inert.

The product shapes are routed here whatever ``bev_down_train.ROUTED_DOWN_TRAIN`` and its siblings hold (the fixture sets
them): the routing rule is a question of speed, these tests are about values."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from mssvt_amd import bev_conv_train as bct, bev_deblock_train as bdt, bev_down_train as bdn, synthetic
from mssvt_amd.base_bev_backbone import BaseBEVBackbone
from mssvt_amd.config import Config
from tests.test_bev_conv_modules_gpu import randomise_batch_norms

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
PRODUCT_CONVS = frozenset({(3, 128, 128, 1, 1), (3, 128, 128, 1, 2), (3, 256, 256, 1, 1)})
PRODUCT_DEBLOCKS = frozenset({(1, 128, 256), (2, 256, 256)})
PRODUCT_DOWN = frozenset({(128, 256)})


@pytest.fixture
def down_calls(monkeypatch):
    """Routes the product shapes and records the layers that really run through ``bev_down_train.down`` and ``conv3x3``."""
    monkeypatch.setattr(bct, "ROUTED_TRAIN", PRODUCT_CONVS)
    monkeypatch.setattr(bdt, "ROUTED_DEBLOCK_TRAIN", PRODUCT_DEBLOCKS)
    monkeypatch.setattr(bdn, "ROUTED_DOWN_TRAIN", PRODUCT_DOWN)
    calls = []
    real = bdn.down

    def counted(conv, x):
        calls.append(conv)
        return real(conv, x)

    monkeypatch.setattr(bdn, "down", counted)
    return calls


def close(got, want, what):
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    assert got.shape == want.shape, what
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    assert err <= TOL * max(scale, 1e-30), (what, err, scale)


def library_calls(module):
    """Forward hooks on every convolution module: the modules called AS MODULES."""
    seen, handles = [], []
    for m in module.modules():
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            handles.append(m.register_forward_hook(lambda mod, inp, out: seen.append(mod)))
    return seen, handles


def backbone(filters, up_filters, **switches):
    torch.manual_seed(6)
    cfg = dict(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=list(filters), UPSAMPLE_STRIDES=[1, 2],
               NUM_UPSAMPLE_FILTERS=list(up_filters), FUSED_TRAIN=True, FUSED_TRAIN_DOWN=True)
    cfg.update(switches)
    bev = BaseBEVBackbone(Config.wrap(cfg), filters[0])
    return randomise_batch_norms(bev, 7).to(DEV).train()


def bev_step(bev, x0, seed_grad):
    bev.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    out = bev(dict(spatial_features=x))
    out["spatial_features_2d"].backward(seed_grad)
    return ({k: v.detach() for k, v in out.items() if k != "spatial_features"}, x.grad.clone(),
            {k: v.grad.clone() for k, v in bev.named_parameters()})


def compare(a, b, what):
    for k in a[0]:
        close(a[0][k], b[0][k], "%s %s" % (what, k))
    close(a[1], b[1], what + " input gradient")
    assert sorted(a[2]) == sorted(b[2])
    for k in a[2]:
        close(a[2][k], b[2][k], "%s d %s" % (what, k))


def test_the_yaml_key_and_the_default():
    bev = BaseBEVBackbone(Config.wrap(dict(LAYER_NUMS=[1], LAYER_STRIDES=[1], NUM_FILTERS=[32], UPSAMPLE_STRIDES=[1],
                                           NUM_UPSAMPLE_FILTERS=[64])), 32)
    assert bev.fused_train_down is False
    assert backbone([32, 64], [64, 32]).fused_train_down is True
    assert backbone([32, 64], [64, 32], FUSED_TRAIN_DOWN=False).fused_train_down is False


# the narrow widths in every combination of the other switches, on two grids; the product widths with none and with all of them
STEP_CASES = [([32, 64], [64, 32], hw, bn, de) for hw in ((12, 10), (10, 14)) for bn in (False, True) for de in (False, True)] + \
             [([128, 256], [256, 256], (12, 10), False, False), ([128, 256], [256, 256], (12, 10), True, True)]


@pytest.mark.parametrize("filters,up_filters,hw,fused_bn,deblocks", STEP_CASES)
def test_two_block_backbone_training_step(filters, up_filters, hw, fused_bn, deblocks, down_calls, monkeypatch):
    bev = backbone(filters, up_filters, FUSED_BN=fused_bn, FUSED_TRAIN_DEBLOCKS=deblocks)
    assert bev.fused_train and bev.fused_train_down and bev.fused_bn is fused_bn and bev.fused_train_deblocks is deblocks
    state = copy.deepcopy(bev.state_dict())
    H, W = hw
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(2, filters[0], H, W, generator=g).clamp_(min=0).to(DEV)
    seed_grad = torch.randn(2, sum(up_filters), H, W, generator=g).to(DEV)
    seen, handles = library_calls(bev)
    threes = []
    real3 = bct.conv3x3
    monkeypatch.setattr(bct, "conv3x3", lambda conv, x: (threes.append(conv), real3(conv, x))[1])
    on = bev_step(bev, x0, seed_grad)
    down = bev.blocks[1][1]
    stride1 = [bev.blocks[0][1], bev.blocks[0][4], bev.blocks[1][4]]
    ups = [bev.deblocks[0][0], bev.deblocks[1][0]]
    # the stride-2 layer through the Function, never through conv3x3 (whose count is what it was), never as a module
    assert [id(m) for m in down_calls] == [id(down)] and bdn.down_shape(down, 1) == tuple(filters)
    assert [id(m) for m in threes] == [id(m) for m in stride1]
    assert sorted(id(m) for m in seen) == sorted(id(m) for m in ([] if deblocks else ups))
    assert tuple(on[0]["spatial_features_2d"].shape) == (2, sum(up_filters), H, W)
    assert tuple(on[0]["spatial_features_2x"].shape) == (2, filters[1], H // 2, W // 2)
    assert set(on[0]) == {"spatial_features_1x", "spatial_features_2x", "spatial_features_2d"}
    # the new switch off: the stride-2 layer is a module again, nothing else changes
    bev.load_state_dict(state)
    bev.fused_train_down = False
    del down_calls[:], seen[:], threes[:]
    no_down = bev_step(bev, x0, seed_grad)
    assert down_calls == [] and sorted(id(m) for m in seen) == sorted(id(m) for m in [down] + ([] if deblocks else ups))
    assert [id(m) for m in threes] == [id(m) for m in stride1]
    # fused_train alone
    bev.load_state_dict(state)
    bev.fused_bn = bev.fused_train_deblocks = False
    del seen[:]
    train_only = bev_step(bev, x0, seed_grad)
    assert down_calls == [] and sorted(id(m) for m in seen) == sorted(id(m) for m in [down] + ups)
    # fused_train off: the new switch alone does nothing
    bev.load_state_dict(state)
    bev.fused_train_down, bev.fused_train = True, False
    del seen[:]
    off = bev_step(bev, x0, seed_grad)
    assert down_calls == [] and len(seen) == 6
    for h in handles:
        h.remove()
    ref = copy.deepcopy(bev)
    ref.load_state_dict(state)
    ref = ref.double().cpu().train()
    want = bev_step(ref, x0.double().cpu(), seed_grad.double().cpu())
    assert sorted(want[2]) == sorted(on[2]) == sorted(k for k, _ in bev.named_parameters())  # state-dict keys unchanged
    assert sorted(bev.state_dict()) == sorted(state)
    compare(on, want, "on vs float64")
    compare(on, no_down, "on vs fused_train_down off")
    compare(on, train_only, "on vs fused_train alone")
    compare(on, off, "on vs fused_train off")


def test_padding_one_spelling_and_no_library_convolution_for_the_layer(down_calls):
    """``Conv2d(..., stride=2, padding=1)`` without the ZeroPad2d is the same layer; under the profiler the layer's forward and
    backward record no convolution operator of the library (aten::convolution / miopen_convolution / convolution_backward),
    while the same stack with the flag off records them."""
    from torch.profiler import ProfilerActivity, profile
    torch.manual_seed(3)
    conv = nn.Conv2d(32, 64, 3, stride=2, padding=1, bias=False).to(DEV)
    paired = nn.Conv2d(32, 64, 3, stride=2, padding=0, bias=False).to(DEV)
    with torch.no_grad():
        paired.weight.copy_(conv.weight)
    x0 = torch.randn(2, 32, 9, 12, device=DEV).contiguous(memory_format=torch.channels_last)
    g = torch.randn(2, 64, 5, 6, device=DEV)

    def step(layers, fused_down):
        for m in layers:
            m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        with profile(activities=[ProfilerActivity.CPU]) as prof:
            y = bct.run_layers_train(layers, x, fused_down=fused_down)
            y.backward(g)
        torch.cuda.synchronize()
        names = {e.key for e in prof.key_averages()}
        return y.detach(), x.grad, [m for m in layers if isinstance(m, nn.Conv2d)][0].weight.grad, \
            sorted(n for n in names if "conv" in n.lower() and n.startswith("aten::"))

    a = step([conv, nn.ReLU()], True)
    b = step([nn.ZeroPad2d(1), paired, nn.ReLU()], True)
    assert [id(m) for m in down_calls] == [id(conv), id(paired)]
    assert a[3] == [] and b[3] == [], (a[3], b[3])
    for u, v in zip(a[:3], b[:3]):
        assert torch.equal(u, v)
    lib = step([conv, nn.ReLU()], False)
    assert len(down_calls) == 2 and any("convolution" in n for n in lib[3]), lib[3]
    for u, v, what in zip(a[:3], lib[:3], ("y", "dx", "dw")):
        close(u, v, what)


@pytest.mark.parametrize("why", ["eval", "no_grad", "amp", "train_off", "cpu"])
def test_the_switch_alone_is_inert(why, down_calls):
    bev = backbone([32, 64], [64, 32])
    if why == "eval":
        bev.eval()
    if why == "amp":
        bev.use_amp = True
    if why == "train_off":
        bev.fused_train = False
    if why == "cpu":
        bev = bev.cpu()
    seen, handles = library_calls(bev)
    x = torch.randn(1, 32, 6, 6, generator=torch.Generator().manual_seed(3)).to("cpu" if why == "cpu" else DEV)
    with (torch.no_grad() if why == "no_grad" else torch.enable_grad()):
        out = bev(dict(spatial_features=x.requires_grad_(why != "no_grad")))
    for h in handles:
        h.remove()
    assert down_calls == [] and len(seen) == 6 and out["spatial_features_2d"].is_contiguous()


def test_an_unrouted_stride_two_layer_stays_a_module(down_calls):
    """(64, 64) is not a covered shape, and a bias takes a covered one out: both stay modules with the switch on."""
    torch.manual_seed(8)
    bev = BaseBEVBackbone(Config.wrap(dict(LAYER_NUMS=[1, 1, 1], LAYER_STRIDES=[1, 2, 2], NUM_FILTERS=[32, 64, 64],
                                           UPSAMPLE_STRIDES=[1, 2, 4], NUM_UPSAMPLE_FILTERS=[32, 32, 32], FUSED_TRAIN=True,
                                           FUSED_TRAIN_DOWN=True)), 32)
    bev = randomise_batch_norms(bev, 9).to(DEV).train()

    def library_calls(module):  # (the Conv2d modules alone: the deblocks are modules here)
        seen, handles = [], []
        for m in module.modules():
            if isinstance(m, nn.Conv2d):
                handles.append(m.register_forward_hook(lambda mod, inp, out: seen.append(mod)))
        return seen, handles

    seen, handles = library_calls(bev)
    x = torch.randn(2, 32, 8, 8, generator=torch.Generator().manual_seed(4)).to(DEV).requires_grad_(True)
    bev(dict(spatial_features=x))["spatial_features_2d"].sum().backward()
    assert [id(m) for m in down_calls] == [id(bev.blocks[1][1])] and [id(m) for m in seen] == [id(bev.blocks[2][1])]
    bev.blocks[1][1] = nn.Conv2d(32, 64, 3, stride=2, padding=0, bias=True).to(DEV)
    seen2, handles2 = library_calls(bev)
    del down_calls[:]
    bev(dict(spatial_features=x))["spatial_features_2d"].sum().backward()
    assert down_calls == [] and sorted(id(m) for m in seen2) == sorted(id(m) for m in (bev.blocks[1][1], bev.blocks[2][1]))
    for h in handles + handles2:
        h.remove()


def test_detector_training_step_with_every_bev_switch_on(down_calls):
    """mssvt.yaml with FUSED_TRAIN + FUSED_BN on both dense modules, FUSED_TRAIN_DEBLOCKS and FUSED_TRAIN_DOWN on the backbone:
    one training step; every parameter the switch-off step gives a gradient gets a finite one, the loss is within 1e-3 relative
    of that step's.  At the sibling tests' size (tests/test_bev_deblock_train_modules_gpu.py): two detectors built and stepped
    once each, far above the few seconds of every other test here when this is the first detector step of the process."""
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
        for key in ("FUSED_TRAIN", "FUSED_BN"):
            cfg.MODEL.MAP_TO_BEV[key] = True
            cfg.MODEL.BACKBONE_2D[key] = True
        cfg.MODEL.BACKBONE_2D["FUSED_TRAIN_DEBLOCKS"] = True
        cfg.MODEL.BACKBONE_2D["FUSED_TRAIN_DOWN"] = on
        torch.manual_seed(0)
        det = centerpoint.build_detector(cfg).to(DEV).train()
        assert det.backbone_2d.fused_train_down is on and det.backbone_2d.fused_train is True
        before = len(down_calls)
        ret, _, _ = det(dict(points=pts, batch_size=B, gt_boxes=torch.from_numpy(gt).to(DEV)))
        ret["loss"].backward()
        routed = len(down_calls) - before
        assert routed == (1 if on else 0)
        assert not on or bdn.down_shape(down_calls[-1], 1) == (128, 256)
        for k, v in det.named_parameters():
            if v.grad is not None:
                assert bool(torch.isfinite(v.grad).all()), k
            if k.split(".")[0] == "backbone_2d":
                assert v.grad is not None and float(v.grad.abs().sum()) > 0, k
        with_grad[on] = sorted(k for k, v in det.named_parameters() if v.grad is not None)
        losses[on] = ret["loss"].item()
        print("detector training step, fused_train_down %s: loss %.6f" % (on, losses[on]))
        assert np.isfinite(losses[on]) and losses[on] > 0
        del det, ret
    assert with_grad[True] == with_grad[False]
    assert abs(losses[True] - losses[False]) <= 1e-3 * abs(losses[False]), losses
