"""BaseBEVBackbone and the whole CenterPoint detector in TRAINING mode with ``fused_train`` + ``fused_train_deblocks`` on:
against a float64 CPU copy of the same module (the project's 1e-3 relative parity tolerance), against the run with the new
switch off and the run with ``fused_train`` off; the switch alone is inert; unsupported deblocks stay modules.

The product shapes are routed here whatever ``bev_deblock_train.ROUTED_DEBLOCK_TRAIN`` and ``bev_conv_train.ROUTED_TRAIN`` hold
(the fixture sets them): the routing rule is a question of speed, these tests are about values."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from mssvt_amd import bev_conv_train as bct, bev_deblock_train as bdt, synthetic
from mssvt_amd.base_bev_backbone import BaseBEVBackbone
from mssvt_amd.config import Config
from tests.test_bev_conv_modules_gpu import randomise_batch_norms

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
PRODUCT_CONVS = frozenset({(3, 128, 128, 1, 1), (3, 128, 128, 1, 2), (3, 256, 256, 1, 1)})
PRODUCT_DEBLOCKS = frozenset({(1, 128, 256), (2, 256, 256)})


@pytest.fixture
def deblock_calls(monkeypatch):
    """Routes the product shapes and records the deblocks that really run through the Function."""
    monkeypatch.setattr(bct, "ROUTED_TRAIN", PRODUCT_CONVS)
    monkeypatch.setattr(bdt, "ROUTED_DEBLOCK_TRAIN", PRODUCT_DEBLOCKS)
    calls = []
    real = bdt.deblock

    def counted(conv, x):
        calls.append(conv)
        return real(conv, x)

    monkeypatch.setattr(bdt, "deblock", counted)
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
               NUM_UPSAMPLE_FILTERS=list(up_filters), FUSED_TRAIN=True, FUSED_TRAIN_DEBLOCKS=True)
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
    assert bev.fused_train_deblocks is False
    assert backbone([32, 64], [64, 32]).fused_train_deblocks is True


@pytest.mark.parametrize("filters,up_filters", [([128, 256], [256, 256]), ([32, 64], [64, 32])])
@pytest.mark.parametrize("fused_bn", [False, True])
def test_two_block_backbone_training_step(filters, up_filters, fused_bn, deblock_calls):
    bev = backbone(filters, up_filters, FUSED_BN=fused_bn)
    assert bev.fused_train and bev.fused_train_deblocks and bev.fused_bn is fused_bn
    state = copy.deepcopy(bev.state_dict())
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(2, filters[0], 12, 10, generator=g).clamp_(min=0).to(DEV)
    seed_grad = torch.randn(2, sum(up_filters), 12, 10, generator=g).to(DEV)
    seen, handles = library_calls(bev)
    on = bev_step(bev, x0, seed_grad)
    # both deblocks through the Function; only the stride-2 layer is called as a module
    assert [id(m) for m in deblock_calls] == [id(bev.deblocks[0][0]), id(bev.deblocks[1][0])]
    assert [id(m) for m in seen] == [id(bev.blocks[1][1])]
    assert tuple(on[0]["spatial_features_2d"].shape) == (2, sum(up_filters), 12, 10)
    assert set(on[0]) == {"spatial_features_1x", "spatial_features_2x", "spatial_features_2d"}
    # the new switch off: both deblocks are modules again
    bev.load_state_dict(state)
    bev.fused_train_deblocks = False
    del deblock_calls[:], seen[:]
    no_deblocks = bev_step(bev, x0, seed_grad)
    assert deblock_calls == [] and sorted(id(m) for m in seen) == sorted(id(m) for m in (bev.blocks[1][1], bev.deblocks[0][0], bev.deblocks[1][0]))
    # fused_train off: the new switch alone does nothing
    bev.load_state_dict(state)
    bev.fused_train_deblocks, bev.fused_train = True, False
    del seen[:]
    off = bev_step(bev, x0, seed_grad)
    assert deblock_calls == [] and len(seen) == 6
    for h in handles:
        h.remove()
    ref = copy.deepcopy(bev)
    ref.load_state_dict(state)
    ref = ref.double().cpu().train()
    want = bev_step(ref, x0.double().cpu(), seed_grad.double().cpu())
    assert sorted(want[2]) == sorted(on[2]) == sorted(k for k, _ in bev.named_parameters())  # state-dict keys unchanged
    assert sorted(bev.state_dict()) == sorted(state)
    compare(on, want, "on vs float64")
    compare(on, no_deblocks, "on vs deblocks off")
    compare(on, off, "on vs fused_train off")


@pytest.mark.parametrize("why", ["eval", "no_grad", "amp", "train_off"])
def test_the_switch_alone_is_inert(why, deblock_calls):
    bev = backbone([32, 64], [64, 32])
    if why == "eval":
        bev.eval()
    if why == "amp":
        bev.use_amp = True
    if why == "train_off":
        bev.fused_train = False
    seen, handles = library_calls(bev)
    x = torch.randn(1, 32, 6, 6, generator=torch.Generator().manual_seed(3)).to(DEV)
    with (torch.no_grad() if why == "no_grad" else torch.enable_grad()):
        out = bev(dict(spatial_features=x.requires_grad_(why != "no_grad")))
    for h in handles:
        h.remove()
    assert deblock_calls == [] and len(seen) == 6 and out["spatial_features_2d"].is_contiguous()


def test_unsupported_deblocks_stay_modules(deblock_calls):
    """A deblock with a bias, and the trailing deblock over the concatenated tensor, run as modules; the others through the Function."""
    torch.manual_seed(8)
    bev = BaseBEVBackbone(Config.wrap(dict(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=[32, 64], UPSAMPLE_STRIDES=[1, 2, 1],
                                           NUM_UPSAMPLE_FILTERS=[64, 32, 0], FUSED_TRAIN=True, FUSED_TRAIN_DEBLOCKS=True)), 32)
    assert len(bev.deblocks) == 3
    bev.deblocks[0][0] = nn.ConvTranspose2d(32, 64, 1, stride=1, bias=True)
    bev = randomise_batch_norms(bev, 9).to(DEV).train()
    state = copy.deepcopy(bev.state_dict())
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(2, 32, 8, 6, generator=g).clamp_(min=0).to(DEV)
    seed_grad = torch.randn(2, 96, 8, 6, generator=g).to(DEV)
    seen, handles = library_calls(bev)
    on = bev_step(bev, x0, seed_grad)
    assert [id(m) for m in deblock_calls] == [id(bev.deblocks[1][0])]
    assert sorted(id(m) for m in seen) == sorted(id(m) for m in (bev.blocks[1][1], bev.deblocks[0][0], bev.deblocks[2][0]))
    for h in handles:
        h.remove()
    bev.load_state_dict(state)
    bev.fused_train = False
    off = bev_step(bev, x0, seed_grad)
    # a bias in front of a training-mode BatchNorm has no gradient but rounding: held to the weight gradient's scale on both paths
    for run in (on, off):
        noise = run[2].pop("deblocks.0.0.bias")
        assert float(noise.abs().max()) <= TOL * float(run[2]["deblocks.0.0.weight"].abs().max())
    compare(on, off, "on vs off")


def test_a_trailing_deblock_of_a_covered_shape_stays_a_module(deblock_calls):
    """The trailing deblock over the concatenated tensor is ConvTranspose2d(256, 256, 2, stride=2) here: a shape the Function
    covers and the fixture routes.  It is still called as a module -- the trailing call is made without the flag."""
    torch.manual_seed(10)
    bev = BaseBEVBackbone(Config.wrap(dict(LAYER_NUMS=[1, 1], LAYER_STRIDES=[1, 2], NUM_FILTERS=[32, 64], UPSAMPLE_STRIDES=[1, 2, 2],
                                           NUM_UPSAMPLE_FILTERS=[64, 192, 0], FUSED_TRAIN=True, FUSED_TRAIN_DEBLOCKS=True)), 32)
    bev = randomise_batch_norms(bev, 11).to(DEV).train()
    trailing = bev.deblocks[2][0]
    assert bdt.deblock_shape(trailing) == (2, 256, 256) and bdt.deblock_train_routed(trailing)
    assert bdt.deblock_train_routed(bev.deblocks[0][0]) and not bdt.deblock_train_supported(bev.deblocks[1][0])  # (2, 64, 192)
    state = copy.deepcopy(bev.state_dict())
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, 32, 8, 6, generator=g).clamp_(min=0).to(DEV)
    seed_grad = torch.randn(2, 256, 16, 12, generator=g).to(DEV)
    seen, handles = library_calls(bev)
    on = bev_step(bev, x0, seed_grad)
    assert [id(m) for m in deblock_calls] == [id(bev.deblocks[0][0])]
    assert sorted(id(m) for m in seen) == sorted(id(m) for m in (bev.blocks[1][1], bev.deblocks[1][0], trailing))
    for h in handles:
        h.remove()
    bev.load_state_dict(state)
    bev.fused_train = False
    compare(on, bev_step(bev, x0, seed_grad), "on vs off")


def test_detector_training_step_with_every_bev_switch_on(deblock_calls):
    """mssvt.yaml with FUSED_TRAIN + FUSED_BN on both dense modules and FUSED_TRAIN_DEBLOCKS on the backbone: one training step;
    every parameter the switch-off step gives a gradient gets a finite one, the loss is within 1e-3 relative of that step's.
    At the sibling test's size (tests/test_bev_conv_train_modules_gpu.py): two detectors built and stepped once each, about 55 s
    on an MI355X when this is the first detector step of the process (the library's first calls), far above the few seconds of
    every other test here."""
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
        cfg.MODEL.BACKBONE_2D["FUSED_TRAIN_DEBLOCKS"] = on
        torch.manual_seed(0)
        det = centerpoint.build_detector(cfg).to(DEV).train()
        assert det.backbone_2d.fused_train_deblocks is on and det.backbone_2d.fused_train is True
        before = len(deblock_calls)
        ret, _, _ = det(dict(points=pts, batch_size=B, gt_boxes=torch.from_numpy(gt).to(DEV)))
        ret["loss"].backward()
        routed = len(deblock_calls) - before
        ups = [m for m in det.backbone_2d.modules() if isinstance(m, nn.ConvTranspose2d)]
        assert routed == (sum(bdt.deblock_train_routed(m) for m in ups) if on else 0)
        assert not on or routed == 2
        for k, v in det.named_parameters():
            if v.grad is not None:
                assert bool(torch.isfinite(v.grad).all()), k
            if k.split(".")[0] == "backbone_2d":
                assert v.grad is not None and float(v.grad.abs().sum()) > 0, k
        with_grad[on] = sorted(k for k, v in det.named_parameters() if v.grad is not None)
        losses[on] = ret["loss"].item()
        print("detector training step, fused_train_deblocks %s: loss %.6f" % (on, losses[on]))
        assert np.isfinite(losses[on]) and losses[on] > 0
        del det, ret
    assert with_grad[True] == with_grad[False]
    assert abs(losses[True] - losses[False]) <= 1e-3 * abs(losses[False]), losses
