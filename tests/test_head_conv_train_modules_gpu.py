"""``CenterHead`` in TRAINING mode with ``fused_train`` on (with and without ``fused_bn``): one training step against a float64 CPU
copy of the same module (the project's 1e-3 relative parity tolerance, as tests/test_bev_down_train_modules_gpu.py) and against
the switch-off run; the reference-run golden at tests/test_head_train_cpu.py's tolerances; the routed stages record no library
convolution; the switch is inert wherever ``head_conv_train.applies`` says so; the whole detector with every switch on."""
import copy
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from mssvt_amd import bn_train, head_conv_train as hct, synthetic
from mssvt_amd.center_head import CenterHead
from mssvt_amd.config import Config
from tests import head_conv_ref
from tests.test_head_train_cpu import _check as check_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1e-3
HEADS = [["Vehicle", "Pedestrian"], ["Cyclist"]]


def close(got, want, what):
    got, want = got.detach().double().cpu().numpy(), want.detach().double().cpu().numpy()
    assert got.shape == want.shape, what
    scale = float(np.abs(want).max())
    err = float(np.abs(got - want).max())
    assert err <= TOL * max(scale, 1e-30), (what, err, scale)


@pytest.fixture
def train_calls(monkeypatch):
    """Records the heads that really run through ``head_conv_train.forward_train`` and the BatchNorms through ``bn_relu``."""
    calls = dict(forward=[], bn=[])
    real_f, real_b = hct.forward_train, bn_train.bn_relu
    monkeypatch.setattr(hct, "forward_train", lambda head, x: (calls["forward"].append(head), real_f(head, x))[1])
    monkeypatch.setattr(bn_train, "bn_relu", lambda bn, x, relu: (calls["bn"].append(bn), real_b(bn, x, relu))[1])
    return calls


def library_calls(module):
    """Forward hooks on every convolution module: the modules called AS MODULES."""
    seen, handles = [], []
    for m in module.modules():
        if isinstance(m, nn.Conv2d):
            handles.append(m.register_forward_hook(lambda mod, inp, out: seen.append(mod)))
    return seen, handles


def small_head(cin=64, **kw):
    kw.setdefault("heads", HEADS)
    head = head_conv_ref.build_head(cin, seed=3, **kw)
    head.model_cfg["LOSS_CONFIG"] = Config.wrap(dict(LOSS_WEIGHTS=dict(cls_weight=1.0, loc_weight=0.25,
                                                                       code_weights=[1.0] * (10 if kw.get("vel") else 8))))
    return head


def boxes(B, device, dtype=torch.float32, vel=False):
    """A few boxes whose centres fall on the small map (the head's range starts at -20 m, one cell per metre); with `vel` two
    velocity columns in front of the class."""
    rng = np.random.default_rng(4)
    gt = np.zeros((B, 6, 8), np.float32)
    for b in range(B):
        n = 5 - b
        gt[b, :n, 0] = rng.uniform(-19, -7, n)
        gt[b, :n, 1] = rng.uniform(-19, -9, n)
        gt[b, :n, 2] = rng.uniform(-1, 1, n)
        gt[b, :n, 3:6] = rng.uniform([1.5, 0.8, 1.0], [4.0, 2.0, 2.0], (n, 3))
        gt[b, :n, 6] = rng.uniform(-3.1, 3.1, n)
        gt[b, :n, 7] = rng.integers(1, 4, n)
    if vel:
        v = np.zeros((B, 6, 2), np.float32)
        v[:, :4] = rng.uniform(-2, 2, (B, 4, 2))
        gt = np.concatenate([gt[..., :7], v, gt[..., 7:]], axis=2)
    return torch.from_numpy(gt).to(device=device, dtype=dtype)


def head_step(head, x0):
    """One training step: (loss, input gradient, {parameter: gradient}, {buffer: value after the step})."""
    head.zero_grad(set_to_none=True)
    x = x0.clone().requires_grad_(True)
    vel = "vel" in head.heads_list[0].sep_head_dict
    head(dict(spatial_features_2d=x, batch_size=x.shape[0], gt_boxes=boxes(x.shape[0], x.device, x.dtype, vel)))
    loss, _ = head.get_loss()
    loss.backward()
    return (loss.detach(), x.grad.clone(), {k: v.grad.clone() for k, v in head.named_parameters()},
            {k: v.detach().clone() for k, v in head.named_buffers() if v.dtype.is_floating_point})


def compare(a, b, what):
    close(a[0], b[0], what + " loss")
    close(a[1], b[1], what + " input gradient")
    assert sorted(a[2]) == sorted(b[2])
    for k in a[2]:
        if k.endswith("0.bias") and k[:-4] + "weight" in a[2] and a[2][k[:-4] + "weight"].dim() == 4:
            # the bias of a convolution in front of a BatchNorm2d in training mode: the batch mean takes a constant shift out, so
            # its exact gradient is ZERO and both runs hold rounding noise.  It is the sum over the pixels of the same dY whose
            # products with x make the weight's gradient: held to the tolerance on that gradient's scale
            scale = float(b[2][k[:-4] + "weight"].abs().max())
            for run in (a, b):
                assert float(run[2][k].abs().max()) <= TOL * scale, (what, k)
            continue
        close(a[2][k], b[2][k], "%s d %s" % (what, k))
    assert sorted(a[3]) == sorted(b[3])
    for k in a[3]:
        close(a[3][k], b[3][k], "%s buffer %s" % (what, k))


def test_the_yaml_keys_and_the_defaults():
    head = small_head()
    assert head.fused_train is False and head.fused_bn is False
    cfg = head_conv_ref.head_config(shared=32, heads=HEADS)
    cfg.update(FUSED_TRAIN=True, FUSED_BN=True)
    on = CenterHead(Config.wrap(cfg), 64, 3, head_conv_ref.CLASSES, np.array([40, 40, 1]), np.array([-20.0, -20.0, -2.0, 20.0, 20.0, 4.0]),
                    [1.0, 1.0, 6.0])
    assert on.fused_train is True and on.fused_bn is True and on.fused_convs is False
    cfg.update(FUSED_BN=False)
    assert CenterHead(Config.wrap(cfg), 64, 3, head_conv_ref.CLASSES, np.array([40, 40, 1]),
                      np.array([-20.0, -20.0, -2.0, 20.0, 20.0, 4.0]), [1.0, 1.0, 6.0]).fused_bn is False
    assert hct.ROUTED_TRAIN <= frozenset(hct.STAGES) and hct.ROUTED_BN <= frozenset({32, 64})
    from mssvt_amd import config
    assert "FUSED_TRAIN" not in config.load_yaml(config.DEFAULT_CFG).MODEL.DENSE_HEAD  # off unless a yaml says so


@pytest.mark.parametrize("vel", [False, True])
@pytest.mark.parametrize("fused_bn", [False, True])
def test_head_training_step(vel, fused_bn, train_calls):
    """(64 -> 32, two heads): the loss, every parameter gradient, the input gradient and the running statistics after the step
    against the float64 CPU copy and against the switch-off run."""
    head = small_head(vel=vel).to(DEV).train()
    head.fused_train, head.fused_bn = True, fused_bn
    assert hct.train_supported(head) and hct.routed_stages(head) == frozenset(hct.STAGES)
    state = copy.deepcopy(head.state_dict())
    nb = sum(len(sep.sep_head_dict) for sep in head.heads_list)
    assert nb == (12 if vel else 10)
    x0 = torch.randn(2, 64, 13, 15, generator=torch.Generator().manual_seed(2)).to(DEV)
    seen, handles = library_calls(head)
    on = head_step(head, x0)
    # the shared layer and the nb first convolutions never ran as modules; the nb finals did
    finals = [getattr(sep, name)[1] for sep in head.heads_list for name in sep.sep_head_dict]
    assert [id(h) for h in train_calls["forward"]] == [id(head)]
    assert sorted(id(m) for m in seen) == sorted(id(m) for m in finals)
    assert len(train_calls["bn"]) == (1 + nb if fused_bn else 0)
    pred = head.forward_ret_dict["pred_dicts"]
    assert [list(p) for p in pred] == [list(sep.sep_head_dict) for sep in head.heads_list]
    assert all(tuple(v.shape) == (2, v.shape[1], 13, 15) for p in pred for v in p.values())
    # the switch off
    head.load_state_dict(state)
    head.fused_train = False
    del seen[:]
    off = head_step(head, x0)
    assert len(train_calls["forward"]) == 1 and len(seen) == 1 + 2 * nb
    off_pred = head.forward_ret_dict["pred_dicts"]
    assert [[tuple(v.shape) for v in p.values()] for p in pred] == [[tuple(v.shape) for v in p.values()] for p in off_pred]
    for h in handles:
        h.remove()
    head.forward_ret_dict = {}  # (holds tensors of the last step's graph: not deep-copyable)
    ref = copy.deepcopy(head)
    ref.load_state_dict(state)
    ref = ref.double().cpu().train()
    want = head_step(ref, x0.double().cpu())
    assert sorted(want[2]) == sorted(on[2]) == sorted(k for k, _ in head.named_parameters())
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in on[2].values())
    compare(on, want, "on vs float64")
    compare(on, off, "on vs switch off")
    compare(off, want, "switch off vs float64")


def test_reference_run_golden_with_the_switch_on(golden_dir, train_calls):
    """tests/golden/det_head_train.npz (64 -> 32 with bias: a covered head) on the GPU through ``forward_train``, at
    tests/test_head_train_cpu.py's tolerances."""
    d = np.load(os.path.join(golden_dir, "det_head_train.npz"))
    cfg = json.loads(str(d["cfg_json"]))
    for fused_bn in (False, True):
        head = CenterHead(cfg["HEAD"], cfg["input_channels"], len(cfg["CLASSES"]), cfg["CLASSES"], np.array(cfg["GRID"]),
                          np.array(cfg["PCR"]), cfg["VOXEL"], predict_boxes_when_training=False)
        head.load_state_dict({k[5:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("head.")}, strict=True)
        head = head.to(DEV).train()
        head.fused_train, head.fused_bn = True, fused_bn
        assert hct.train_supported(head)
        del train_calls["forward"][:]
        head(dict(spatial_features_2d=torch.from_numpy(d["spatial_features_2d"]).to(DEV), batch_size=int(d["batch_size"]),
                  gt_boxes=torch.from_numpy(d["gt_boxes"]).to(DEV)))
        assert [id(h) for h in train_calls["forward"]] == [id(head)]
        check_golden(d, head)


def test_the_routed_stages_record_no_library_convolution():
    """Under the profiler the forward and backward of both Functions record no convolution operator of the library
    (aten::convolution / miopen_convolution / convolution_backward), while the same layers as modules record them."""
    from torch.profiler import ProfilerActivity, profile
    torch.manual_seed(3)
    shared = nn.Conv2d(64, 32, 3, padding=1, bias=True).to(DEV)
    firsts = [nn.Conv2d(32, 32, 3, padding=1, bias=(b == 0)).to(DEV) for b in range(3)]
    x0 = torch.randn(2, 64, 9, 12, device=DEV).contiguous(memory_format=torch.channels_last)
    gs = [torch.randn(2, 32, 9, 12, device=DEV) for _ in range(3)]

    def step(fused):
        for m in [shared] + firsts:
            m.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        with profile(activities=[ProfilerActivity.CPU]) as prof:
            if fused:
                y = hct.SharedFunction.apply(x, shared.weight, shared.bias)
                ts = hct.TrunkFunction.apply(y, 3, *([m.weight for m in firsts] + [m.bias for m in firsts]))
            else:
                y = shared(x)
                ts = [m(y) for m in firsts]
            torch.autograd.backward(list(ts), gs)
        torch.cuda.synchronize()
        names = {e.key for e in prof.key_averages()}
        grads = [x.grad, shared.weight.grad, shared.bias.grad] + [m.weight.grad for m in firsts] + [firsts[0].bias.grad]
        return [t.detach() for t in ts] + grads, sorted(n for n in names if "conv" in n.lower() and n.startswith("aten::"))

    ours, names = step(True)
    assert names == [], names
    lib, lib_names = step(False)
    assert any("convolution" in n for n in lib_names), lib_names
    for k, (u, v) in enumerate(zip(ours, lib)):
        close(u, v, "tensor %d" % k)


@pytest.mark.parametrize("why", ["eval", "no_grad", "autocast", "use_amp", "cpu", "num_conv", "s48", "train_off"])
def test_the_switch_is_inert(why, train_calls):
    kw = {}
    if why == "num_conv":
        kw["num_conv"] = {"center": 1}
    if why == "s48":
        kw["shared"] = 48
    head = small_head(**kw).to("cpu" if why == "cpu" else DEV).train()
    head.fused_train = head.fused_bn = True
    if why == "eval":
        head.eval()
    if why == "use_amp":
        head.use_amp = True
    if why == "train_off":
        head.fused_train = False  # fused_bn alone
    assert hct.train_supported(head) == (why not in ("cpu", "num_conv", "s48"))
    nb = sum(len(sep.sep_head_dict) for sep in head.heads_list)
    seen, handles = library_calls(head)
    x = torch.randn(1, 64, 8, 9, generator=torch.Generator().manual_seed(3)).to("cpu" if why == "cpu" else DEV)  # (>= 50 cells)
    x.requires_grad_(why != "no_grad")
    data = dict(spatial_features_2d=x, batch_size=1, gt_boxes=boxes(1, x.device))
    assert not hct.applies(head, x) or why in ("no_grad", "autocast")  # (those two conditions hold inside the regions below)
    with (torch.no_grad() if why == "no_grad" else torch.enable_grad()):
        with torch.autocast("cuda", enabled=(why == "autocast")):
            assert not hct.applies(head, x)
            head(data)
    for h in handles:
        h.remove()
    assert train_calls["forward"] == [] and train_calls["bn"] == []
    assert len(seen) == 1 + 2 * nb - (1 if why == "num_conv" else 0) * len(head.heads_list)


def test_detector_training_step_with_every_switch_on(train_calls):
    """mssvt.yaml with every BEV switch plus the head's FUSED_TRAIN + FUSED_BN and ``fused_loss`` on, against the all-off run: one
    training step each; every parameter the switch-off step gives a gradient gets a finite one, the loss is within 1e-3 relative
    of that step's.  The product stages are routed here whatever ``ROUTED_TRAIN`` holds: the rule is a question of speed."""
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
    mp = pytest.MonkeyPatch()
    mp.setattr(hct, "ROUTED_TRAIN", frozenset(hct.STAGES))
    mp.setattr(hct, "ROUTED_BN", frozenset({64}))
    try:
        for on in (True, False):
            cfg = config.load_yaml(config.DEFAULT_CFG)
            for key in ("FUSED_TRAIN", "FUSED_BN"):
                cfg.MODEL.MAP_TO_BEV[key] = on
                cfg.MODEL.BACKBONE_2D[key] = on
                cfg.MODEL.DENSE_HEAD[key] = on
            cfg.MODEL.BACKBONE_2D["FUSED_TRAIN_DEBLOCKS"] = on
            cfg.MODEL.BACKBONE_2D["FUSED_TRAIN_DOWN"] = on
            torch.manual_seed(0)
            det = centerpoint.build_detector(cfg).to(DEV).train()
            det.dense_head.fused_loss = on
            assert det.dense_head.fused_train is on and det.dense_head.fused_bn is on
            before = len(train_calls["forward"])
            ret, _, _ = det(dict(points=pts, batch_size=B, gt_boxes=torch.from_numpy(gt).to(DEV)))
            ret["loss"].backward()
            assert len(train_calls["forward"]) - before == (1 if on else 0)
            for k, v in det.named_parameters():
                if v.grad is not None:
                    assert bool(torch.isfinite(v.grad).all()), k
                if k.split(".")[0] == "dense_head":
                    assert v.grad is not None, k
                if k.startswith("dense_head.") and (k.endswith("shared_conv.0.weight") or k.endswith(".0.0.weight")):
                    assert float(v.grad.abs().sum()) > 0, k  # (the layers the Functions ran)
            with_grad[on] = sorted(k for k, v in det.named_parameters() if v.grad is not None)
            losses[on] = float(ret["loss"])
            print("detector training step, every switch %s: loss %.6f" % (on, losses[on]))
            assert np.isfinite(losses[on]) and losses[on] > 0
            del det, ret
    finally:
        mp.undo()
    assert with_grad[True] == with_grad[False]
    assert abs(losses[True] - losses[False]) <= 1e-3 * abs(losses[False]), losses
