"""``DynamicVFE.fused_train`` on the MI355X: the training step on the run kernels of csrc/vfe_train.hip against the reference's own
training step (tests/golden/dynamic_vfe_train_32_64.npz, with the checks and tolerances of
tests/test_vfe_train_cpu.py::_check) and against the torch branch of the same module on the same inputs (voxel_coords equal,
features and every parameter gradient within those same tolerances: BatchNorm sees the same rows in another order, so its
statistics differ by rounding only)."""
import os

import numpy as np
import pytest
import torch

from mssvt_amd import synthetic
from mssvt_amd.dynamic_vfe import DynamicVFE
from tests.test_vfe_train_cpu import _check

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the MI355X")]
DEV = "cuda"


def golden_module(golden_dir, fused):
    d = np.load(os.path.join(golden_dir, "dynamic_vfe_train_32_64.npz"))
    cfg = dict(NUM_FILTERS=d["num_filters"].tolist(), WITH_CLUSTER_CENTER=True, WITH_VOXEL_CENTER=True)
    vfe = DynamicVFE(cfg, 5, d["voxel_size"].tolist(), d["grid_size"].tolist(), d["point_cloud_range"].tolist())
    vfe.load_state_dict({k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd.")}, strict=True)
    vfe = vfe.to(DEV).train()
    vfe.fused_train = fused
    return d, vfe


def golden_step(golden_dir, fused):
    d, vfe = golden_module(golden_dir, fused)
    out = vfe(dict(points=torch.from_numpy(d["points"]).to(DEV), batch_size=int(d["batch_size"])))
    (out["voxel_features"] * torch.from_numpy(d["weight_of_the_loss"]).to(DEV)).sum().backward()
    return d, vfe, out


@pytest.fixture
def calls(monkeypatch):
    """counts which branch a forward takes"""
    seen = dict(fused=0, torch=0)
    fused, plain = DynamicVFE._forward_train_fused, DynamicVFE._forward_train

    def count_fused(self, batch_dict):
        seen["fused"] += 1
        return fused(self, batch_dict)

    def count_plain(self, batch_dict):
        seen["torch"] += 1
        return plain(self, batch_dict)

    monkeypatch.setattr(DynamicVFE, "_forward_train_fused", count_fused)
    monkeypatch.setattr(DynamicVFE, "_forward_train", count_plain)
    return seen


def test_the_switch_is_off_by_default_and_read_from_the_config():
    args = (5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE, synthetic.POINT_CLOUD_RANGE)
    assert DynamicVFE(dict(NUM_FILTERS=[32, 64]), *args).fused_train is False
    assert DynamicVFE(dict(NUM_FILTERS=[32, 64], FUSED_TRAIN=True), *args).fused_train is True


def test_fused_training_step_matches_the_reference_run(golden_dir, calls):
    d, vfe, out = golden_step(golden_dir, True)
    assert calls == dict(fused=1, torch=0)
    assert out["voxel_coords"].dtype == torch.int32 and out["voxel_coords"].is_contiguous()
    _check(d, vfe, out)


def compare_with_torch_branch(make, points, batch_size, weight_seed=0):
    """the same module and inputs through both branches; the checks of _check between them"""
    res = []
    for fused in (True, False):
        torch.manual_seed(11)
        vfe = make().to(DEV).train()
        vfe.fused_train = fused
        # the torch branch under torch's deterministic algorithms (ordered index_add / index_put instead of float atomics):
        # with atomics its activations move in the last bits from run to run, and one that sits within rounding of the
        # ReLU's edge then switches a whole gradient term on or off -- the reference of this comparison must not do that
        was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
        torch.use_deterministic_algorithms(not fused, warn_only=True)
        try:
            out = vfe(dict(points=points.clone(), batch_size=batch_size))
            w = torch.randn(out["voxel_features"].shape, generator=torch.Generator().manual_seed(weight_seed)).to(DEV)
            (out["voxel_features"] * w).sum().backward()
        finally:
            torch.use_deterministic_algorithms(was, warn_only=warn)
        res.append((vfe, out))
    (fv, fo), (tv, to) = res
    assert torch.equal(fo["voxel_coords"], to["voxel_coords"])
    got_f, want_f = fo["voxel_features"].detach().cpu().numpy(), to["voxel_features"].detach().cpu().numpy()
    print("features: max |err| / tolerance %.3g" % float((np.abs(got_f - want_f) / (1e-5 + 1e-5 * np.abs(want_f))).max()))
    np.testing.assert_allclose(got_f, want_f, rtol=1e-5, atol=1e-5)
    want = {k: v.grad.cpu().numpy() for k, v in tv.named_parameters()}
    scale = max(float(np.abs(v).max()) for v in want.values())
    for k, v in fv.named_parameters():
        assert v.grad is not None, k
        if k.endswith(".0.bias"):
            assert float(v.grad.abs().max()) <= 1e-6 * scale and float(np.abs(want[k]).max()) <= 1e-6 * scale, k
            continue
        tol = 1e-5 * max(1.0, float(np.abs(want[k]).max())) + 1e-4 * np.abs(want[k])
        print("%s: max |err| / tolerance %.3g" % (k, float((np.abs(v.grad.cpu().numpy() - want[k]) / tol).max())))
        np.testing.assert_allclose(v.grad.cpu().numpy(), want[k], rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(want[k]).max())),
                                   err_msg=k)
    for (k, a), (_, b) in zip(fv.state_dict().items(), tv.state_dict().items()):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg=k)
    return fv, fo


def test_fused_step_matches_the_torch_branch_on_the_golden_inputs(golden_dir, calls):
    d, _ = golden_module(golden_dir, True)

    def make():
        return golden_module(golden_dir, True)[1]

    compare_with_torch_branch(make, torch.from_numpy(d["points"]).to(DEV), int(d["batch_size"]))
    assert calls == dict(fused=1, torch=1)


def hand_made_cloud(n=3000, seed=0):
    """B = 2; one voxel holding 600 points, duplicated points (exact ties in front of the ReLU), points outside the range
    on every side and points exactly on the lower and the upper bounds"""
    rng = np.random.default_rng(seed)
    pts = synthetic.make_batch_points(n // 2, 2, seed)
    lo, hi = np.array(synthetic.POINT_CLOUD_RANGE[:3], np.float32), np.array(synthetic.POINT_CLOUD_RANGE[3:], np.float32)
    vs = np.array(synthetic.VOXEL_SIZE, np.float32)
    crowd = np.zeros((600, pts.shape[1]), np.float32)
    cell = lo + vs * np.array([7, 9, 3], np.float32)
    crowd[:, 1:4] = cell + vs * rng.uniform(0.05, 0.95, (600, 3)).astype(np.float32)
    crowd[:, 4:] = rng.uniform(0, 1, (600, pts.shape[1] - 4))
    crowd[300:] = crowd[:300]  # every crowd point twice
    dup = pts[:200].copy()
    outside = []
    for k in range(3):
        for side, bound in ((-1, lo), (1, hi)):
            p = pts[:5].copy()
            p[:, 1 + k] = bound[k] + side * np.float32(0.5)
            outside.append(p)
    edge_lo, edge_hi = pts[:4].copy(), pts[:4].copy()
    edge_lo[:, 1:4] = lo  # inside: cell 0
    edge_hi[:, 1:4] = hi  # outside: cell == grid size
    allp = np.concatenate([pts, crowd, dup] + outside + [edge_lo, edge_hi]).astype(np.float32)
    return torch.from_numpy(allp[rng.permutation(len(allp))]).to(DEV)


CONFIGS = {"default_64_128": dict(NUM_FILTERS=[64, 128]),
           "with_distance": dict(NUM_FILTERS=[32, 64], WITH_DISTANCE=True),
           "no_cluster_center": dict(NUM_FILTERS=[32, 64], WITH_CLUSTER_CENTER=False),
           "one_filter": dict(NUM_FILTERS=[64])}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_fused_step_matches_the_torch_branch(name, calls):
    def make():
        return DynamicVFE(CONFIGS[name], 5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE, synthetic.POINT_CLOUD_RANGE)

    compare_with_torch_branch(make, hand_made_cloud(), 2)
    assert calls == dict(fused=1, torch=1)


def test_two_identical_steps_are_bit_identical(calls):
    pts = hand_made_cloud()
    runs = []
    for _ in range(2):
        torch.manual_seed(5)
        vfe = DynamicVFE(CONFIGS["default_64_128"], 5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE,
                         synthetic.POINT_CLOUD_RANGE).to(DEV).train()
        vfe.fused_train = True
        out = vfe(dict(points=pts, batch_size=2))
        w = torch.randn(out["voxel_features"].shape, generator=torch.Generator().manual_seed(1)).to(DEV)
        (out["voxel_features"] * w).sum().backward()
        runs.append((out["voxel_features"].detach(), {k: v.grad for k, v in vfe.named_parameters()}))
    assert calls["fused"] == 2 and calls["torch"] == 0
    assert torch.equal(runs[0][0], runs[1][0])
    for k in runs[0][1]:
        assert torch.equal(runs[0][1][k], runs[1][1][k]), k


def test_train_mode_under_no_grad_moves_the_statistics_and_builds_no_graph(golden_dir, calls):
    d, vfe = golden_module(golden_dir, True)
    batch = dict(points=torch.from_numpy(d["points"]).to(DEV), batch_size=int(d["batch_size"]))
    before = vfe.pfn[0][1].running_mean.clone()
    with torch.no_grad():
        quiet = vfe(dict(batch))
    assert not quiet["voxel_features"].requires_grad and quiet["voxel_features"].grad_fn is None
    assert not torch.equal(before, vfe.pfn[0][1].running_mean)
    d2, vfe2 = golden_module(golden_dir, True)
    graph = vfe2(dict(batch))
    assert graph["voxel_features"].requires_grad
    assert torch.equal(quiet["voxel_features"], graph["voxel_features"].detach())
    assert calls == dict(fused=2, torch=0)


def test_sync_batchnorm_conversion_reaches_both_layers_and_the_fused_step_runs_through_them(golden_dir, calls):
    """One process, no collective: outside a process group SyncBatchNorm normalises with the batch statistics of its own
    rows, so the converted module's fused step is held to the reference run like the unconverted one."""
    d, vfe = golden_module(golden_dir, True)
    keys = list(vfe.state_dict().keys())
    conv = torch.nn.SyncBatchNorm.convert_sync_batchnorm(vfe)
    assert [type(blk[1]) for blk in conv.pfn] == [torch.nn.SyncBatchNorm] * 2
    assert list(conv.state_dict().keys()) == keys
    assert conv.fused_train is True
    out = conv(dict(points=torch.from_numpy(d["points"]).to(DEV), batch_size=int(d["batch_size"])))
    (out["voxel_features"] * torch.from_numpy(d["weight_of_the_loss"]).to(DEV)).sum().backward()
    assert calls == dict(fused=1, torch=0)
    _check(d, conv, out)


def both_branches(make, batch):
    """(outcome of the flag set, outcome of the flag clear): the outputs, or the exception's type"""
    res = []
    for fused in (True, False):
        torch.manual_seed(3)
        vfe = make().to(DEV).train()
        vfe.fused_train = fused
        try:
            out = vfe(dict(batch))
            res.append((out["voxel_features"], out["voxel_coords"]))
        except Exception as e:  # noqa: BLE001 -- the torch branch's own behaviour, whatever it is, is the expectation
            res.append(type(e))
    return res


def assert_same(a, b):
    if isinstance(a, type) or isinstance(b, type):
        assert a is b, (a, b)
        return
    assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


def test_what_the_kernels_do_not_cover_takes_the_torch_branch(calls):
    """With the flag set, what the kernels do not cover must run the torch branch (counted) and give what it gives.  The
    modules here have no cluster centre: that is the torch branch's one forward reduction on float atomics (two of ITS runs
    differ in the last bits), without it its forward is a function of its inputs and the outputs must be EQUAL."""
    args = (5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE, synthetic.POINT_CLOUD_RANGE)
    pts = hand_made_cloud(1000)
    # a width that is no multiple of 4
    a, b = both_branches(lambda: DynamicVFE(dict(NUM_FILTERS=[30, 64], WITH_CLUSTER_CENTER=False), *args),
                         dict(points=pts, batch_size=2))
    assert_same(a, b)
    assert calls == dict(fused=0, torch=2)
    # points that carry a gradient
    a, b = both_branches(lambda: DynamicVFE(dict(NUM_FILTERS=[32, 64], WITH_CLUSTER_CENTER=False), *args),
                         dict(points=pts.clone().requires_grad_(), batch_size=2))
    assert_same(a, b)
    assert calls == dict(fused=0, torch=4)
    # every point outside the grid: the fused step finds N == 0 and hands over
    far = pts.clone()
    far[:, 1] = synthetic.POINT_CLOUD_RANGE[3] + 10.0
    a, b = both_branches(lambda: DynamicVFE(dict(NUM_FILTERS=[32, 64], WITH_CLUSTER_CENTER=False), *args),
                         dict(points=far, batch_size=2))
    assert_same(a, b)
    assert calls == dict(fused=1, torch=6)


def test_autocast_takes_the_torch_branch(calls):
    """under autocast the PFN layers produce half-precision rows, which the run kernels do not take: the step must fall back
    before it starts, not raise in the middle"""
    args = (5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE, synthetic.POINT_CLOUD_RANGE)
    pts = hand_made_cloud(1000)
    with torch.autocast("cuda"):
        a, b = both_branches(lambda: DynamicVFE(dict(NUM_FILTERS=[32, 64], WITH_CLUSTER_CENTER=False), *args),
                             dict(points=pts, batch_size=2))
    assert_same(a, b)
    assert calls == dict(fused=0, torch=2)


def test_eval_mode_ignores_the_flag(golden_dir, calls):
    """the flag from the config key: eval mode never enters either training branch and gives the bits it gives without it"""
    d, plain = golden_module(golden_dir, False)
    cfg = dict(NUM_FILTERS=d["num_filters"].tolist(), WITH_CLUSTER_CENTER=True, WITH_VOXEL_CENTER=True, FUSED_TRAIN=True)
    vfe = DynamicVFE(cfg, 5, d["voxel_size"].tolist(), d["grid_size"].tolist(), d["point_cloud_range"].tolist())
    vfe.load_state_dict(plain.state_dict(), strict=True)
    vfe = vfe.to(DEV).eval()
    plain.eval()
    assert vfe.fused_train is True and plain.fused_train is False
    batch = dict(points=torch.from_numpy(d["points"]).to(DEV), batch_size=int(d["batch_size"]))
    on, off = vfe(dict(batch)), plain(dict(batch))
    assert calls == dict(fused=0, torch=0)
    assert torch.equal(on["voxel_features"], off["voxel_features"]) and torch.equal(on["voxel_coords"], off["voxel_coords"])
    vfe.train()
    vfe(dict(batch))
    assert calls == dict(fused=1, torch=0)  # and the same module trains on the fused step
