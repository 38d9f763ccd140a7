"""CenterHead's fused loss on the MI355X (csrc/center_loss.hip through ``center_head.center_loss`` and
``CenterHead.fused_loss``) against its numpy float64 statement (tests/center_loss_ref.py), forward values and every gradient.

Bounds (the project's own for this quantity, tests/test_head_train_cpu.py): loss terms 1e-5 relative to the float64
reference; gradients rtol 1e-4, atol 1e-5 max(1, max|want|); num_pos and num equal; gradients at saturated logits exactly 0.
Sizes where the heat-map kernels change path (tests/center_loss_cases.py mirrors the kernel's constants, and
tests/test_center_loss_cpu.py holds the mirror to the header): one workgroup sweeps SWEEP = 1024 elements per step as one
float4 per thread, the grid is min(ceil(n / SWEEP), MAX_BLOCKS = 2048): n = 1 and 15 (no float4 at all), n % 4 != 0,
n = SWEEP - 1, SWEEP, SWEEP + 1, MAX_BLOCKS SWEEP + 4 (the first float4 of a second grid-stride step); logits one float
off the 16-byte boundary with the targets on it (the scalar kernel) and with the targets off it too (a 3-element head)."""
import json

import numpy as np
import pytest
import torch

from mssvt_amd import _lib, center_head
from mssvt_amd.center_head import center_loss
from tests import center_loss_cases as cases
from tests import center_loss_ref as ref
from tests.test_head_train_cpu import _check, _step

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the MI355X")]
DEV = "cuda"
G_HM, G_LOC = 3.0, 0.5

_CACHE = {}


def case_and_reference(name):
    """the case and its float64 reference (forward, and the gradients of 1 hm_loss and of 1 loc_loss: the loss is linear
    in the two upstream gradients), computed once and left unchanged"""
    if name not in _CACHE:
        c = cases.make_case(name)
        args = (c["hm"], c["heatmap"], c["maps"], c["target_boxes"], c["inds"], c["masks"], c["code_weights"], c["loc_weight"])
        fwd = ref.forward(*args)
        d_hm, _ = ref.backward(*args, g_hm=1.0, g_loc=0.0)
        _, d_maps = ref.backward(*args, g_hm=0.0, g_loc=1.0)
        _CACHE[name] = (c, fwd, d_hm, d_maps)
    return _CACHE[name]


def upload(x, offset=0, grad=False):
    """a contiguous device tensor whose first element sits `offset` floats behind a 16-byte boundary of its storage"""
    t = torch.from_numpy(np.ascontiguousarray(x))
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[offset:offset + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * offset) % 16
    return v.detach().requires_grad_(grad)


def upload_case(c, frozen=(), hm_offset=0, gt_offset=0):
    return dict(hm=upload(c["hm"], hm_offset, grad=True), maps=[upload(m, grad=k not in frozen) for k, m in enumerate(c["maps"])],
                heatmap=upload(c["heatmap"], gt_offset), target_boxes=upload(c["target_boxes"]), inds=upload(c["inds"]),
                masks=upload(c["masks"]), code_weights=upload(c["code_weights"]), loc_weight=c["loc_weight"])


def compute(t, g_hm=G_HM, g_loc=G_LOC, read_counts=True):
    """center_loss and the gradients of g_hm hm_loss + g_loc loc_loss (a None factor leaves the term out); nothing is read
    back with read_counts=False"""
    hm, maps = t["hm"], t["maps"]
    hm_loss, loc_loss, per_dim = center_loss(hm, maps, t["heatmap"], t["target_boxes"], t["inds"], t["masks"],
                                             t["code_weights"], t["loc_weight"])
    assert hm_loss.dim() == 0 and loc_loss.dim() == 0 and not per_dim.requires_grad
    counts = None
    if read_counts:  # num_pos and num: int32 bit patterns in the buffer the autograd context keeps (freed by the backward)
        counts = hm_loss.grad_fn.saved_tensors[6][2:4].view(torch.int32).cpu().numpy()
    total = sum(g * v for g, v in ((g_hm, hm_loss), (g_loc, loc_loss)) if g is not None)
    wanted = [hm] + [m for m in maps if m.requires_grad]
    grads = list(torch.autograd.grad(total, wanted))
    d_hm = grads.pop(0)
    d_maps = [grads.pop(0) if m.requires_grad else None for m in maps]
    return dict(hm_loss=hm_loss.detach(), loc_loss=loc_loss.detach(), per_dim=per_dim, counts=counts, d_hm=d_hm, d_maps=d_maps)


def run(c, g_hm=G_HM, g_loc=G_LOC, **where):
    return compute(upload_case(c, **where), g_hm, g_loc)


def assert_loss_close(got, want, what):
    got = float(got)
    print("%s: got %.9g want %.9g rel %.3g" % (what, got, want, abs(got - want) / max(abs(want), 1e-300)))
    assert np.isfinite(got), what
    assert abs(got - want) <= 1e-5 * abs(want), (what, got, want)


def assert_grad_close(got, want, what):
    got = got.cpu().numpy()
    tol = 1e-5 * max(1.0, float(np.abs(want).max())) + 1e-4 * np.abs(want)
    print("%s: max |err| / tolerance %.3g" % (what, float((np.abs(got - want) / tol).max())))
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(want).max())), err_msg=what)


def check(got, name, g_hm=G_HM, g_loc=G_LOC):
    c, fwd, d_hm, d_maps = case_and_reference(name)
    assert_loss_close(got["hm_loss"], fwd["hm_loss"], "hm_loss")
    assert_loss_close(got["loc_loss"], fwd["loc_loss"], "loc_loss")
    per_dim = got["per_dim"].cpu().numpy()
    for d in range(len(per_dim)):
        assert_loss_close(per_dim[d], fwd["per_dim"][d], "per_dim[%d]" % d)
    assert int(got["counts"][0]) == fwd["num_pos"] and int(got["counts"][1]) == fwd["num"], got["counts"]
    assert_grad_close(got["d_hm"], (g_hm or 0.0) * d_hm, "d_hm")
    for k, g in enumerate(got["d_maps"]):
        if g is not None:
            assert_grad_close(g, (g_loc or 0.0) * d_maps[k], "d_map%d" % k)
    flat = got["d_hm"].reshape(-1).cpu().numpy()
    saturated = np.flatnonzero(np.abs(c["hm"].reshape(-1)) >= 9.5)
    assert set(c["planted"].tolist()) <= set(saturated.tolist())
    assert (flat[saturated] == 0.0).all()  # through the clamp: exactly zero, not small
    assert np.isfinite(flat).all()
    return c, fwd


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_loss_and_gradients_match_the_reference(name):
    c, fwd = check(run(cases.make_case(name)), name)
    (B, C, H, W, M, D), opt = cases.CASES[name]
    if opt.get("positives") == "none":
        assert fwd["num_pos"] == 0 and fwd["hm_loss"] > 0  # the -neg branch
    if opt.get("masks") == "none":
        assert fwd["num"] == 0 and fwd["loc_loss"] == 0.0
    if opt.get("plant"):
        assert len(c["planted"]) == 6 and (c["heatmap"].reshape(-1)[c["planted"][4:]] == 1.0).all()
    if opt.get("poison"):
        assert fwd["num"] == int(c["masks"].sum()) and np.isfinite(fwd["loc_loss"])


@pytest.mark.parametrize("hm_offset,gt_offset", [(1, 0), (1, 1), (3, 3), (0, 2)])
def test_logits_off_the_16_byte_boundary(hm_offset, gt_offset):
    check(run(cases.make_case("odd_n"), hm_offset=hm_offset, gt_offset=gt_offset), "odd_n")


def test_upstream_gradients_and_a_frozen_map():
    c = cases.make_case("odd_n")
    check(run(c, g_hm=1.0, g_loc=None), "odd_n", g_hm=1.0, g_loc=None)  # hm_loss alone: the maps' gradients are zero
    check(run(c, g_hm=None, g_loc=1.0), "odd_n", g_hm=None, g_loc=1.0)  # loc_loss alone: d_hm is zero
    got = run(c, frozen=(2,))
    assert got["d_maps"][2] is None
    check(got, "odd_n")
    double = dict(c, hm=c["hm"].astype(np.float64), maps=[m.astype(np.float64) for m in c["maps"]])
    got = run(double)  # other float dtypes are converted under autograd: the gradients come back in the inputs' dtype
    assert got["d_hm"].dtype == torch.float64 and got["d_maps"][0].dtype == torch.float64
    check(dict(got, d_hm=got["d_hm"].float(), d_maps=[g.float() for g in got["d_maps"]]), "odd_n")


def test_results_are_bit_identical_run_to_run_and_across_streams():
    t = upload_case(cases.make_case("with_vel"))
    first, second = compute(t), compute(t)
    torch.cuda.synchronize()
    outs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):  # both in flight together: each call owns its workspace
        with torch.cuda.stream(s):
            outs.append(compute(t, read_counts=False))
    torch.cuda.synchronize()
    for other in [second] + outs:
        for k in ("hm_loss", "loc_loss", "per_dim", "d_hm"):
            assert torch.equal(first[k], other[k]), k
        for a, b in zip(first["d_maps"], other["d_maps"]):
            assert torch.equal(a, b)


def _fused_step(golden_dir):
    d, head = _step(golden_dir, DEV)
    head.fused_loss = True
    return d, head


def test_module_with_fused_loss_matches_the_reference_run(golden_dir):
    d, head = _fused_step(golden_dir)
    loss, tb = head.get_loss()
    want_tb = json.loads(str(d["tb_json"]))
    assert loss.is_cuda and set(tb) == set(want_tb)
    assert abs(float(loss.detach()) - float(d["loss"])) <= 1e-5 * float(d["loss"])
    for k, v in want_tb.items():
        assert torch.is_tensor(tb[k]) and tb[k].is_cuda and tb[k].dim() == 0 and not tb[k].requires_grad, k
        assert abs(float(tb[k]) - v) <= 1e-5 * max(1.0, abs(v)), k
    loss.backward()
    n = 0
    for k, v in head.named_parameters():
        if "grad." + k in d.files:
            want = d["grad." + k]
            np.testing.assert_allclose(v.grad.cpu().numpy(), want, rtol=1e-4, atol=1e-5 * max(1.0, float(np.abs(want).max())), err_msg=k)
            n += 1
    assert n >= 30
    d, head = _step(golden_dir, DEV)  # the same step with the attribute at its default, within the same bounds
    assert head.fused_loss is False
    _check(d, head)


def test_training_step_with_fused_loss_never_synchronises_the_host(golden_dir):
    d, head = _fused_step(golden_dir)
    warm, _ = head.get_loss()  # the code weights reach the device here, once
    warm.backward()
    head.zero_grad()
    batch = dict(spatial_features_2d=torch.from_numpy(d["spatial_features_2d"]).to(DEV), batch_size=int(d["batch_size"]),
                 gt_boxes=torch.from_numpy(d["gt_boxes"]).to(DEV))
    torch.cuda.synchronize()
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
            head(batch)
            loss, tb = head.get_loss()
            loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not live:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not make .item() raise on this build")
    assert abs(float(loss) - float(d["loss"])) <= 1e-5 * float(d["loss"])
    assert all(torch.is_tensor(v) and v.is_cuda for v in tb.values())
    assert head.shared_conv[0].weight.grad is not None


def test_arguments():
    c = cases.make_case("tail_only")
    t = {k: torch.from_numpy(c[k]) for k in ("hm", "heatmap", "target_boxes", "inds", "masks", "code_weights")}
    maps = [torch.from_numpy(m) for m in c["maps"]]
    with pytest.raises(_lib.MssvtHipError, match="no CPU path"):
        center_loss(t["hm"], maps, t["heatmap"], t["target_boxes"], t["inds"], t["masks"], t["code_weights"], 0.25)
    with pytest.raises(_lib.MssvtHipError, match="no CPU path"):
        center_loss(t["hm"].to(DEV), [m.to(DEV) for m in maps], t["heatmap"].to(DEV), t["target_boxes"], t["inds"].to(DEV),
                    t["masks"].to(DEV), t["code_weights"], 0.25)
    lib = _lib.lib()
    limit_m, limit_d = center_head.CENTER_LOSS_MAX_OBJS, center_head.CENTER_LOSS_MAX_CODE
    assert lib.mssvt_center_loss_workspace_bytes(1, 1, 5, 3, limit_m, limit_d) > 0
    assert lib.mssvt_center_loss_workspace_bytes(1, 1, 5, 3, limit_m + 1, 8) <= 0
    assert lib.mssvt_center_loss_workspace_bytes(1, 1, 5, 3, 4, limit_d + 1) <= 0
    assert lib.mssvt_center_loss_workspace_bytes(2, 1, 32768, 32768, 4, 8) <= 0  # n = 2^31
    many = cases.generate(1, 1, 5, 3, limit_m + 1, 8)
    with pytest.raises(_lib.MssvtHipError, match="limits"):
        run(many)
    wide = cases.generate(1, 1, 5, 3, 4, limit_d + 1)
    with pytest.raises(_lib.MssvtHipError, match="limits"):
        run(wide)
    at_limit = cases.generate(1, 1, 5, 3, limit_m, 8, dup="all")  # the whole LDS table, every slot on one cell
    args = (at_limit["hm"], at_limit["heatmap"], at_limit["maps"], at_limit["target_boxes"], at_limit["inds"], at_limit["masks"],
            at_limit["code_weights"], at_limit["loc_weight"])
    got = run(at_limit)
    fwd = ref.forward(*args)
    assert_loss_close(got["loc_loss"], fwd["loc_loss"], "loc_loss")
    _, d_maps = ref.backward(*args, g_hm=G_HM, g_loc=G_LOC)
    for k, g in enumerate(got["d_maps"]):
        assert_grad_close(g, d_maps[k], "d_map%d" % k)
