"""The numpy float64 statement of CenterHead's loss (tests/center_loss_ref.py) against what is already pinned: torch autograd
in float64 over ``centernet_focal_loss`` / ``centernet_reg_loss`` with the clamp bounds float32 sees, and the reference's
own training step (tests/golden/det_head_train.npz); and every generated input of tests/test_center_loss_gpu.py
(tests/center_loss_cases.py) against the conditions its bounds rest on."""
import json

import numpy as np
import pytest
import torch

from mssvt_amd.center_head import centernet_focal_loss, centernet_reg_loss
from tests import center_loss_cases as cases
from tests import center_loss_ref as ref
from tests.test_head_train_cpu import _step

# the torch expressions gather every slot: cases with an index outside the map or NaN targets are the reference's own ground
TORCH_CASES = ["one_cell", "tail_only", "odd_n", "with_vel", "no_positives", "no_objects", "one_empty_sample", "two_on_a_cell",
               "three_on_a_cell", "all_on_a_cell"]


def _args(c):
    return (c["hm"], c["heatmap"], c["maps"], c["target_boxes"], c["inds"], c["masks"], c["code_weights"], c["loc_weight"])


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max()) / max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("name", TORCH_CASES)
def test_reference_matches_torch_autograd_in_float64(name):
    c = cases.make_case(name)
    D = sum(m.shape[1] for m in c["maps"])
    hm = torch.from_numpy(c["hm"]).double().requires_grad_()
    maps = [torch.from_numpy(m).double().requires_grad_() for m in c["maps"]]
    pred = torch.clamp(hm.sigmoid(), min=float(ref.LO), max=float(ref.HI))  # the bounds float32 sees, as doubles
    hm_loss = centernet_focal_loss(pred, torch.from_numpy(c["heatmap"]).double())
    per_dim = centernet_reg_loss(torch.cat(maps, dim=1), torch.from_numpy(c["masks"]), torch.from_numpy(c["inds"]),
                                 torch.from_numpy(c["target_boxes"][:, :, :D]).double())
    loc_loss = (per_dim * torch.from_numpy(c["code_weights"]).double()).sum() * c["loc_weight"]
    (3.0 * hm_loss + 0.5 * loc_loss).backward()
    fwd = ref.forward(*_args(c))
    d_hm, d_maps = ref.backward(*_args(c), g_hm=3.0, g_loc=0.5)
    assert _rel(fwd["hm_loss"], hm_loss.item()) <= 1e-12
    assert _rel(fwd["loc_loss"], loc_loss.item()) <= 1e-12
    assert _rel(fwd["per_dim"], per_dim.detach().numpy()) <= 1e-12
    assert fwd["num_pos"] == int((c["heatmap"] == 1).sum()) and fwd["num"] == int(c["masks"].sum())
    assert _rel(d_hm, hm.grad.numpy()) <= 1e-12
    for k, m in enumerate(maps):
        assert _rel(d_maps[k], m.grad.numpy()) <= 1e-12, k


def test_double_clamp_constants_would_miss_float32_by_more_than_the_rounding():
    """why the reference clamps at np.float32 bounds: on an all-saturated map the double constants move the loss by
    ~1.8e-5 relative, more than the 1e-5 the GPU test allows"""
    hm = np.full((1, 1, 4, 4), 30.0, np.float32)
    gt = np.zeros((1, 1, 4, 4), np.float32)
    with_f32 = -16 * np.log(1.0 - np.float64(ref.HI)) * np.float64(ref.HI) ** 2
    with_f64 = -16 * np.log(1.0 - (1 - 1e-4)) * (1 - 1e-4) ** 2
    maps = [np.zeros((1, 1, 4, 4), np.float32)]
    fwd = ref.forward(hm, gt, maps, np.zeros((1, 1, 2), np.float32), np.zeros((1, 1), np.int64), np.zeros((1, 1), np.int64), [1.0], 1.0)
    assert abs(fwd["hm_loss"] - with_f32) <= 1e-12 * with_f32
    assert 1e-5 < abs(with_f64 - with_f32) / with_f32 < 3e-5


def test_poisoned_slots_are_skipped_by_the_reference():
    c = cases.make_case("poisoned_slots")
    fwd = ref.forward(*_args(c))
    d_hm, d_maps = ref.backward(*_args(c))
    assert np.isfinite(fwd["loc_loss"]) and np.isfinite(fwd["per_dim"]).all() and all(np.isfinite(g).all() for g in d_maps)
    assert fwd["num"] == int(c["masks"].sum())
    clean = dict(c, masks=c["masks"].copy())
    clean["masks"][:, 2] = 0  # without the slots outside the map: the same sums over one object less per sample
    clean["inds"] = np.where(clean["masks"] != 0, c["inds"], 0)
    clean["target_boxes"] = np.nan_to_num(c["target_boxes"])
    want = ref.forward(*_args(clean))
    assert want["num"] == fwd["num"] - 2
    np.testing.assert_allclose(fwd["per_dim"] * fwd["num"], want["per_dim"] * want["num"], rtol=1e-13)


def test_reference_reproduces_the_reference_run(golden_dir):
    """the statement on the CPU head's own predictions against the loss terms of the reference's training step"""
    d, head = _step(golden_dir, "cpu")
    cfg = json.loads(str(d["cfg_json"]))
    weights = cfg["HEAD"]["LOSS_CONFIG"]["LOSS_WEIGHTS"]
    order = list(cfg["HEAD"]["SEPARATE_HEAD_CFG"]["HEAD_ORDER"])
    want_tb = json.loads(str(d["tb_json"]))
    td = head.forward_ret_dict["target_dicts"]
    total = 0.0
    for idx, pd in enumerate(head.forward_ret_dict["pred_dicts"]):
        fwd = ref.forward(pd["hm"].detach().numpy(), td["heatmaps"][idx].numpy(), [pd[k].detach().numpy() for k in order],
                          td["target_boxes"][idx].numpy(), td["inds"][idx].numpy(), td["masks"][idx].numpy(),
                          weights["code_weights"], weights["loc_weight"])
        for key, got in (("hm_loss_head_%d" % idx, fwd["hm_loss"]), ("loc_loss_head_%d" % idx, fwd["loc_loss"])):
            assert abs(got - want_tb[key]) <= 1e-5 * max(1.0, abs(want_tb[key])), key
        total += fwd["hm_loss"] + fwd["loc_loss"]
    assert abs(total - float(d["loss"])) <= 1e-5 * float(d["loss"])
    assert abs(total - want_tb["rpn_loss"]) <= 1e-5 * max(1.0, abs(want_tb["rpn_loss"]))


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_generated_inputs_stay_clear_of_the_clamp_edges(name):
    c = cases.make_case(name)
    a = np.abs(c["hm"])
    assert not ((a > 9.0) & (a < 9.5)).any()
    assert (a >= 9.5).mean() <= 0.02
    (B, C, H, W, M, D), _ = cases.CASES[name]
    assert c["hm"].shape == c["heatmap"].shape == (B, C, H, W) and c["target_boxes"].shape == (B, M, D + 1)
    assert sum(m.shape[1] for m in c["maps"]) == D and float(c["heatmap"].max()) <= 1.0
    edges = np.log(np.float64(ref.LO) / (1 - np.float64(ref.LO))), np.log(np.float64(ref.HI) / (1 - np.float64(ref.HI)))
    assert -9.5 < edges[0] < -9.0 and 9.0 < edges[1] < 9.5
