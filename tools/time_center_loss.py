"""Times CenterHead's loss ALONE, forward + backward, on the GPU at mssvt.yaml's head shape (3 classes in one head, a
470 x 470 map, NUM_MAX_OBJS = 500, 8 code dimensions) at B = 1 and 4, on the same inputs, one JSON line per batch size:
  (a) fused: ``center_head.center_loss`` (csrc/center_loss.hip: two launches forward, three backward, nothing read back);
  (b) unfused: the expressions of ``CenterHead.get_loss`` (clamped sigmoid, ``centernet_focal_loss`` with its Python branch
      on num_pos, the concatenated maps through ``centernet_reg_loss``, the weighted sum) under autograd, without the
      ``.item()`` calls that follow them in ``get_loss``.
The targets are real ones (``CenterHead.assign_targets_device`` on random boxes), the predictions random maps that require
gradients.  Each figure is the median over REPEATS runs of CALLS calls between two device events, after a warm-up.  The
fused forward alone is timed too and set against its byte floor, 8 n bytes (logits + targets, each read once).
The kernels' own times come from a run of its own under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o center_loss -- python tools/time_center_loss.py --skip-unfused
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mssvt_amd.center_head import _get, center_loss, centernet_focal_loss, centernet_reg_loss  # noqa: E402
from time_center_targets import H, W, M, random_boxes, yaml_head  # noqa: E402


def median_us(fn, calls, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        runs.append(t0.elapsed_time(t1) * 1e3 / calls)
    return statistics.median(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--objects", type=int, default=200)
    ap.add_argument("--skip-unfused", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_center_loss.py measures on the GPU; none found")
    head = yaml_head()
    weights = _get(_get(head.model_cfg, "LOSS_CONFIG"), "LOSS_WEIGHTS")
    order = list(_get(head.separate_head_cfg, "HEAD_ORDER"))
    channels = {k: int(v["out_channels"]) for k, v in dict(_get(head.separate_head_cfg, "HEAD_DICT")).items()}
    code_weights = torch.tensor([float(v) for v in weights["code_weights"]], dtype=torch.float32, device="cuda")
    loc_weight = float(weights["loc_weight"])
    gt_all = torch.from_numpy(random_boxes(head, args.objects, seed=args.objects)).cuda()
    for B in (1, 4):
        td = head.assign_targets_device(gt_all[:B].contiguous(), (H, W))
        heatmap, target_boxes, inds, masks = (td[k][0] for k in ("heatmaps", "target_boxes", "inds", "masks"))
        C = heatmap.shape[1]
        gen = torch.Generator(device="cuda").manual_seed(B)
        hm = (torch.randn((B, C, H, W), device="cuda", generator=gen) - 2.19).requires_grad_()
        maps = [torch.randn((B, channels[k], H, W), device="cuda", generator=gen).requires_grad_() for k in order]
        leaves = [hm] + maps

        def fused_forward():
            return center_loss(hm, maps, heatmap, target_boxes, inds, masks, code_weights, loc_weight)

        def fused():
            hm_loss, loc_loss, _ = fused_forward()
            return torch.autograd.grad(hm_loss + loc_loss, leaves)

        def unfused_forward():
            pred = torch.clamp(hm.sigmoid(), min=1e-4, max=1 - 1e-4)
            hm_loss = centernet_focal_loss(pred, heatmap)
            reg = centernet_reg_loss(torch.cat(maps, dim=1), masks, inds, target_boxes)
            return hm_loss, (reg * reg.new_tensor(list(weights["code_weights"]))).sum() * loc_weight

        def unfused():
            hm_loss, loc_loss = unfused_forward()
            return torch.autograd.grad(hm_loss + loc_loss, leaves)

        n = hm.numel()
        us_fwd = median_us(fused_forward, args.calls, args.warmup, args.repeats)
        us = median_us(fused, args.calls, args.warmup, args.repeats)
        rec = dict(shape="B=%d c=%d %dx%d M=%d D=%d" % (B, C, H, W, M, sum(channels[k] for k in order)),
                   objects_per_sample=args.objects, calls=args.calls, repeats=args.repeats,
                   fused_fwd_bwd_us=round(us, 1), fused_fwd_us=round(us_fwd, 1), fwd_floor_bytes=8 * n,
                   fwd_floor_GB_per_s=round(8 * n / us_fwd * 1e-3, 1))
        if not args.skip_unfused:
            a, b = [v.detach() for v in fused_forward()], [v.detach() for v in unfused_forward()]
            assert abs(float(a[0]) - float(b[0])) <= 1e-4 * abs(float(b[0])) and abs(float(a[1]) - float(b[1])) <= 1e-4 * abs(float(b[1]))
            us_old = median_us(unfused, args.calls, args.warmup, args.repeats)
            us_old_fwd = median_us(unfused_forward, args.calls, args.warmup, args.repeats)
            rec.update(unfused_fwd_bwd_us=round(us_old, 1), unfused_fwd_us=round(us_old_fwd, 1), ratio=round(us_old / us, 2))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
