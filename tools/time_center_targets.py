"""Times CenterHead's target assignment on the GPU at mssvt.yaml's shape (B = 4, 3 classes in one head, a 470 x 470 map,
NUM_MAX_OBJS = 500) with 60 and 200 objects per sample, one JSON line per load:
  (a) the operator (csrc/center_targets.hip through CenterHead.assign_targets_device: one launch): device events around
      CALLS calls after a warm-up, and the bytes it writes over that time;
  (b) the host loop (CenterHead.assign_targets_host on the same device boxes: boxes to the host, one numpy patch and one
      torch.max per object, maps back to the device): wall clock between two device synchronisations, since it
      synchronises anyway.
The kernel's own time comes from a run of its own under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o center_targets -- python tools/time_center_targets.py --skip-host
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mssvt_amd.center_head import CenterHead  # noqa: E402
from mssvt_amd.config import DEFAULT_CFG, load_yaml  # noqa: E402

H = W = 470
B, M = 4, 500


def yaml_head():
    cfg = load_yaml(DEFAULT_CFG)
    pcr = np.array(cfg["DATA_CONFIG"]["POINT_CLOUD_RANGE"], dtype=np.float64)
    voxel = None
    for proc in cfg["DATA_CONFIG"]["DATA_PROCESSOR"]:
        if "VOXEL_SIZE" in proc:
            voxel = list(proc["VOXEL_SIZE"])
    classes = list(cfg["CLASS_NAMES"])
    grid = np.round((pcr[3:] - pcr[:3]) / np.array(voxel)).astype(np.int64)
    return CenterHead(cfg["MODEL"]["DENSE_HEAD"], 8, len(classes), classes, grid, pcr, voxel, predict_boxes_when_training=False)


def random_boxes(head, n, seed):
    """(B, M, 8): n objects per sample in the range, Waymo-like sizes, then padding rows (label 0) up to M."""
    rng = np.random.default_rng(seed)
    x, y = float(head.point_cloud_range[3]), float(head.point_cloud_range[4])
    gt = np.zeros((B, M, 8), np.float32)
    gt[:, :n, 0] = rng.uniform(-x, x, (B, n))
    gt[:, :n, 1] = rng.uniform(-y, y, (B, n))
    gt[:, :n, 2] = rng.uniform(-1, 2, (B, n))
    gt[:, :n, 3] = rng.uniform(0.5, 6.0, (B, n))
    gt[:, :n, 4] = rng.uniform(0.5, 2.5, (B, n))
    gt[:, :n, 5] = rng.uniform(1.0, 2.5, (B, n))
    gt[:, :n, 6] = rng.uniform(-np.pi, np.pi, (B, n))
    gt[:, :n, 7] = rng.integers(1, 4, (B, n))
    return gt


def timed_events(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls  # us per call


def timed_wall(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-calls", type=int, default=100)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_center_targets.py measures on the GPU; none found")
    head = yaml_head()
    for n in (60, 200):
        gt = torch.from_numpy(random_boxes(head, n, seed=n)).cuda()
        out = head.assign_targets_device(gt, (H, W))
        out_bytes = sum(out[k][0].numel() * out[k][0].element_size() for k in ("heatmaps", "target_boxes", "inds", "masks"))
        us = timed_events(lambda: head.assign_targets_device(gt, (H, W)), args.calls, args.warmup)
        rec = dict(objects_per_sample=n, shape="B=%d c=3 %dx%d M=%d" % (B, H, W, M), operator_us_per_call=round(us, 2),
                   calls=args.calls, written_bytes=out_bytes, written_GB_per_s=round(out_bytes / us * 1e-3, 1))
        if not args.skip_host:
            host = head.assign_targets_host(gt, (H, W))
            for k in ("inds", "masks"):
                assert torch.equal(host[k][0], out[k][0]), k
            assert float((host["heatmaps"][0] - out["heatmaps"][0]).abs().max()) <= 1.2e-7
            us_host = timed_wall(lambda: head.assign_targets_host(gt, (H, W)), args.host_calls, 3)
            rec.update(host_loop_us_per_call=round(us_host, 1), host_calls=args.host_calls, ratio=round(us_host / us, 1))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
