"""Times CenterHead's inference decode on the GPU at mssvt.yaml's shape (one head of 3 classes, a 470 x 470 map,
MAX_OBJ_PER_SAMPLE = 500, NMS 4096 -> 500 at 0.7) for B = 1 and 4 on two heat maps -- (i) about 100 planted peaks per
sample over a -6 background, (ii) the untrained head's near-constant map (hm bias -2.19: every cell just above SCORE_THRESH)
-- one JSON line per (map, B):
  (a) the padded path (CenterHead.generate_predicted_boxes_padded: csrc/center_decode.hip + csrc/nms_bev_batched.hip, no
      host synchronisation): device events around every call after a warm-up, the median of CALLS calls;
  (b) the list path (CenterHead.generate_predicted_boxes: torch.topk, gathers, boolean masks, one NMS per sample): wall
      clock between two device synchronisations, since it synchronises anyway.
The kernels' own times come from a run of its own under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o center_decode -- python tools/time_center_decode.py --skip-list
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
C = 3


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


def make_maps(kind, B, seed):
    """The maps of the one head: regression maps as an initialised head leaves them (small offsets, sizes around a car's),
    `kind` = "peaks" (about 100 objects per sample: a 3 x 3 bump each over a -6 background) or "untrained" (-2.19 + noise
    of the size a freshly initialised last convolution adds)."""
    rng = np.random.default_rng(seed)
    if kind == "peaks":
        hm = np.full((B, C, H, W), -6.0, np.float32) + rng.normal(0, 0.05, (B, C, H, W)).astype(np.float32)
        for b in range(B):
            for _ in range(100):
                c, y, x = int(rng.integers(0, C)), int(rng.integers(1, H - 1)), int(rng.integers(1, W - 1))
                hm[b, c, y - 1:y + 2, x - 1:x + 2] = rng.uniform(-1.0, 0.5)
                hm[b, c, y, x] = rng.uniform(1.0, 4.0)
    else:
        hm = np.full((B, C, H, W), -2.19, np.float32) + rng.normal(0, 1e-3, (B, C, H, W)).astype(np.float32)
    pd = dict(hm=hm, center=rng.uniform(0, 1, (B, 2, H, W)).astype(np.float32),
              center_z=rng.uniform(-1, 2, (B, 1, H, W)).astype(np.float32),
              dim=np.log(rng.uniform([3.5, 1.6, 1.4], [5.5, 2.2, 2.0], (B, H, W, 3))).transpose(0, 3, 1, 2).astype(np.float32),
              rot=rng.normal(0, 1, (B, 2, H, W)).astype(np.float32))
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in pd.items()}


def median_events(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(calls):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        pairs.append((t0, t1))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in pairs])) * 1e3  # us


def median_wall(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--list-calls", type=int, default=50)
    ap.add_argument("--skip-list", action="store_true")
    args = ap.parse_args()
    if args.calls < 50:
        raise SystemExit("--calls: the median is taken over at least 50 calls")
    if not torch.cuda.is_available():
        raise SystemExit("time_center_decode.py measures on the GPU; none found")
    head = yaml_head()
    for kind in ("peaks", "untrained"):
        for B in (1, 4):
            pd = make_maps(kind, B, seed=B)
            with torch.no_grad():
                padded = head.generate_predicted_boxes_padded(B, [pd])
                us = median_events(lambda: head.generate_predicted_boxes_padded(B, [pd]), args.calls, args.warmup)
                rec = dict(map=kind, shape="B=%d c=%d %dx%d K=500" % (B, C, H, W), boxes_per_sample=padded["num"].tolist(),
                           padded_us_per_call=round(us, 1), calls=args.calls)
                if not args.skip_list:
                    listed = head.generate_predicted_boxes(B, [pd])
                    rec["list_boxes_per_sample"] = [int(d["pred_boxes"].shape[0]) for d in listed]
                    us_list = median_wall(lambda: head.generate_predicted_boxes(B, [pd]), args.list_calls, 3)
                    rec.update(list_us_per_call=round(us_list, 1), list_calls=args.list_calls, ratio=round(us_list / us, 1))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
