"""Times the pairwise box operators (csrc/box_iou.hip) on the GPU: device events around CALLS launches after a warm-up,
one JSON line per shape.  Kernel times come from a run of its own under the profiler:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o box_iou -- python tools/time_box_iou.py

Each shape uses another instantiation of k_box_pairs, so the kernel statistics keep them apart:
  (a) 500 x 200, 3-D IoU        -- the recall bookkeeping call of CenterPoint.post_processing   -> k_box_pairs<2>
  (b) 4096 x 4096, BEV IoU      -- NMS_PRE_MAXSIZE boxes against themselves, next to nms_gpu on the same boxes
                                   (k_nms_mask evaluates the strict upper triangle of these pairs)  -> k_box_pairs<1>
  (c) 212 064 anchors x 128, BEV overlap -- what an anchor target assigner asks for              -> k_box_pairs<0>
For (c) the share of (row, 64-column tile) wavefront-rows whose every pair fails the kernel's rejection test (and so skip
rect_overlap) is computed on the host from the same float32 expression.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mssvt_amd import iou3d_nms_utils as u  # noqa: E402


def random_boxes(n, seed, spread, dup=True):
    rng = np.random.default_rng(seed)
    b = np.zeros((n, 7), np.float32)
    b[:, 0:2] = rng.uniform(-spread, spread, (n, 2))
    b[:, 2] = rng.uniform(-1, 1, n)
    b[:, 3] = rng.uniform(1.5, 5.0, n)
    b[:, 4] = rng.uniform(0.8, 2.5, n)
    b[:, 5] = rng.uniform(1.0, 2.0, n)
    b[:, 6] = rng.uniform(-np.pi, np.pi, n)
    if dup:  # near duplicates, as the NMS tests make them
        q = n // 4
        b[q:2 * q] = b[:q] + rng.normal(0, 0.15, (q, 7)).astype(np.float32)
    return b, rng.uniform(0.1, 1.0, n).astype(np.float32)


def anchor_boxes():
    c = ((np.arange(188) + 0.5) * 0.8 - 75.2).astype(np.float32)
    out = np.zeros((3, 2, 188, 188, 7), np.float32)
    out[..., 0] = c[None, None, :, None]
    out[..., 1] = c[None, None, None, :]
    for s, size in enumerate([[4.7, 2.1, 1.7], [0.91, 0.86, 1.73], [1.78, 0.84, 1.78]]):
        out[s, ..., 3:6] = np.array(size, np.float32)
    out[:, 1, ..., 6] = np.float32(np.pi / 2)
    return out.reshape(-1, 7)


def skipped_wave_rows(a, b):
    """Share of (row, 64-column tile) pairs of the launch in which no lane passes the kernel's rejection test."""
    f = np.float32
    ra = f(0.5) * np.sqrt(a[:, 3] * a[:, 3] + a[:, 4] * a[:, 4]) + f(0.02)
    rb = f(0.5) * np.sqrt(b[:, 3] * b[:, 3] + b[:, 4] * b[:, 4]) + f(0.02)
    tiles = -(-b.shape[0] // 64)
    live = np.zeros((a.shape[0], tiles), bool)
    for t in range(tiles):
        bt, rt = b[t * 64:(t + 1) * 64], rb[t * 64:(t + 1) * 64]
        dx, dy = a[:, None, 0] - bt[None, :, 0], a[:, None, 1] - bt[None, :, 1]
        reach = ra[:, None] + rt[None, :]
        live[:, t] = (~(dx * dx + dy * dy > reach * reach)).any(axis=1)
    return 1.0 - float(live.mean())


def timed(fn, calls, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shapes", default="abc")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_box_iou.py measures on the GPU; none found")
    dev = "cuda"
    if "a" in args.shapes:
        a, b = random_boxes(500, 1, 75.0)[0], random_boxes(200, 2, 75.0)[0]
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        us = timed(lambda: u.boxes_iou3d_gpu(ta, tb), args.calls, args.warmup)
        print(json.dumps(dict(shape="a", what="boxes_iou3d_gpu 500 x 200", us_per_call=round(us, 2), calls=args.calls)))
    if "b" in args.shapes:
        bx, sc = random_boxes(4096, 9, 75.0)
        tb, ts = torch.from_numpy(bx).to(dev), torch.from_numpy(sc).to(dev)
        us = timed(lambda: u.boxes_iou_bev(tb, tb), args.calls, args.warmup)
        us_nms = timed(lambda: u.nms_gpu(tb, ts, 0.7), args.calls, args.warmup)
        print(json.dumps(dict(shape="b", what="boxes_iou_bev 4096 x 4096", us_per_call=round(us, 2), calls=args.calls,
                              out_bytes=4096 * 4096 * 4, nms_gpu_us_per_call=round(us_nms, 2))))
    if "c" in args.shapes:
        a, b = anchor_boxes(), random_boxes(128, 5, 75.0, dup=False)[0]
        ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        us = timed(lambda: u.boxes_overlap_bev(ta, tb), args.calls, args.warmup)
        print(json.dumps(dict(shape="c", what="boxes_overlap_bev 212064 x 128", us_per_call=round(us, 2), calls=args.calls,
                              out_bytes=a.shape[0] * 128 * 4, wave_rows_skipping_rect_overlap=round(skipped_wave_rows(a, b), 5))))


if __name__ == "__main__":
    main()
