"""Times DynamicVFE's training step ALONE, forward + backward, on the GPU: the default [64, 128] configuration on
mssvt_amd/synthetic.py scenes of 160k points at B = 1 and B = 2, on the same inputs and the same initial parameters, one JSON
line per batch size:
  (a) fused: ``vfe.fused_train = True`` (csrc/vfe_train.hip: grouping, augmentation and the two run reductions as HIP
      kernels, one host read per step, bit-identical gradients);
  (b) torch: the torch branch (``_forward_train``: mask compaction, torch.unique, index_add, scatter_reduce, [inv] gathers).
A step is forward, a weighted sum of the voxel features, backward.  Each figure is the median over REPEATS runs of CALLS steps
between two device events, after a warm-up; both paths wait for the host inside a step, so the figures are wall time of the
step as a training loop would see it.  The launches of one step (kernels and device copies / fills the profiler records) are
counted with torch.profiler in a run of their own, after the timing.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mssvt_amd import synthetic  # noqa: E402
from mssvt_amd.dynamic_vfe import DynamicVFE  # noqa: E402


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


def count_launches(fn):
    """device kernels and device memory operations of one call, or None where the profiler records none"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        events = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    except Exception as e:  # noqa: BLE001 -- the count is a side figure: the timing above stands without it
        print("profiler unavailable: %r" % (e,), file=sys.stderr)
        return None
    return len(events) or None


def make_step(fused, points, B, weight):
    torch.manual_seed(0)
    vfe = DynamicVFE(dict(NUM_FILTERS=[64, 128]), 5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE,
                     synthetic.POINT_CLOUD_RANGE).cuda().train()
    vfe.fused_train = fused
    params = list(vfe.parameters())

    def step():
        out = vfe(dict(points=points, batch_size=B))
        return out, torch.autograd.grad((out["voxel_features"] * weight[:out["voxel_features"].shape[0]]).sum(), params,
                                        allow_unused=True)

    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=160000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-torch", action="store_true")
    ap.add_argument("--skip-count", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_vfe_train.py measures on the GPU; none found")
    for B in (1, 2):
        points = torch.from_numpy(synthetic.make_batch_points(args.points, B, 0)).cuda()
        weight = torch.randn((points.shape[0], 128), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B))
        fused = make_step(True, points, B, weight)
        out, grads = fused()
        again, grads2 = fused()
        identical = torch.equal(out["voxel_features"], again["voxel_features"]) and all(
            torch.equal(a, b) for a, b in zip(grads, grads2) if a is not None)
        rec = dict(shape="B=%d points=%d voxels=%d filters=[64, 128]" % (B, points.shape[0], out["voxel_coords"].shape[0]),
                   calls=args.calls, repeats=args.repeats, fused_bit_identical=bool(identical),
                   fused_fwd_bwd_us=round(median_us(fused, args.calls, args.warmup, args.repeats), 1))
        if not args.skip_count:
            rec["fused_launches"] = count_launches(fused)
        if not args.skip_torch:
            plain = make_step(False, points, B, weight)
            ref, _ = plain()
            assert torch.equal(ref["voxel_coords"], out["voxel_coords"])
            err = float((ref["voxel_features"] - out["voxel_features"]).detach().abs().max())
            assert err <= 1e-4, err
            us = median_us(plain, args.calls, args.warmup, args.repeats)
            rec.update(torch_fwd_bwd_us=round(us, 1), ratio=round(us / rec["fused_fwd_bwd_us"], 2), max_feature_diff=err)
            if not args.skip_count:
                rec["torch_launches"] = count_launches(plain)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
