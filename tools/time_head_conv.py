#!/usr/bin/env python3
"""CenterHead's convolutions in eval mode, library (MIOpen through torch) against csrc/head_conv.hip, at the head shape of
mssvt.yaml (512 -> 64 shared layer, five branches 64 -> 64 -> {2, 1, 3, 2, 3}) on the 470 x 470 map, B = 1 and 4:

  * per stage -- shared, trunk (the first Conv + BN + ReLU of the five branches), finals (their last convolutions) -- the library
    as the module runs it (Conv, BatchNorm and ReLU as separate launches) on NCHW and on channels-last tensors, and the kernel
    with its exponent pass; for the shared layer also the kernel behind the one layout conversion the switch causes when the
    features arrive NCHW (backbone switch off);
  * the whole head (all eleven convolutions, no decoding) with fused_convs off and on, on NCHW and on channels-last features.

Library and kernels alternate in the same process; every figure is a device-event time around a warmed-up window of several
launches; every run is written out, not a median.  Routing rule: a stage is routed only where the kernel's SLOWEST
run beats the library's FASTEST (over both layouts) at every batch size.  The shared layer is judged twice: on channels-last
features (no conversion) and behind the conversion of NCHW features; where only the first clears the rule the module takes
the kernel for channels-last features only (head_conv.SHARED_FROM_NCHW).  The whole head is measured with exactly those
stages routed, and mssvt_amd/head_conv.py::ROUTED / SHARED_FROM_NCHW must name them.

    python tools/time_head_conv.py [--runs 5] [--out profiles/head_conv_times.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mssvt_amd import centerpoint, config, head_conv  # noqa: E402
from mssvt_amd.center_head import CenterHead  # noqa: E402

DEV = "cuda"
GRID = 470


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, runs, iters):
    """{name: [ms per call, one per run]}: warm up all, then one window each, in turn, `runs` times."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            out[k].append(window_ms(fn, iters))
    return out


def build_head():
    cfg = config.load_yaml(config.DEFAULT_CFG)
    torch.manual_seed(1)
    info = centerpoint.dataset_info(cfg)
    head = CenterHead(cfg.MODEL.DENSE_HEAD, 512, len(info.class_names), info.class_names, info.grid_size, info.point_cloud_range,
                      info.voxel_size, predict_boxes_when_training=False)
    with torch.no_grad():
        for mod in head.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
    return head.to(DEV).eval()


def record(stage, B, cin, cout, t, hip_keys):
    flop = 2.0 * B * GRID * GRID * cout * cin * 9
    lib_best = min(t["library_nchw"] + t["library_nhwc"])
    hip_worst = max(v for k in hip_keys for v in t[k])
    rec = dict(stage=stage, B=B, H=GRID, W=GRID, cin=cin, cout=cout, flop=flop, ms=t,
               tflops={n: [flop / (v * 1e-3) / 1e12 for v in vs] for n, vs in t.items()},
               hip_slowest_ms=hip_worst, library_fastest_ms=lib_best, cleared=hip_worst < lib_best)
    print("%-6s B%d: hip %s | library nchw %.3f..%.3f, nhwc %.3f..%.3f ms (%.0f TFLOP/s) %s" % (
        stage, B, ", ".join("%s %.3f..%.3f ms (%.0f TFLOP/s)" % (k, min(t[k]), max(t[k]), flop / min(t[k]) / 1e9) for k in hip_keys),
        min(t["library_nchw"]), max(t["library_nchw"]), min(t["library_nhwc"]), max(t["library_nhwc"]), flop / lib_best / 1e9,
        "CLEARED" if rec["cleared"] else "not cleared"), flush=True)
    return rec


def stage_times(head, B, runs):
    shared, trunk, finals = head_conv.layers(head)
    packs = head_conv.pack(head)
    s, nb = packs["trunk"].s, packs["trunk"].nb
    seqs = [seq for _, _, seq in head_conv.branches(head)]
    out = []
    with torch.no_grad():
        x = torch.randn(B, 512, GRID, GRID, device=DEV).clamp_(min=0)
        xl = x.contiguous(memory_format=torch.channels_last)
        rows = xl.permute(0, 2, 3, 1)
        t = alternate({"library_nchw": lambda: head.shared_conv(x), "library_nhwc": lambda: head.shared_conv(xl),
                       "hip": lambda: head_conv.run_shared(packs["shared"], rows),
                       "hip_from_nchw": lambda: head_conv.run_shared(
                           packs["shared"], x.contiguous(memory_format=torch.channels_last).permute(0, 2, 3, 1))}, runs, 5)
        rec = record("shared", B, 512, s, t, ["hip"])
        rec["cleared_from_nchw"] = max(t["hip_from_nchw"]) < rec["library_fastest_ms"]
        print("       behind the conversion of NCHW features: %.3f..%.3f ms, %s" % (
            min(t["hip_from_nchw"]), max(t["hip_from_nchw"]), "CLEARED" if rec["cleared_from_nchw"] else "not cleared"), flush=True)
        out.append(rec)
        y, e = head_conv.run_shared(packs["shared"], rows)
        del x, xl, rows
        yl = y.permute(0, 3, 1, 2)  # channels-last in memory
        yc = yl.contiguous()
        t = alternate({"library_nchw": lambda: [q[0](yc) for q in seqs], "library_nhwc": lambda: [q[0](yl) for q in seqs],
                       "hip": lambda: head_conv.run_trunk(packs["trunk"], y, e)}, runs, 5)
        out.append(record("trunk", B, s, nb * s, t, ["hip"]))
        tt, e2 = head_conv.run_trunk(packs["trunk"], y, e)
        tv = tt.permute(0, 3, 1, 2)
        parts_l = [tv[:, b * s:(b + 1) * s].contiguous(memory_format=torch.channels_last) for b in range(nb)]
        parts_c = [p.contiguous() for p in parts_l]
        t = alternate({"library_nchw": lambda: [c(p) for c, p in zip(finals, parts_c)],
                       "library_nhwc": lambda: [c(p) for c, p in zip(finals, parts_l)],
                       "hip": lambda: head_conv.run_finals(packs["finals"], tt, e2)}, runs, 10)
        out.append(record("finals", B, s, sum(packs["finals"].ks), t, ["hip"]))
    return out


def head_times(head, B, runs, routed, from_nchw):
    def library(v):
        y = head.shared_conv(v)
        return [sep(y) for sep in head.heads_list]

    keep = head_conv.ROUTED, head_conv.SHARED_FROM_NCHW
    head_conv.ROUTED, head_conv.SHARED_FROM_NCHW = frozenset(routed), from_nchw
    try:
        with torch.no_grad():
            x = torch.randn(B, 512, GRID, GRID, device=DEV).clamp_(min=0)
            xl = x.contiguous(memory_format=torch.channels_last)
            on, off = head_conv.forward(head, xl), library(x)
            diff = max(float((p[k] - q[k]).abs().max()) for p, q in zip(on, off) for k in q)
            t = alternate({"library_nchw": lambda: library(x), "library_nhwc": lambda: library(xl),
                           "fused_convs_nchw": lambda: head_conv.forward(head, x),
                           "fused_convs_nhwc": lambda: head_conv.forward(head, xl)}, runs, 3)
    finally:
        head_conv.ROUTED, head_conv.SHARED_FROM_NCHW = keep
    print("head B%d: library nchw %.2f..%.2f, nhwc %.2f..%.2f ms | fused_convs from nchw %.2f..%.2f, from nhwc %.2f..%.2f ms "
          "(max |difference| %.2e)" % (B, min(t["library_nchw"]), max(t["library_nchw"]), min(t["library_nhwc"]),
                                       max(t["library_nhwc"]), min(t["fused_convs_nchw"]), max(t["fused_convs_nchw"]),
                                       min(t["fused_convs_nhwc"]), max(t["fused_convs_nhwc"]), diff), flush=True)
    return dict(B=B, ms=t, max_abs_difference=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_conv_times.json"))
    args = ap.parse_args()
    assert args.runs >= 5, "at least five runs each"
    head = build_head()
    assert head_conv.supported(head)
    stages = [r for B in (1, 4) for r in stage_times(head, B, args.runs)]
    routed = [s for s in head_conv.STAGES if all(r["cleared"] for r in stages if r["stage"] == s)]
    from_nchw = "shared" in routed and all(r["cleared_from_nchw"] for r in stages if r["stage"] == "shared")
    heads = [head_times(head, B, args.runs, routed, from_nchw) for B in (1, 4)]
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, runs=args.runs, grid=GRID, stages=stages,
               routed=routed, shared_from_nchw=from_nchw, routed_in_package=[s for s in head_conv.STAGES if s in head_conv.ROUTED],
               shared_from_nchw_in_package=head_conv.SHARED_FROM_NCHW, heads=heads)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("routed (cleared at B = 1 and B = 4): %s, shared layer behind a layout conversion: %s -> %s" % (routed, from_nchw, args.out))


if __name__ == "__main__":
    main()
