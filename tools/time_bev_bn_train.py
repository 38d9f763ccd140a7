#!/usr/bin/env python3
"""BatchNorm2d + ReLU in TRAINING mode, library (torch modules, autograd) against ``bn_train.BnReluFunction``
(csrc/bn_train.hip), at the shapes of mssvt.yaml (470 x 470 BEV grid, B = 1 and 4):

  * forward + backward of one BatchNorm + ReLU at (C, H) = (128, 470), (256, 235), (256, 470) -- the library on NCHW tensors
    (what the modules run without fused_train) and on channels-last tensors (what they run with it), the Function on
    channels-last tensors;
  * the whole map_to_bev_module + backbone_2d training step (forward + backward) with fused_train on, against fused_train +
    fused_bn with exactly the widths routed that cleared the rule (if none did: with every covered width routed, so that the
    figure exists, and the record says so).

One process; library and kernels alternate in it; every figure is a device-event time around a warmed-up window of several
steps; every run is written out, not a median.  Every GPU step (one shape at one batch size, one stage) runs under its own
time limit: an alarm whose default action ends the process, so nothing more is started on the GPU after a step that hangs;
the results so far are on disk.  Routing rule: a width is routed only where the Function's SLOWEST run beats the
library's FASTEST (over both layouts) at every timed shape of that width and at every batch size;
mssvt_amd/bn_train.py::ROUTED_BN must name exactly those.

    python tools/time_bev_bn_train.py [--runs 5] [--out profiles/bev_bn_train_times.json]
"""
import argparse
import json
import os
import signal
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mssvt_amd import bn_train, config  # noqa: E402
from mssvt_amd.base_bev_backbone import BaseBEVBackbone  # noqa: E402
from mssvt_amd.height_compression import HeightCompression  # noqa: E402
from mssvt_amd.mssvt_utils import SparseTensor  # noqa: E402

DEV = "cuda"
GRID = 470
# (channels, input size, layers of this shape per frame in mssvt.yaml)
LAYERS = [(128, GRID, 9), (256, GRID // 2, 6), (256, GRID, 2)]
STEP_LIMIT_S = 240


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, runs, iters):
    """{name: [ms per step, one per run]}: warm up all, then one window each, in turn, `runs` times."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            out[k].append(window_ms(fn, iters))
    return out


def limited(fn, *args):
    """`fn(*args)` under STEP_LIMIT_S: the alarm's default action ends the process."""
    signal.alarm(STEP_LIMIT_S)
    try:
        return fn(*args)
    finally:
        signal.alarm(0)


def layer_times(shape, B, runs):
    C, size, per_frame = shape
    torch.manual_seed(C + size + B)
    bn = nn.BatchNorm2d(C, eps=1e-3, momentum=0.01).to(DEV).train()
    relu = nn.ReLU()
    x = torch.randn(B, C, size, size, device=DEV).requires_grad_(True)
    xl = x.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    g = torch.randn(B, C, size, size, device=DEV)
    gl = g.contiguous(memory_format=torch.channels_last)

    def step(fwd, inp, grad):
        inp.grad = bn.weight.grad = bn.bias.grad = None
        fwd(inp).backward(grad)

    lib = lambda t: relu(bn(t))  # noqa: E731
    hip = lambda t: bn_train.bn_relu(bn, t, True)  # noqa: E731
    step(lib, xl, gl)
    dx_lib, dw_lib = xl.grad.clone(), bn.weight.grad.clone()
    step(hip, xl, gl)
    diff = dict(dx=float((xl.grad - dx_lib).abs().max() / dx_lib.abs().max()),
                dgamma=float((bn.weight.grad - dw_lib).abs().max() / dw_lib.abs().max()))
    nbytes = 4.0 * B * C * size * size
    t = alternate({"library_nchw": lambda: step(lib, x, g), "library_nhwc": lambda: step(lib, xl, gl),
                   "hip": lambda: step(hip, xl, gl)}, runs, max(3, int(4e9 / nbytes)))
    lib_best = min(t["library_nchw"] + t["library_nhwc"])
    rec = dict(C=C, B=B, H=size, W=size, layers_per_frame=per_frame, tensor_bytes=nbytes, ms=t, relative_difference_to_library=diff,
               hip_slowest_ms=max(t["hip"]), library_fastest_ms=lib_best, cleared=max(t["hip"]) < lib_best,
               hip_tensor_passes_per_second_tb=8 * nbytes / (min(t["hip"]) * 1e-3) / 1e12)
    print("C %3d B%d %dx%d fwd+bwd: hip %.3f..%.3f ms | library nchw %.3f..%.3f, nhwc %.3f..%.3f ms %s" % (
        C, B, size, size, min(t["hip"]), max(t["hip"]), min(t["library_nchw"]), max(t["library_nchw"]),
        min(t["library_nhwc"]), max(t["library_nhwc"]), "CLEARED" if rec["cleared"] else "not cleared"), flush=True)
    return rec


def stage_times(B, runs, routed):
    cfg = config.load_yaml(config.DEFAULT_CFG)
    torch.manual_seed(1)
    hc = HeightCompression(cfg.MODEL.MAP_TO_BEV).to(DEV).train()
    bev = BaseBEVBackbone(cfg.MODEL.BACKBONE_2D, hc.num_bev_features).to(DEV).train()
    hc.fused_train = bev.fused_train = True
    g = torch.Generator().manual_seed(B)
    rows = []
    for b in range(B):
        cells = torch.randperm(GRID * GRID, generator=g)[:36000].sort().values  # ~1/6 of the cells, as a Waymo frame leaves
        rows.append(torch.stack([torch.full_like(cells, b), torch.zeros_like(cells), cells % GRID, cells // GRID], dim=1))
    vc = torch.cat(rows).int().to(DEV)
    feats = torch.randn(vc.shape[0], 128, device=DEV)
    sp = SparseTensor(features=feats, indices=vc, spatial_shape=[GRID, GRID, 1], voxel_size=[0.32, 0.32, 6.0],
                      point_cloud_range=[-75.2, -75.2, -2, 75.2, 75.2, 4], batch_size=B, hash_size=400009)
    grad = torch.randn(B, bev.num_bev_features, GRID, GRID, device=DEV) * 1e-3
    params = list(hc.parameters()) + list(bev.parameters())

    def run(on):
        hc.fused_bn = bev.fused_bn = on
        for p in params:
            p.grad = None
        sp.features = feats.clone().requires_grad_(True)
        out = bev(hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1)))["spatial_features_2d"]
        out.backward(grad)
        return out.detach(), [p.grad for p in params]

    keep = bn_train.ROUTED_BN
    bn_train.ROUTED_BN = frozenset(routed)
    try:
        (y1, g1), (y0, g0) = run(True), run(False)
        diff = dict(output=float((y1 - y0).abs().max() / y0.abs().max()),
                    gradients=max(float((a - b).abs().max() / b.abs().max().clamp_(min=1e-30)) for a, b in zip(g1, g0)))
        del y1, g1, y0, g0
        t = alternate({"fused_train": lambda: run(False), "fused_train_fused_bn": lambda: run(True)}, runs, 3)
    finally:
        bn_train.ROUTED_BN = keep
    print("stage B%d fwd+bwd: fused_train %.2f..%.2f ms, fused_train + fused_bn %.2f..%.2f ms (relative difference: output %.2e, gradients %.2e)" % (
        B, min(t["fused_train"]), max(t["fused_train"]), min(t["fused_train_fused_bn"]), max(t["fused_train_fused_bn"]),
        diff["output"], diff["gradients"]), flush=True)
    return dict(B=B, ms=t, relative_difference=diff, routed_in_this_measurement=sorted(routed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev_bn_train_times.json"))
    args = ap.parse_args()
    assert args.runs >= 5, "at least five runs each"
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, runs=args.runs, grid=GRID, layers=[], stages=[],
               routed_in_package=sorted(bn_train.ROUTED_BN))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)

    for s in LAYERS:
        for B in (1, 4):
            out["layers"].append(limited(layer_times, s, B, args.runs))
            save()
    routed = sorted({r["C"] for r in out["layers"]} - {r["C"] for r in out["layers"] if not r["cleared"]})
    out["routed"] = routed
    save()
    for B in (1, 4):
        out["stages"].append(limited(stage_times, B, args.runs, routed or bn_train.CHANNELS))
        save()
    print("routed (cleared at every shape of the width, B = 1 and B = 4): %s -> %s" % (routed, args.out))


if __name__ == "__main__":
    main()
