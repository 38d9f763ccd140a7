#!/usr/bin/env python3
"""The dense BEV part of the detector in eval mode, library (MIOpen through torch) against csrc/bev_conv.hip, at the shapes of
mssvt.yaml (470 x 470 BEV grid, B = 1 and 4):

  * every covered layer shape as Conv + BatchNorm + ReLU -- the library on NCHW tensors (what the modules run today) and on
    channels-last tensors, the kernel through bev_conv.conv_bn_act;
  * the whole map_to_bev_module + backbone_2d pass with fused_convs off and on.

Library and kernel alternate in the same process; every figure is a device-event time around a warmed-up window of several
launches; every run is written out, not a median.  Routing rule: a shape is routed only where the kernel's
SLOWEST run beats the library's FASTEST (over both layouts) at every batch size; the pass is measured with exactly those
shapes routed, and mssvt_amd/bev_conv.py::ROUTED must name them.

    python tools/time_bev_conv.py [--runs 5] [--out profiles/bev_conv_times.json]
"""
import argparse
import json
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mssvt_amd import bev_conv, config  # noqa: E402
from mssvt_amd.base_bev_backbone import BaseBEVBackbone  # noqa: E402
from mssvt_amd.height_compression import HeightCompression  # noqa: E402
from mssvt_amd.mssvt_utils import SparseTensor  # noqa: E402

DEV = "cuda"
GRID = 470
# (ksize, cin, cout, stride, dilation, input size, layers of this shape per frame in mssvt.yaml)
LAYERS = [(3, 128, 128, 1, 1, GRID, 8), (3, 128, 128, 1, 2, GRID, 1), (3, 128, 256, 2, 1, GRID, 1), (3, 256, 256, 1, 1, GRID // 2, 5),
          (1, 128, 256, 1, 1, GRID, 1)]


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, runs, iters):
    """{name: [ms per launch, one per run]}: warm up all, then one window each, in turn, `runs` times."""
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            out[k].append(window_ms(fn, iters))
    return out


def layer_times(shape, B, runs):
    k, cin, cout, stride, dil, size, per_frame = shape
    torch.manual_seed(k * 1000 + cin + cout + stride + dil)
    if k == 1:
        conv = nn.ConvTranspose2d(cin, cout, 1, stride=1, bias=False)
    else:
        conv = nn.Conv2d(cin, cout, 3, stride=stride, padding=dil, dilation=dil, bias=False)
    bn, relu = nn.BatchNorm2d(cout, eps=1e-3, momentum=0.01), nn.ReLU()
    conv, bn = conv.to(DEV).eval(), bn.to(DEV).eval()
    x = torch.randn(B, cin, size, size, device=DEV).clamp_(min=0)
    xl = x.contiguous(memory_format=torch.channels_last)
    packed = bev_conv.pack(conv, bn)
    ho, wo = packed.out_size(size, size)
    flop = 2.0 * B * ho * wo * cout * cin * k * k
    with torch.no_grad():
        t = alternate({"library_nchw": lambda: relu(bn(conv(x))), "library_nhwc": lambda: relu(bn(conv(xl))),
                       "hip": lambda: bev_conv.conv_bn_act(xl, packed, True)}, runs, max(3, int(2e11 / flop)))
    lib_best = min(t["library_nchw"] + t["library_nhwc"])
    rec = dict(ksize=k, cin=cin, cout=cout, stride=stride, dilation=dil, B=B, H=size, W=size, layers_per_frame=per_frame,
               flop=flop, ms=t, tflops={n: [flop / (v * 1e-3) / 1e12 for v in vs] for n, vs in t.items()},
               hip_slowest_ms=max(t["hip"]), library_fastest_ms=lib_best, cleared=max(t["hip"]) < lib_best)
    print("k%d %3d->%3d s%d d%d B%d %dx%d: hip %.3f..%.3f ms (%.0f TFLOP/s) | library nchw %.3f..%.3f, nhwc %.3f..%.3f ms (%.0f TFLOP/s) %s" % (
        k, cin, cout, stride, dil, B, size, size, min(t["hip"]), max(t["hip"]), flop / min(t["hip"]) / 1e9,
        min(t["library_nchw"]), max(t["library_nchw"]), min(t["library_nhwc"]), max(t["library_nhwc"]), flop / lib_best / 1e9,
        "CLEARED" if rec["cleared"] else "not cleared"), flush=True)
    return rec


def pass_times(B, runs, routed):
    cfg = config.load_yaml(config.DEFAULT_CFG)
    torch.manual_seed(1)
    hc = HeightCompression(cfg.MODEL.MAP_TO_BEV).to(DEV).eval()
    bev = BaseBEVBackbone(cfg.MODEL.BACKBONE_2D, hc.num_bev_features).to(DEV).eval()
    g = torch.Generator().manual_seed(B)
    rows = []
    for b in range(B):
        cells = torch.randperm(GRID * GRID, generator=g)[:36000].sort().values  # ~1/6 of the cells, as a Waymo frame leaves
        rows.append(torch.stack([torch.full_like(cells, b), torch.zeros_like(cells), cells % GRID, cells // GRID], dim=1))
    vc = torch.cat(rows).int().to(DEV)
    sp = SparseTensor(features=torch.randn(vc.shape[0], 128, device=DEV), indices=vc, spatial_shape=[GRID, GRID, 1],
                      voxel_size=[0.32, 0.32, 6.0], point_cloud_range=[-75.2, -75.2, -2, 75.2, 75.2, 4], batch_size=B,
                      hash_size=400009)

    def run(on):
        hc.fused_convs = bev.fused_convs = on
        return bev(hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1)))["spatial_features_2d"]

    keep = bev_conv.ROUTED
    bev_conv.ROUTED = frozenset(routed)
    try:
        with torch.no_grad():
            diff = float((run(True) - run(False)).abs().max())
            t = alternate({"library": lambda: run(False), "fused_convs": lambda: run(True)}, runs, 3)
    finally:
        bev_conv.ROUTED = keep
    print("pass B%d: library %.2f..%.2f ms, fused_convs %.2f..%.2f ms (max |difference| %.2e)" % (
        B, min(t["library"]), max(t["library"]), min(t["fused_convs"]), max(t["fused_convs"]), diff), flush=True)
    return dict(B=B, ms=t, max_abs_difference=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev_conv_times.json"))
    args = ap.parse_args()
    assert args.runs >= 5, "at least five runs each"
    layers = [layer_times(s, B, args.runs) for s in LAYERS for B in (1, 4)]
    routed = sorted({(r["ksize"], r["cin"], r["cout"], r["stride"], r["dilation"]) for r in layers} -
                    {(r["ksize"], r["cin"], r["cout"], r["stride"], r["dilation"]) for r in layers if not r["cleared"]})
    passes = [pass_times(B, args.runs, routed) for B in (1, 4)]
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, runs=args.runs, grid=GRID, layers=layers,
               routed=[list(s) for s in routed], routed_in_package=sorted(list(s) for s in bev_conv.ROUTED), passes=passes)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("routed (cleared at B = 1 and B = 4): %s -> %s" % (routed, args.out))


if __name__ == "__main__":
    main()
