#!/usr/bin/env python3
"""The deblock stage of BaseBEVBackbone in eval mode at the shapes of mssvt.yaml (470 x 470 BEV grid, B = 1 and 4), with the
method of tools/time_bev_conv.py (kernel and library alternate in one process, device events around warmed-up windows of
>= 3 launches, five runs, every run written out):

  (a) the 2 x 2 stride-2 transposed deblock 256 -> 256, 235^2 -> 470^2, alone: bev_conv.up2_bn_act (exponent pass included)
      against the library's ConvTranspose + BN + ReLU on NCHW and on channels-last tensors.  Rule: the kernel's
      SLOWEST run must beat the library's FASTEST over both layouts, at both batch sizes; only then does (256, 256) belong in
      bev_conv.ROUTED_UP2;
  (b) the stage: both deblocks into one shared tensor (up-2 on the kernel, and up-2 through the library + copy_) against
      today's fused_convs stage (1 x 1 on the kernel, library transposed deblock, torch.cat);
  (c) the whole map_to_bev_module + backbone_2d pass with fused_convs, fused_deblocks off (the parent's path) and on.
      `--parent` measures the off path alone: run it with MSSVT_LIB naming a build of the parent commit's library.

Every invocation APPENDS one record to the JSON.

    python tools/time_bev_deblocks.py [--runs 5] [--out profiles/bev_deblock_times.json] [--parent] [--label TEXT]
"""
import argparse
import json
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from mssvt_amd import _lib, bev_conv, config  # noqa: E402
from mssvt_amd.base_bev_backbone import BaseBEVBackbone  # noqa: E402
from mssvt_amd.height_compression import HeightCompression  # noqa: E402
from mssvt_amd.mssvt_utils import SparseTensor  # noqa: E402
from time_bev_conv import alternate  # noqa: E402

DEV = "cuda"
GRID = 470


def layers():
    torch.manual_seed(7)
    one = nn.Sequential(nn.ConvTranspose2d(128, 256, 1, stride=1, bias=False), nn.BatchNorm2d(256, eps=1e-3, momentum=0.01), nn.ReLU())
    up = nn.Sequential(nn.ConvTranspose2d(256, 256, 2, stride=2, bias=False), nn.BatchNorm2d(256, eps=1e-3, momentum=0.01), nn.ReLU())
    return one.to(DEV).eval(), up.to(DEV).eval()


def spread(vs):
    return "%.3f..%.3f" % (min(vs), max(vs))


def up2_times(B, runs):
    _, up = layers()
    x = torch.randn(B, 256, GRID // 2, GRID // 2, device=DEV).clamp_(min=0)
    xl = x.contiguous(memory_format=torch.channels_last)
    packed = bev_conv.pack_up2(up[0], up[1])
    with torch.no_grad():
        diff = float((bev_conv.up2_bn_act(xl, packed, True) - up(x)).abs().max())
        t = alternate({"library_nchw": lambda: up(x), "library_nhwc": lambda: up(xl),
                       "hip": lambda: bev_conv.up2_bn_act(xl, packed, True)}, runs, 3)
    lib_best = min(t["library_nchw"] + t["library_nhwc"])
    rec = dict(B=B, H=GRID // 2, W=GRID // 2, cin=256, cout=256, ms=t, hip_slowest_ms=max(t["hip"]), library_fastest_ms=lib_best,
               cleared=max(t["hip"]) < lib_best, max_abs_difference=diff)
    print("(a) up-2 256->256 B%d: hip %s ms | library nchw %s, nhwc %s ms  %s (max |difference| %.2e)" % (
        B, spread(t["hip"]), spread(t["library_nchw"]), spread(t["library_nhwc"]), "CLEARED" if rec["cleared"] else "not cleared", diff),
        flush=True)
    return rec


def stage_times(B, runs):
    one, up = layers()
    x1 = torch.randn(B, 128, GRID, GRID, device=DEV).clamp_(min=0).contiguous(memory_format=torch.channels_last)
    x2 = torch.randn(B, 256, GRID // 2, GRID // 2, device=DEV).clamp_(min=0).contiguous(memory_format=torch.channels_last)
    p1, p2 = bev_conv.pack(one[0], one[1]), bev_conv.pack_up2(up[0], up[1])

    def today():
        return torch.cat([bev_conv.conv_bn_act(x1, p1, True), up(x2)], dim=1)

    def into(kernel):
        out = torch.empty((B, GRID, GRID, 512), dtype=torch.float32, device=DEV).permute(0, 3, 1, 2)
        bev_conv.conv_bn_act(x1, p1, True, out=out, channel=0)
        if kernel:
            bev_conv.up2_bn_act(x2, p2, True, out=out, channel=256)
        else:
            out[:, 256:].copy_(up(x2))
        return out

    with torch.no_grad():
        diff = float((into(True) - today()).abs().max())
        t = alternate({"fused_convs_stage": today, "into_kernel_up2": lambda: into(True), "into_library_up2": lambda: into(False)},
                      runs, 3)
    print("(b) stage B%d: today %s ms | into, up-2 on the kernel %s | into, up-2 through the library %s (max |difference| %.2e)" % (
        B, spread(t["fused_convs_stage"]), spread(t["into_kernel_up2"]), spread(t["into_library_up2"]), diff), flush=True)
    return dict(B=B, ms=t, max_abs_difference=diff)


def pass_times(B, runs, parent, up2_routed):
    cfg = config.load_yaml(config.DEFAULT_CFG)
    torch.manual_seed(1)
    hc = HeightCompression(cfg.MODEL.MAP_TO_BEV).to(DEV).eval()
    bev = BaseBEVBackbone(cfg.MODEL.BACKBONE_2D, hc.num_bev_features).to(DEV).eval()
    hc.fused_convs = bev.fused_convs = True
    g = torch.Generator().manual_seed(B)
    rows = []
    for b in range(B):
        cells = torch.randperm(GRID * GRID, generator=g)[:36000].sort().values  # ~1/6 of the cells, as a Waymo frame leaves
        rows.append(torch.stack([torch.full_like(cells, b), torch.zeros_like(cells), cells % GRID, cells // GRID], dim=1))
    vc = torch.cat(rows).int().to(DEV)
    sp = SparseTensor(features=torch.randn(vc.shape[0], 128, device=DEV), indices=vc, spatial_shape=[GRID, GRID, 1],
                      voxel_size=[0.32, 0.32, 6.0], point_cloud_range=[-75.2, -75.2, -2, 75.2, 75.2, 4], batch_size=B,
                      hash_size=400009)

    def run(deblocks):
        bev.fused_deblocks = deblocks
        return bev(hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1)))["spatial_features_2d"]

    keep = bev_conv.ROUTED_UP2
    bev_conv.ROUTED_UP2 = frozenset({(256, 256)}) if up2_routed else frozenset()
    try:
        with torch.no_grad():
            if parent:
                t, diff = alternate({"fused_convs": lambda: run(False)}, runs, 3), None
            else:
                diff = float((run(True) - run(False)).abs().max())
                t = alternate({"fused_convs": lambda: run(False), "fused_deblocks": lambda: run(True)}, runs, 3)
    finally:
        bev_conv.ROUTED_UP2 = keep
    print("(c) pass B%d: %s" % (B, ", ".join("%s %s ms" % (k, spread(v)) for k, v in t.items())), flush=True)
    return dict(B=B, ms=t, up2_on_the_kernel=bool(up2_routed), max_abs_difference=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev_deblock_times.json"))
    ap.add_argument("--parent", action="store_true", help="(c) only, fused_deblocks off: for a build of the parent's library")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    assert args.runs >= 5, "at least five runs each"
    rec = dict(label=args.label, device=torch.cuda.get_device_name(0), torch=torch.__version__, runs=args.runs, grid=GRID,
               library=os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH))
    if args.parent:
        rec["passes"] = [pass_times(B, args.runs, True, False) for B in (1, 4)]
    else:
        rec["up2"] = [up2_times(B, args.runs) for B in (1, 4)]
        cleared = all(r["cleared"] for r in rec["up2"])
        rec["routed_up2"] = [[256, 256]] if cleared else []
        rec["routed_up2_in_package"] = sorted(list(s) for s in bev_conv.ROUTED_UP2)
        rec["stage"] = [stage_times(B, args.runs) for B in (1, 4)]
        rec["passes"] = [pass_times(B, args.runs, False, cleared) for B in (1, 4)]
        print("ROUTED_UP2 by the rule: %s" % rec["routed_up2"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    records = []
    if os.path.exists(args.out):
        with open(args.out) as f:
            records = json.load(f)["records"]
    with open(args.out, "w") as f:
        json.dump(dict(records=records + [rec]), f, indent=1)
    print("appended record %d to %s" % (len(records) + 1, args.out))


if __name__ == "__main__":
    main()
