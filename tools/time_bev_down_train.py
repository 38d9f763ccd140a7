#!/usr/bin/env python3
"""The 3 x 3 stride-2 BEV convolution in TRAINING mode, library (MIOpen through torch autograd) against
``bev_down_train.DownFunction`` (csrc/bev_conv.hip: forward on the inference kernel, input gradient as four parity phases and
weight gradient on the split-fp16 kernels), at the shape of mssvt.yaml (128 -> 256, 470 x 470 -> 235 x 235, B = 1 and 4):

  (a) forward + backward (input and weight gradient) of the one layer -- the library on NCHW tensors (what the modules run
      today) and on channels-last tensors, the Function on channels-last tensors; the weight gradient and the input gradient
      alone as well;
  (b) the whole map_to_bev_module + backbone_2d training step (forward + backward) with fused_train + fused_bn +
      fused_train_deblocks on, without and with fused_train_down, in one process.  `--parent` measures the step without the
      new switch alone: run it with MSSVT_LIB naming a build of the parent commit's library, in a process of its own.

One process; library and kernels alternate in it; every figure is a device-event time around a warmed-up window of several
steps; every run is written out, not a median.  Every GPU step (one batch size, one stage) runs under its own time limit: an
alarm whose default action ends the process, so nothing more is started on the GPU after a step that hangs.
Routing rule: the shape is routed only if the Function's SLOWEST run beats the library's FASTEST (over both
layouts) at every batch size; the stage is measured with the layer routed whatever the outcome (its second figure is what the
switch would give), and mssvt_amd/bev_down_train.py::ROUTED_DOWN_TRAIN must follow the rule.  Each invocation appends one
record to the output file.

    python tools/time_bev_down_train.py [--runs 5] [--out profiles/bev_down_train_times.json] [--parent] [--label TEXT]
"""
import argparse
import json
import os
import signal
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mssvt_amd import _lib, bev_conv_train as bct, bev_deblock_train as bdt, config  # noqa: E402
from mssvt_amd.base_bev_backbone import BaseBEVBackbone  # noqa: E402
from mssvt_amd.height_compression import HeightCompression  # noqa: E402
from mssvt_amd.mssvt_utils import SparseTensor  # noqa: E402

DEV = "cuda"
GRID = 470
SHAPE = (128, 256)  # (cin, cout)
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
    """{name: [ms per step, one per run]}: warm up all (single steps, then one unrecorded window each: the library settles on
    its algorithms and workspaces during its first calls), then one window each, in turn, `runs` times."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for fn in fns.values():
        window_ms(fn, iters)
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


def spread(v):
    return "%.3f..%.3f" % (min(v), max(v))


def layer_times(B, runs):
    from mssvt_amd import bev_down_train as bdn
    cin, cout = SHAPE
    torch.manual_seed(cin + cout + B)
    w = (torch.randn(cout, cin, 3, 3, device=DEV) * 0.03).requires_grad_(True)
    x = torch.randn(B, cin, GRID, GRID, device=DEV).clamp_(min=0).requires_grad_(True)
    xl = x.detach().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    ho, wo = bdn.out_size(GRID, GRID)
    g = torch.randn(B, cout, ho, wo, device=DEV)
    gl = g.contiguous(memory_format=torch.channels_last)

    def step(fwd, inp, grad):
        inp.grad = w.grad = None
        fwd(inp).backward(grad)

    lib = lambda t: F.conv2d(t, w, None, 2, 1)  # noqa: E731
    hip = lambda t: bdn.DownFunction.apply(t, w)  # noqa: E731
    step(lib, xl, gl)
    dx_lib, dw_lib = xl.grad.clone(), w.grad.clone()
    step(hip, xl, gl)
    diff = dict(dx=float((xl.grad - dx_lib).abs().max() / dx_lib.abs().max()), dw=float((w.grad - dw_lib).abs().max() / dw_lib.abs().max()))
    flop = 3 * 2.0 * B * ho * wo * cin * cout * 9  # forward, input gradient, weight gradient
    xd = xl.detach()
    t = alternate({"library_nchw": lambda: step(lib, x, g), "library_nhwc": lambda: step(lib, xl, gl),
                   "hip": lambda: step(hip, xl, gl), "hip_wgrad_alone": lambda: bdn.down_wgrad(xd, gl),
                   "hip_dgrad_alone": lambda: bdn.down_dgrad(gl, w, GRID, GRID)}, runs, max(3, int(3e11 / flop)))
    lib_best = min(t["library_nchw"] + t["library_nhwc"])
    rec = dict(cin=cin, cout=cout, B=B, H=GRID, W=GRID, flop_forward_backward=flop, ms=t, relative_difference_to_library=diff,
               hip_slowest_ms=max(t["hip"]), library_fastest_ms=lib_best, cleared=max(t["hip"]) < lib_best)
    print("(a) %3d->%3d stride 2 B%d %dx%d fwd+bwd: hip %s ms (wgrad alone %s, dgrad alone %s) | library nchw %s, nhwc %s ms %s" % (
        cin, cout, B, GRID, GRID, spread(t["hip"]), spread(t["hip_wgrad_alone"]), spread(t["hip_dgrad_alone"]),
        spread(t["library_nchw"]), spread(t["library_nhwc"]), "CLEARED" if rec["cleared"] else "not cleared"), flush=True)
    return rec


def stage_times(B, runs, parent):
    cfg = config.load_yaml(config.DEFAULT_CFG)
    torch.manual_seed(1)
    hc = HeightCompression(cfg.MODEL.MAP_TO_BEV).to(DEV).train()
    bev = BaseBEVBackbone(cfg.MODEL.BACKBONE_2D, hc.num_bev_features).to(DEV).train()
    hc.fused_train = bev.fused_train = hc.fused_bn = bev.fused_bn = bev.fused_train_deblocks = True
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

    def run(down):
        bev.fused_train_down = down
        for p in params:
            p.grad = None
        sp.features = feats.clone().requires_grad_(True)
        out = bev(hc(dict(encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1)))["spatial_features_2d"]
        out.backward(grad)
        return out.detach(), [p.grad for p in params]

    if parent:
        t, diff = alternate({"all_switches_without_down": lambda: run(False)}, runs, 3), None
    else:
        from mssvt_amd import bev_down_train as bdn
        keep = bdn.ROUTED_DOWN_TRAIN
        bdn.ROUTED_DOWN_TRAIN = frozenset({SHAPE})
        try:
            (y1, g1), (y0, g0) = run(True), run(False)
            diff = dict(output=float((y1 - y0).abs().max() / y0.abs().max()),
                        gradients=max(float((a - b).abs().max() / b.abs().max().clamp_(min=1e-30)) for a, b in zip(g1, g0)))
            del y1, g1, y0, g0
            t = alternate({"all_switches_without_down": lambda: run(False), "all_switches_with_down": lambda: run(True)}, runs, 3)
        finally:
            bdn.ROUTED_DOWN_TRAIN = keep
    print("(b) stage B%d fwd+bwd: %s (relative difference: %s)" % (
        B, ", ".join("%s %s ms" % (k, spread(v)) for k, v in t.items()), diff), flush=True)
    return dict(B=B, ms=t, relative_difference=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev_down_train_times.json"))
    ap.add_argument("--parent", action="store_true", help="(b) only, the new switch off: for a build of the parent's library")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    assert args.runs >= 5, "at least five runs each"
    rec = dict(label=args.label, device=torch.cuda.get_device_name(0), torch=torch.__version__, runs=args.runs, grid=GRID,
               library=os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
               routed_convs_in_package=sorted(list(s) for s in bct.ROUTED_TRAIN),
               routed_deblocks_in_package=sorted(list(s) for s in bdt.ROUTED_DEBLOCK_TRAIN))
    if args.parent:
        rec["stages"] = [limited(stage_times, B, args.runs, True) for B in (1, 4)]
    else:
        from mssvt_amd import bev_down_train as bdn
        rec["layer"] = [limited(layer_times, B, args.runs) for B in (1, 4)]
        rec["routed"] = [list(SHAPE)] if all(r["cleared"] for r in rec["layer"]) else []
        rec["routed_in_package"] = sorted(list(s) for s in bdn.ROUTED_DOWN_TRAIN)
        rec["stages"] = [limited(stage_times, B, args.runs, False) for B in (1, 4)]
        print("ROUTED_DOWN_TRAIN by the rule (cleared at B = 1 and B = 4): %s" % rec["routed"])
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
