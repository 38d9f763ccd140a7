#!/usr/bin/env python3
"""CenterHead's convolutions in TRAINING mode, library (MIOpen through torch autograd) against ``head_conv_train``'s Functions
(csrc/head_conv.hip: forward on the inference kernel, input and weight gradients on the split-fp16 kernels, ordered bias sums), at
the head shape of mssvt.yaml (512 -> 64, five branches, 470 x 470, B = 1 and 4):

  (a) forward + backward of the shared layer (Conv2d 512 -> 64 with bias), and its dX, dW and db alone;
  (b) forward + backward of the trunk (five Conv2d 64 -> 64 with bias reading one tensor), and its dy, dW and db alone;
  (c) BatchNorm2d + ReLU at C = 64 in training mode, forward + backward: the modules against ``bn_train.BnReluFunction``;
  (d) forward + backward of the whole head's convolution stack (shared layer, BatchNorm, ReLU, the five branches with their
      BatchNorm, ReLU and final convolutions): the modules against ``head_conv_train.forward_train`` with both stages routed,
      without and with ``fused_bn``.

The library runs on NCHW tensors (what the modules run today) and on channels-last tensors.  One process; library and kernels
alternate in it, first in one order and then in the reverse order; every figure is a device-event time around a warmed-up
window of several steps; every run is written out, not a median.  Every GPU step (one batch size, one item) runs under its own
time limit: an alarm whose default action ends the process, so nothing more is started on the GPU after a step that hangs.
Routing rule: a stage enters ``head_conv_train.ROUTED_TRAIN`` only if the Function's SLOWEST run beats the
library's FASTEST (over both layouts) at both batch sizes; 64 enters ``ROUTED_BN`` by the same rule on (c).  Each invocation
appends one record to the output file.

    python tools/time_head_conv_train.py [--runs 5] [--out profiles/head_conv_train_times.json] [--label TEXT]
"""
import argparse
import json
import os
import signal
import sys

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mssvt_amd import _lib, bn_train, config, head_conv_train as hct  # noqa: E402
from mssvt_amd.center_head import CenterHead  # noqa: E402

DEV = "cuda"
GRID = 470
CIN, S, NB = 512, 64, 5
STEP_LIMIT_S = 240
TOL = 1e-3  # the project's parity tolerance: no record is written with a head gradient further from the library's


def window_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, runs, iters):
    """{name: [ms per step]}: warm up all (single steps, then one unrecorded window each: the library settles on its algorithms
    and workspaces during its first calls), then one window each in turn, `runs` times in the given order and `runs` times in
    the reverse order."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for fn in fns.values():
        window_ms(fn, iters)
    out = {k: [] for k in fns}
    for order in (list(fns), list(fns)[::-1]):
        for _ in range(runs):
            for k in order:
                out[k].append(window_ms(fns[k], iters))
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


def verdict(t, ours, theirs):
    slow, fast = max(t[ours]), min(sum((t[k] for k in theirs), []))
    return dict(hip_slowest_ms=slow, library_fastest_ms=fast, cleared=slow < fast)


class Smooth(nn.ReLU):
    """Stands in for an nn.ReLU module (the head's structure test wants one) with a continuous activation."""

    def forward(self, x):
        return F.softplus(x)


def nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_(min=1e-30))


def shared_times(B, runs):
    torch.manual_seed(B)
    w = (torch.randn(S, CIN, 3, 3, device=DEV) * 0.02).requires_grad_(True)
    b = torch.randn(S, device=DEV).requires_grad_(True)
    x = torch.randn(B, CIN, GRID, GRID, device=DEV).clamp_(min=0).requires_grad_(True)
    xl = nhwc(x.detach()).requires_grad_(True)
    g = torch.randn(B, S, GRID, GRID, device=DEV)
    gl = nhwc(g)

    def step(fwd, inp, grad):
        inp.grad = w.grad = b.grad = None
        fwd(inp).backward(grad)

    lib = lambda t: F.conv2d(t, w, b, 1, 1)  # noqa: E731
    hip = lambda t: hct.SharedFunction.apply(t, w, b)  # noqa: E731
    step(lib, xl, gl)
    want = [xl.grad.clone(), w.grad.clone(), b.grad.clone()]
    step(hip, xl, gl)
    diff = dict(zip(("dx", "dw", "db"), (rel(a, c) for a, c in zip((xl.grad, w.grad, b.grad), want))))
    del want
    flop = 3 * 2.0 * B * GRID * GRID * CIN * S * 9
    xd = xl.detach()
    t = alternate({"library_nchw": lambda: step(lib, x, g), "library_nhwc": lambda: step(lib, xl, gl),
                   "hip": lambda: step(hip, xl, gl), "hip_forward_alone": lambda: hct.shared_forward(xd, w, b),
                   "hip_dgrad_alone": lambda: hct.shared_dgrad(gl, w), "hip_wgrad_alone": lambda: hct.shared_wgrad(xd, gl),
                   "hip_bgrad_alone": lambda: hct.bias_grad([gl])}, runs, max(3, int(3e11 / flop)))
    rec = dict(stage="shared", cin=CIN, s=S, B=B, H=GRID, W=GRID, flop_forward_backward=flop, ms=t,
               relative_difference_to_library=diff, **verdict(t, "hip", ("library_nchw", "library_nhwc")))
    print("(a) shared %d->%d B%d fwd+bwd: hip %s ms (fwd %s, dX %s, dW %s, db %s) | library nchw %s, nhwc %s ms %s" % (
        CIN, S, B, spread(t["hip"]), spread(t["hip_forward_alone"]), spread(t["hip_dgrad_alone"]), spread(t["hip_wgrad_alone"]),
        spread(t["hip_bgrad_alone"]), spread(t["library_nchw"]), spread(t["library_nhwc"]),
        "CLEARED" if rec["cleared"] else "not cleared"), flush=True)
    return rec


def trunk_times(B, runs):
    torch.manual_seed(10 + B)
    ws = [(torch.randn(S, S, 3, 3, device=DEV) * 0.05).requires_grad_(True) for _ in range(NB)]
    bs = [torch.randn(S, device=DEV).requires_grad_(True) for _ in range(NB)]
    y = torch.randn(B, S, GRID, GRID, device=DEV).clamp_(min=0).requires_grad_(True)
    yl = nhwc(y.detach()).requires_grad_(True)
    gs = [torch.randn(B, S, GRID, GRID, device=DEV) for _ in range(NB)]
    gls = [nhwc(g) for g in gs]

    def step(fwd, inp, grads):
        inp.grad = None
        for p in ws + bs:
            p.grad = None
        torch.autograd.backward(list(fwd(inp)), grads)

    lib = lambda t: [F.conv2d(t, w, b, 1, 1) for w, b in zip(ws, bs)]  # noqa: E731
    hip = lambda t: hct.TrunkFunction.apply(t, NB, *(ws + bs))  # noqa: E731
    step(lib, yl, gls)
    want = [yl.grad.clone()] + [p.grad.clone() for p in ws + bs]
    step(hip, yl, gls)
    diffs = [rel(a, c) for a, c in zip([yl.grad] + [p.grad for p in ws + bs], want)]
    diff = dict(dy=diffs[0], dw=max(diffs[1:1 + NB]), db=max(diffs[1 + NB:]))
    del want
    flop = 3 * 2.0 * B * GRID * GRID * S * S * 9 * NB
    yd = yl.detach()
    t = alternate({"library_nchw": lambda: step(lib, y, gs), "library_nhwc": lambda: step(lib, yl, gls),
                   "hip": lambda: step(hip, yl, gls), "hip_forward_alone": lambda: hct.trunk_forward(yd, ws, bs),
                   "hip_dgrad_alone": lambda: hct.trunk_dgrad(gls, ws), "hip_wgrad_alone": lambda: hct.trunk_wgrad(yd, gls),
                   "hip_bgrad_alone": lambda: hct.bias_grad(gls)}, runs, max(3, int(3e11 / flop)))
    rec = dict(stage="trunk", s=S, nb=NB, B=B, H=GRID, W=GRID, flop_forward_backward=flop, ms=t,
               relative_difference_to_library=diff, **verdict(t, "hip", ("library_nchw", "library_nhwc")))
    print("(b) trunk %d->%dx%d B%d fwd+bwd: hip %s ms (fwd %s, dy %s, dW %s, db %s) | library nchw %s, nhwc %s ms %s" % (
        S, NB, S, B, spread(t["hip"]), spread(t["hip_forward_alone"]), spread(t["hip_dgrad_alone"]), spread(t["hip_wgrad_alone"]),
        spread(t["hip_bgrad_alone"]), spread(t["library_nchw"]), spread(t["library_nhwc"]),
        "CLEARED" if rec["cleared"] else "not cleared"), flush=True)
    return rec


def bn_times(B, runs):
    torch.manual_seed(20 + B)
    bn = nn.BatchNorm2d(S).to(DEV).train()
    relu = nn.ReLU()
    x = torch.randn(B, S, GRID, GRID, device=DEV).requires_grad_(True)
    xl = nhwc(x.detach()).requires_grad_(True)
    g = torch.randn(B, S, GRID, GRID, device=DEV)
    gl = nhwc(g)

    def step(fwd, inp, grad):
        inp.grad = bn.weight.grad = bn.bias.grad = None
        fwd(inp).backward(grad)

    lib = lambda t: relu(bn(t))  # noqa: E731
    hip = lambda t: bn_train.bn_relu(bn, t, True)  # noqa: E731
    t = alternate({"library_nchw": lambda: step(lib, x, g), "library_nhwc": lambda: step(lib, xl, gl),
                   "hip": lambda: step(hip, xl, gl)}, runs, 10)
    rec = dict(stage="bn_relu", C=S, B=B, H=GRID, W=GRID, ms=t, **verdict(t, "hip", ("library_nchw", "library_nhwc")))
    print("(c) BatchNorm + ReLU C=%d B%d fwd+bwd: hip %s ms | library nchw %s, nhwc %s ms %s" % (
        S, B, spread(t["hip"]), spread(t["library_nchw"]), spread(t["library_nhwc"]), "CLEARED" if rec["cleared"] else "not cleared"),
        flush=True)
    return rec


def head_times(B, runs):
    cfg = config.load_yaml(config.DEFAULT_CFG)
    torch.manual_seed(1)
    names = list(cfg.CLASS_NAMES)
    head = CenterHead(cfg.MODEL.DENSE_HEAD, CIN, len(names), names, [GRID, GRID, 1], [-75.2, -75.2, -2, 75.2, 75.2, 4],
                      [0.32, 0.32, 6.0], predict_boxes_when_training=False).to(DEV).train()
    assert hct.train_supported(head)
    x = torch.randn(B, CIN, GRID, GRID, device=DEV).clamp_(min=0).requires_grad_(True)
    xl = nhwc(x.detach()).requires_grad_(True)
    params = list(head.parameters())
    grads = None

    def modules(t):
        y = head.shared_conv(t)
        return [m for sep in head.heads_list for m in sep(y).values()]

    def fused(t):
        return [m for d in hct.forward_train(head, t) for m in d.values()]

    def step(fwd, inp, fused_bn=False):
        head.fused_bn = fused_bn
        inp.grad = None
        for p in params:
            p.grad = None
        torch.autograd.backward(fwd(inp), grads)

    with torch.no_grad():
        grads = [torch.randn_like(m) * 1e-3 for m in modules(xl)]
    keep = hct.ROUTED_TRAIN, hct.ROUTED_BN
    hct.ROUTED_TRAIN, hct.ROUTED_BN = frozenset(hct.STAGES), frozenset({S})
    try:
        keys = ["input"] + [k for k, _ in head.named_parameters()]

        def gradients(fwd, inp, fused_bn=False):
            step(fwd, inp, fused_bn)
            return dict(zip(keys, [inp.grad.clone()] + [p.grad.clone() for p in params]))

        def differences(got, want):
            # the bias of a convolution in front of a BatchNorm in training mode has the exact gradient ZERO (the batch mean takes
            # a constant shift out): both runs hold rounding noise there, stated against the scale of the same layer's weight
            # gradient (the same dY makes both); every other gradient against the reference's own
            per = {k: (float(got[k].abs().max() / want[k[:-4] + "weight"].abs().max()) if k.endswith(".0.bias") else rel(got[k], want[k]))
                   for k in keys}
            worst = max(per, key=per.get)
            return dict(per_tensor=per, largest=per[worst], at=worst)

        # (1) with the ReLUs: a step function behind every BatchNorm.  Two evaluations that differ by 1e-6 put the ~1e-6 of the
        # 85 million pre-activations that lie that close to zero on different sides, and each such unit changes the gradients
        # around it by its whole contribution: the library differs from ITSELF (NCHW against channels-last features) by as much
        # as the Functions differ from it.  Reported, all three; not a parity figure
        want = gradients(modules, xl)
        diff = dict(relu=dict(library_nchw_against_library_nhwc=differences(gradients(modules, x), want),
                              fused_bn_off=differences(gradients(fused, xl), want),
                              fused_bn_on=differences(gradients(fused, xl, True), want)))
        # (2) the same head with a smooth activation in place of every nn.ReLU module (softplus; bn_train's own ReLU cannot be
        # replaced, so fused_bn stays off): the composition is continuous and every gradient must agree to the parity tolerance
        relus = [(parent, name) for parent in head.modules() for name, m in parent.named_children() if type(m) is nn.ReLU]
        for parent, name in relus:
            setattr(parent, name, Smooth())
        try:
            want = gradients(modules, xl)
            diff["smooth"] = dict(fused_bn_off=differences(gradients(fused, xl), want))
        finally:
            for parent, name in relus:
                setattr(parent, name, nn.ReLU())
        del want
        for kind, d in diff.items():
            for tag, v in d.items():
                print("    B%d %s %s, the three largest: %s" % (B, kind, tag, ", ".join(
                    "%s %.2e" % (k, v["per_tensor"][k]) for k in sorted(v["per_tensor"], key=v["per_tensor"].get)[-3:])), flush=True)
        v = diff["smooth"]["fused_bn_off"]
        assert v["largest"] <= TOL, "smooth activation: gradient %s differs from the library's by %.3e of its scale" % (v["at"], v["largest"])
        t = alternate({"library_nchw": lambda: step(modules, x), "library_nhwc": lambda: step(modules, xl),
                       "hip_both_stages": lambda: step(fused, xl), "hip_both_stages_fused_bn": lambda: step(fused, xl, True)}, runs, 3)
    finally:
        hct.ROUTED_TRAIN, hct.ROUTED_BN = keep
    rec = dict(stage="head", B=B, H=GRID, W=GRID, ms=t, relative_difference_of_gradients_to_library=diff)
    print("(d) head B%d fwd+bwd: %s" % (B, ", ".join("%s %s ms" % (k, spread(v)) for k, v in t.items())), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_conv_train_times.json"))
    ap.add_argument("--label", default="")
    ap.add_argument("--head-only", action="store_true", help="item (d) alone (its value check and times); no routing verdict")
    args = ap.parse_args()
    assert args.runs >= 5, "at least five runs in each order"
    rec = dict(label=args.label, device=torch.cuda.get_device_name(0), torch=torch.__version__, runs_per_order=args.runs, grid=GRID,
               library=os.path.basename(os.path.dirname(_lib.LIB_PATH)) + "/" + os.path.basename(_lib.LIB_PATH),
               wgrad_slice_pixels=hct.slice_pixels(CIN, S))
    if not args.head_only:
        rec["shared"] = [limited(shared_times, B, args.runs) for B in (1, 4)]
        rec["trunk"] = [limited(trunk_times, B, args.runs) for B in (1, 4)]
        rec["bn_relu"] = [limited(bn_times, B, args.runs) for B in (1, 4)]
    rec["head"] = [limited(head_times, B, args.runs) for B in (1, 4)]
    if not args.head_only:
        rec["routed_train"] = sorted(k for k in ("shared", "trunk") if all(r["cleared"] for r in rec[k]))
        rec["routed_bn"] = [S] if all(r["cleared"] for r in rec["bn_relu"]) else []
    rec["routed_train_in_package"] = sorted(hct.ROUTED_TRAIN)
    rec["routed_bn_in_package"] = sorted(hct.ROUTED_BN)
    if not args.head_only:
        print("ROUTED_TRAIN by the rule (cleared at B = 1 and B = 4): %s; ROUTED_BN: %s" % (rec["routed_train"], rec["routed_bn"]))
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
