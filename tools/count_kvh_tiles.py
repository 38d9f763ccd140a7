"""How many (window, head group) steps of k_attn_kvh keep every live key in key tile 0, and how many passes a window takes,
on frame 0 of the bench scene (usage: python tools/count_kvh_tiles.py [batch] [points]).

Per two-scale Block: the plan's kmeta of both groups and the nq_valid row of the Block's query pattern, from the
Python-driven path (fused.two_scale_plan).  A step is ACTIVE when its window has a valid query of that pattern (the work
order lists exactly those); it is ONE-TILE when no slot 16 .. K-1 of its key list holds a row.  Prints one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from mssvt_amd import config, fused  # noqa: E402
from mssvt_amd.mssvt_utils import SparseTensor  # noqa: E402

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1
points = int(sys.argv[2]) if len(sys.argv) > 2 else 160000
dev = torch.device("cuda", 0)
torch.manual_seed(0)
net = config.build_backbone_from_cfg().to(dev).eval()
_, _, vc, feats = bench.make_inputs(points, batch, 0, dev)
out = {"points": points, "batch": batch, "blocks": []}
seen = set()
with torch.no_grad():
    sp = SparseTensor(features=feats, indices=vc.int().contiguous(), spatial_shape=net.grid_size,
                      voxel_size=net.voxel_size, point_cloud_range=net.point_cloud_range, batch_size=batch,
                      hash_size=net.hash_size)
    for bi, blk in enumerate(net.backbone):
        if not hasattr(blk, "cbs_pattern") or not hasattr(blk, "ms_attn"):
            continue
        pat = int(blk.cbs_pattern)
        if pat in seen:  # the plan depends on the voxel positions alone: one Block per query pattern
            continue
        seen.add(pat)
        p = fused.two_scale_plan(blk, sp)
        nw = int(p.num_wins.item())
        nqv = p.nq_valid[{1: 0, 0: 1, 2: 2}[pat]][:nw].long()
        active = nqv > 0
        passes = (nqv[active] + 3) // 4
        rec = {"block": bi, "cbs_pattern": pat, "windows": nw, "active_windows": int(active.sum()),
               "query_rows": int(nqv.sum()), "passes_total": int(passes.sum()),
               "passes_per_window": {str(k): int((passes == k).sum()) for k in sorted(set(passes.tolist()))}, "groups": []}
        for g, km in enumerate(p.kmeta):
            rows = km.view(torch.int32)[:nw, :, 3]
            live = rows >= 0
            one = ~live[:, 16:].any(1)
            rec["groups"].append({
                "group": g, "window_size": list(blk.window_size[g]) if hasattr(blk, "window_size") else None,
                "live_slots_active": int(live[active].sum()), "slots_active": int(active.sum()) * rows.shape[1],
                "one_tile_steps": int((one & active).sum()), "active_steps": int(active.sum()),
                "one_tile_share": float((one & active).sum()) / max(int(active.sum()), 1),
                "one_tile_pass_share": float(passes[one[active]].sum()) / max(int(passes.sum()), 1)})
        out["blocks"].append(rec)
steps = sum(g["active_steps"] for b in out["blocks"] for g in b["groups"])
one = sum(g["one_tile_steps"] for b in out["blocks"] for g in b["groups"])
out["one_tile_share_all"] = one / max(steps, 1)
print(json.dumps(out))
