"""How many steps and passes k_attn_kvh saves when two one-tile windows share a wavefront, on frame 0 of the bench scene
(usage: python tools/count_kvh_pairs.py [batch] [points]).

Per query pattern and head group, from the Python-driven plan (fused.two_scale_plan), as tools/count_kvh_tiles.py: a window
is ACTIVE when it has a valid query of the pattern, ONE-TILE in a group when no slot 16 .. K-1 of its key list holds a row.
The work order sorts windows by query count (descending); pairing takes the one-tile windows of a query-count bucket two by
two, so at most one of them per bucket stays single.  A pair takes ceil((nqA + nqB) / 4) passes.  Prints one JSON line."""
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
out = {"points": points, "batch": batch, "patterns": []}
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
        nqv = p.nq_valid[{1: 0, 0: 1, 2: 2}[pat]][:nw].long().cpu()
        active = nqv > 0
        rec = {"block": bi, "cbs_pattern": pat, "active_windows": int(active.sum()), "groups": []}
        for g, km in enumerate(p.kmeta):
            rows = km.view(torch.int32)[:nw, :, 3].cpu()
            one = ~(rows[:, 16:] >= 0).any(1)
            steps0 = int(active.sum())
            passes0 = int(((nqv[active] + 3) // 4).sum())
            steps1 = passes1 = singles = pairs = 0
            for n in sorted(set(nqv[active].tolist())):
                c1 = int((active & one & (nqv == n)).sum())   # pairable
                c2 = int((active & ~one & (nqv == n)).sum())  # upper tile live: single
                steps1 += (c1 + 1) // 2 + c2
                pairs += c1 // 2
                singles += c1 % 2
                passes1 += (c1 // 2) * ((2 * n + 3) // 4) + (c1 % 2 + c2) * ((n + 3) // 4)
            rec["groups"].append({
                "group": g, "window_size": list(blk.window_size[g]) if hasattr(blk, "window_size") else None,
                "one_tile_windows": int((active & one).sum()), "steps": steps0, "steps_paired": steps1,
                "passes": passes0, "passes_paired": passes1, "pairs": pairs, "one_tile_left_single": singles})
        s0 = sum(x["steps"] for x in rec["groups"])
        s1 = sum(x["steps_paired"] for x in rec["groups"])
        rec["steps"], rec["steps_paired"], rec["steps_saved_share"] = s0, s1, 1.0 - s1 / max(s0, 1)
        rec["passes"] = sum(x["passes"] for x in rec["groups"])
        rec["passes_paired"] = sum(x["passes_paired"] for x in rec["groups"])
        out["patterns"].append(rec)
print(json.dumps(out))
