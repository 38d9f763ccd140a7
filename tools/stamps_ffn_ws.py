"""Developer tool: where a wave of k_ffn_ws spends its cycles (build with MSSVT_EXTRA_HIPCC_FLAGS=-DMSSVT_STAMPS).

    python tools/stamps_ffn_ws.py [rows] [out.json]

Runs the Block form (interpolation table and plain input, next LayerNorm) at `rows` and, with a device row count, the CompressBlock form
(plain input, no LayerNorm) at rows / 4; prints the per-phase clocks and writes them to out.json."""
import ctypes, json, os, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mssvt_amd import config, fused, _lib
dev = torch.device("cuda", 0)
torch.manual_seed(0)
net = config.build_backbone_from_cfg().to(dev).eval()
blk = net.backbone[0]
n = int(sys.argv[1]) if len(sys.argv) > 1 else 74270
out_path = sys.argv[2] if len(sys.argv) > 2 else None
class SP(object):
    _next_norm1 = net.backbone[1].norm1
class SPnone(object):
    _next_norm1 = None
fused.FFN_ARITH = "f16x3"
# slots of g_ws_stamps: s_memtime clocks between consecutive WSTAMP sites, summed over the tiles of a wave (about 2.25 per ns
# on the MI355X: 89 000 per wave over a 39.7 us workgroup; the spans below are on the 100 MHz wall clock)
names = {7: "head: entry -> every head load issued", 8: "head: -> at the first barrier (LayerNorm parameters in LDS)",
         10: "head: first barrier", 11: "head: A(t0) (waits for the gathers)", 12: "head: second barrier",
         0: "head: GEMM1(t0) (waits for W1)", 1: "loop top (first: third barrier, wait for W2)",
         2: "I2: GEMM2(t) | A(t+1), issue t+2", 3: "barrier behind I2", 4: "I1: D(t) | GEMM1(t+1), split u -> LDS", 5: "barrier behind I1",
         6: "exit", 14: "tail: GEMM2(t)", 15: "tail: barrier, D(t)"}
order = [7, 8, 10, 11, 12, 0, 1, 2, 3, 4, 5, 14, 15, 6]
HEAD = (7, 8, 10, 11, 12, 0)


def run(label, sp, rows, n_dev, tabbed=False):
    x = torch.randn(rows, 128, device=dev)
    table = None
    if tabbed:  # three interpolation sources per row ~160 rows apart, as the x-slabs of a window are; every 16th row unowned
        g = torch.Generator(device="cpu").manual_seed(1)
        tab_row = ((torch.arange(rows).unsqueeze(1) + torch.tensor([[-160, 0, 160, 0]])).clamp(0, rows - 1)).to(torch.int32)
        tab_row[::16, 0] = -1
        tab_w = torch.rand(rows, 4, generator=g)
        table = ((tab_row.to(dev).contiguous(), tab_w.to(dev).contiguous()), torch.randn(rows, 128, device=dev))
    with torch.no_grad():
        for _ in range(3):
            if tabbed:
                fused._ffn_tail(blk, sp, None, x_in=x, table=table)
            else:
                fused._ffn_tail(blk, sp, x, n_rows_dev=n_dev, apply_out=n_dev is None)
    torch.cuda.synchronize()
    buf = np.zeros(4 * 8 * 16, dtype=np.uint64)
    _lib.lib().mssvt_debug_read_ffn_ws_stamps(buf.ctypes.data_as(ctypes.c_void_p))
    s = buf.reshape(32, 16).astype(np.float64)
    tiles = s[:, 9].mean()
    tot = s[:, order].sum(1).mean()
    print("%s: %d rows, waves %d, loop iterations per wave %.1f, clocks per wave %.0f (s_memtime clocks: set them against the workgroup durations below)"
          % (label, rows, s.shape[0], tiles, tot))
    for k in order:
        print("   %-60s %9.0f   %5.1f%%" % (names[k], s[:, k].mean(), 100 * s[:, k].mean() / tot))
    head = s[:, HEAD].sum(1)
    first = s[:, (7, 8, 10)].sum(1)
    print("   entry -> first barrier released: mean %.0f; entry -> loop entry: mean %.0f, min %.0f, max %.0f; last tile, loop top -> exit: %.0f"
          % (first.mean(), head.mean(), head.min(), head.max(), s[:, 13].mean()))
    return {"rows": rows, "loop_iterations_per_wave": tiles, "clocks_mean_over_32_waves": {names[k]: s[:, k].mean() for k in order},
            "entry_to_first_barrier_released": first.mean(), "entry_to_loop_entry": head.mean(),
            "last_tile_loop_top_to_exit": s[:, 13].mean(),
            "per_wave_of_workgroup_0": {names[k]: s[:8, k].tolist() for k in order}}


res = {"block_form_table": run("Block form <table, next LayerNorm>", SP(), n, None, tabbed=True),
       "block_form_plain": run("Block form <plain input, next LayerNorm>", SP(), n, None)}
cnt = torch.tensor([n // 4], dtype=torch.int32, device=dev)
res["compress_form_device_count"] = run("CompressBlock form <plain, no LayerNorm, device row count>", SPnone(), n // 4, cnt)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)

# ---- launch skew and tail of the grid: start / end of every workgroup on the 100 MHz wall clock (round 4)
x = torch.randn(n, 128, device=dev)
if hasattr(_lib.lib(), "mssvt_debug_read_ffn_ws_spans"):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        e0.record()
        fused._ffn_tail(blk, SP(), x)
        e1.record()
    torch.cuda.synchronize()
    sp = np.zeros(1024 * 2, dtype=np.uint64)
    _lib.lib().mssvt_debug_read_ffn_ws_spans(sp.ctypes.data_as(ctypes.c_void_p))
    grid = min(256, (n + 15) // 16)
    sp = sp.reshape(1024, 2)[:grid].astype(np.float64) / 100.0  # us
    t0 = sp[:, 0].min()
    st, en = sp[:, 0] - t0, sp[:, 1] - t0
    print("grid %d: event time of the launch %.1f us; first start -> last end %.1f us" % (grid, e0.elapsed_time(e1) * 1e3, en.max()))
    pct = lambda v: " ".join("%.1f" % np.percentile(v, p) for p in (0, 10, 50, 90, 100))
    print("   start offsets (us, p0 p10 p50 p90 p100): ", pct(st))
    print("   end   offsets (us):                      ", pct(en))
    print("   workgroup durations (us):                ", pct(en - st))
