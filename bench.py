"""bench.py -- frames/s of the MsSVT backbone on MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--points 160000] [--batch 1]
                    [--attn-dtype f32|bf16] [--train] [--cfg yaml] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one backbone forward (voxel_coords, voxel_features -> encoded SparseTensor, eval mode)
over one batch of synthetic Waymo-shaped scenes already resident in HBM; with ``--train`` one
DistributedDataParallel training step (forward + backward + gradient all-reduce over RCCL + SGD).
Workload at N=1: BASELINE.json configs[1] -- one 160k-point scene, the full mssvt.yaml backbone
("W": 4 Blocks + 1 CompressBlock, C=128, windows [3,3,5]/[7,7,7]), fp32.  ``--batch 8 --attn-dtype
bf16`` is configs[2]; ``--gpus 8 --batch 4`` the per-GPU shape of configs[3].

``--gpus N`` with N > 1 and no torchrun environment: this process starts N ranks itself
(``python -m torch.distributed.run``, one per GPU, RCCL) BEFORE it makes any GPU call, relays their
output and exits with their status.  Scenes are sharded by rank (no data-path collective; weak
scaling); the time is the max over ranks between barriers.

Prints ONE JSON line on rank 0 with the driver's contract fields (metric, value, unit, higher_is_better, dtype,
ms_per_step = the milliseconds of one of the K timed steps) and the configuration that ran.  A plain run does only that:
set up, warm up, time the K steps, write the outputs (--dump-outputs), print the line.  ``--full`` adds, after the timed
steps and outside them,
  "timing":       median / p10 / p90 of >= 50 steps timed one by one with HIP events;
  "one_frame_in_flight": with frames in flight, the same K steps one at a time on one stream;
  "roofline":     the dominant kernel (k_ffn_ws: the FFN tail in one launch, HBM bound) measured live with HIP events, and
                  "frame": the whole frame's algorithmic bytes / FLOP against both roofs (off with --no-roofline);
  "cpu_baseline": the CPU oracle (a port of the reference's CUDA semantics; the reference has no CPU
                  path) timed on the host: the whole forward on all cores and on one thread (off with --no-cpu-baseline);
  config.output_voxels: the output rows of frame 0, run once more (also with --from-points, whose byte count reads it;
                  a --train line always reports its last step's).

``--dump-outputs DIR``: right after the timed steps, rank 0 writes what the last timed step returned to its caller --
every array of the output dict that is not an input of the step (the SparseTensor as ``<key>.features`` /
``<key>.indices``) -- as ``DIR/<name>.npy``, floating point as float32 (float64 stays float64), integers as float64.
Above 64 MiB in all, every array is replaced by a fixed seeded sample of its flattened elements, written beside the
flat positions it took (``DIR/<name>.index.npy``).  The inputs depend on the arguments alone (seeded generators), so two
builds can be compared output for output.
"""
import argparse
import json
import os
import subprocess
import sys

os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")  # see mssvt_amd/__init__.py (must precede the first GPU call)
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E peak 8 TB/s (6.3 TB/s achievable)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--points", type=int, default=160000, help="LiDAR points per scene")
    ap.add_argument("--batch", type=int, default=1, help="scenes per GPU per step")
    ap.add_argument("--impl", default=None, choices=[None, "fused", "ops"])
    ap.add_argument("--attn-dtype", default="f32", choices=["f32", "bf16"],
                    help="operand type of the window-attention matrix products (accumulation and softmax stay fp32)")
    ap.add_argument("--train", action="store_true", help="DDP training step instead of the inference forward")
    ap.add_argument("--detector", action="store_true",
                    help="with --train: the whole CenterPoint detector (DynamicVFE -> backbone -> HeightCompression -> BEV backbone -> "
                         "CenterHead losses) under DistributedDataParallel, points + synthetic boxes in (ref tools/train.py:143-144)")
    ap.add_argument("--sync-bn", action="store_true",
                    help="with --detector: BatchNorm layers -> SyncBatchNorm before the DDP wrap (ref tools/train.py:118-119)")
    ap.add_argument("--cfg", default=None, help="backbone yaml (default: mssvt_amd/cfgs/mssvt.yaml = BASELINE configs[1])")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--ffn-arith", choices=["f16x3", "f32"], default=None,
                    help="matrix products of the FFN / CompressBlock: split-fp16 operands (default) or the fp32 MFMA")
    ap.add_argument("--arith", choices=["split16", "f32"], default="split16",
                    help="every matrix product of the fp32 path: fp32 operands as two fp16 halves on the 16-bit MFMA (default), "
                         "or f32 = the native v_mfma_f32_16x16x4_f32 in the FFN, the CompressBlock AND the three attention "
                         "launches (the reference's own operand width; the comparator line kept beside the headline)")
    ap.add_argument("--from-points", action="store_true",
                    help="a step = points -> voxelizer + DynamicVFE -> backbone -> dense() / HeightCompression view (SURVEY 8 f1, "
                         "f2: the neighbours either side of the path), with its own algorithmic bytes; not the BASELINE metric")
    ap.add_argument("--master-port", type=int, default=0, help="rendezvous port when this process starts the ranks")
    ap.add_argument("--in-flight", type=int, default=None,
                    help="frames in flight (mssvt_amd/pipeline.py: consecutive frames are independent; each runs on its own HIP "
                         "stream with its own workspace); 1: one frame at a time on one stream, as every round before round 5; "
                         "default: pipeline.auto_depth(batch) -- 4 below four scenes per step, 1 from there on")
    ap.add_argument("--frames", type=int, default=4,
                    help="distinct resident frames the steps rotate over (1: the same frame from the same addresses every step)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure per-step timing, one frame in flight, the roofline and the CPU "
                         "baseline (module docstring); off: the headline figure only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (module docstring)")
    args = ap.parse_args(argv)
    if args.in_flight is None:
        from mssvt_amd.pipeline import auto_depth
        args.in_flight = auto_depth(args.batch)
    return args


def spawn_ranks(args):
    """--gpus N without a torchrun environment: start the N ranks as children (nothing in this process
    has touched the GPU yet, and nothing will), relay their stdout / stderr, return their exit status."""
    # a port of our own choosing could be taken between the probe and torchrun's bind: unless one is given, torchrun's
    # c10d rendezvous picks a free one itself (--rdzv-endpoint ...:0)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus)]
    if args.master_port:
        cmd += ["--master-addr", "127.0.0.1", "--master-port", str(args.master_port)]
    else:
        cmd += ["--rdzv-backend", "c10d", "--rdzv-endpoint", "127.0.0.1:0", "--local-addr", "127.0.0.1"]
    cmd += [os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    return subprocess.call(cmd, env=env)


def make_inputs(points, batch, rank, device, frame=0):
    """Frame `frame` of this rank: frame 0 is the scene set every earlier round benchmarked (and the tests pin to the
    oracle); further frames are other scenes of the same generator (the timed steps rotate over them)."""
    from mssvt_amd import synthetic
    from mssvt_amd.dist import scene_seeds
    pts = synthetic.make_batch_points(points, batch, seed0=scene_seeds(rank, batch)[0] + 7919 * frame)
    vc, _, _ = synthetic.voxelize_numpy(pts)
    g = torch.Generator().manual_seed(1000 + rank + 31 * frame)
    feats = torch.randn(vc.shape[0], 128, generator=g)
    return vc, feats.numpy(), torch.from_numpy(vc).to(device), feats.to(device)


def event_time_ms(fn, iters, warm=3):
    """Average duration of fn() (which enqueues work on torch's current HIP stream)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def per_step_times_ms(step, iters):
    """Each step between two HIP events on the launching stream (the library launches on torch's current
    stream); returns the sorted list."""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    torch.cuda.synchronize()
    for e0, e1 in evs:
        e0.record()
        step()
        e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) for e0, e1 in evs)


DUMP_LIMIT_BYTES = 64 << 20


def output_arrays(out, inputs):
    """{name: numpy array} of a step's output dict without its `inputs` keys: tensors as they are, a SparseTensor as
    `<key>.features` / `<key>.indices`; floating point as float32 (float64 kept), integers and booleans as float64."""
    import numpy as np
    from mssvt_amd.pipeline import FramePipeline
    out = FramePipeline.result(out)
    arrays = {}

    def put(name, t):
        a = t.detach().cpu().numpy()
        arrays[name] = a.astype(a.dtype if a.dtype == np.float64 else
                                np.float32 if np.issubdtype(a.dtype, np.floating) else np.float64)
    for key in sorted(out):
        v = out[key]
        if key in inputs:
            continue
        if isinstance(v, torch.Tensor):
            put(key, v)
        elif hasattr(v, "features") and hasattr(v, "indices"):
            put(key + ".features", v.features)
            put(key + ".indices", v.indices)
    return arrays


def dump_outputs(arrays, dirname, limit=DUMP_LIMIT_BYTES):
    """Write `arrays` as DIR/<name>.npy; above `limit` bytes in all, a seeded sample of every array's flattened elements
    (the same positions for arrays of the same size) and those positions as DIR/<name>.index.npy (float64)."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    # a sampled element costs its own bytes + 8 for its position
    frac = 1.0 if total <= limit else limit / float(sum(a.size * (a.itemsize + 8) for a in arrays.values()))
    for name, a in arrays.items():
        if frac < 1.0:
            keep = int(a.size * frac)
            pos = np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))
            np.save(os.path.join(dirname, name + ".index.npy"), pos.astype(np.float64))
            a = a.reshape(-1)[pos]
        np.save(os.path.join(dirname, name + ".npy"), a)


def cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("model name"):
                    return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def physical_cores():
    """Distinct (package, core) pairs of /proc/cpuinfo, capped by this process's affinity mask."""
    cores = set()
    try:
        pkg = core = None
        with open("/proc/cpuinfo") as f:
            for ln in f:
                if ln.startswith("physical id"):
                    pkg = ln.split(":")[1].strip()
                elif ln.startswith("core id"):
                    core = ln.split(":")[1].strip()
                elif not ln.strip():
                    if pkg is not None and core is not None:
                        cores.add((pkg, core))
                    pkg = core = None
    except OSError:
        pass
    n = len(cores) or (os.cpu_count() or 1)
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    return max(n, 1)


def cpu_baseline(net, cfg, vc_np, feats_np, batch, gpu_out=None):
    """The oracle's WHOLE forward of the same frame(s) on the host, first on all physical cores (OpenMP
    loops of the C oracle + torch-CPU dense math), then on one thread.  Its output doubles as a parity check of
    the frame just benchmarked (outside the timed region; the oracle is the checker, never the product)."""
    import numpy as np
    from mssvt_amd import synthetic
    from oracle import block_ref, cref
    params = [dict(p) for p in cfg.MODEL.BACKBONE_3D.PARAMS]
    sd = {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}
    keep = torch.get_num_threads()
    cores = physical_cores()
    runs = {}
    want = None
    try:
        for tag, nt in (("all_cores", cores), ("one_thread", 1)):
            torch.set_num_threads(nt)
            cref.set_num_threads(nt)
            t0 = time.perf_counter()
            want = block_ref.backbone_forward(sd, params, feats_np, vc_np, batch, synthetic.GRID_SIZE,
                                              synthetic.VOXEL_SIZE, synthetic.POINT_CLOUD_RANGE,
                                              int(cfg.MODEL.BACKBONE_3D.HASH_SIZE))
            runs[tag] = time.perf_counter() - t0
    finally:
        torch.set_num_threads(keep)
        cref.set_num_threads(0)
    res = {"value": batch / runs["all_cores"], "unit": "frames/s", "cores": cores, "kind": "port",
           "one_thread_value": batch / runs["one_thread"], "cpu_model": cpu_model(), "host_cpus": os.cpu_count(),
           "sample": "CPU oracle (C/OpenMP + torch-CPU port of the reference CUDA semantics; the reference has no CPU "
                     "path): the WHOLE forward of the same %d frame(s), %.1f s on %d cores (the numpy glue between the "
                     "kernels is single-threaded), %.1f s on one thread" % (batch, runs["all_cores"], cores,
                                                                            runs["one_thread"])}
    if gpu_out is not None and want is not None:
        got = gpu_out.features.float().cpu().numpy()
        same_idx = bool(np.array_equal(gpu_out.indices.cpu().numpy(), want.indices))
        err = float((np.abs(got - want.features) / np.maximum(1.0, np.abs(want.features))).max()) if same_idx else None
        res["parity_of_the_benchmarked_frame"] = {"indices_bit_exact": same_idx, "max_scaled_feature_err": err}
    return res


_ARITH_TEXT = {
    "split16": "fp32 operands as two fp16 halves (hi + 2^-11 lo: 22 of 24 mantissa bits, the lo x lo term dropped), 3 x "
               "v_mfma_f32_16x16x32_f16, fp32 accumulate",
    "f32": "v_mfma_f32_16x16x4_f32", "bf16": "bf16 operands, fp32 accumulate (v_mfma_f32_16x16x32_bf16), one launch"}


def arith_of(net):
    """(attn_arith, ffn_arith, per-block list): the arithmetic the blocks RAN on -- the outcome of the fp16-range guards on
    the parameters as they are (mssvt_amd/fused.py::arith_report), not the policy."""
    from mssvt_amd import fused
    rep = fused.arith_report(net)

    def name(key, blocks):
        kinds = sorted({b[key].split(" (")[0] for b in blocks})
        txt = " + ".join(_ARITH_TEXT.get(k, k) for k in kinds)
        return "%s: %s" % (" / ".join(kinds), txt) if kinds else None
    body = [b for b in rep[:-1]] if len(rep) > 1 else rep
    return name("attn", body), name("ffn", rep), rep


def workload_name(args, cfg_given):
    if args.train and getattr(args, "detector", False):
        return ("CenterPoint detector training step (mssvt.yaml: DynamicVFE + MsSVT backbone + BEV backbone + CenterHead), %d-point "
                "scenes x batch %d per GPU with 12 synthetic boxes each, fp32, forward + loss + backward + all-reduce + SGD%s"
                % (args.points, args.batch, ", SyncBatchNorm" if args.sync_bn else ""))
    if cfg_given:
        return "%s: %d-point scene x batch %d per GPU" % (os.path.basename(args.cfg), args.points, args.batch)
    base = ("%d-point Waymo-shaped scene x batch %d per GPU, full mssvt.yaml backbone (4 Blocks [3,3,5]/[7,7,7] cbs "
            "1,0,1,0 + CompressBlock [1,1,32], C=128, heads [4,4], HASH_SIZE 400000)" % (args.points, args.batch))
    if args.train:
        return "BASELINE configs[3] (DDP training reading): " + base + ", fp32, forward + backward + all-reduce + SGD"
    if args.attn_dtype == "bf16":
        tag = "BASELINE configs[2]" if (args.batch == 8 and args.points == 160000) else "configs[2] kernels"
        return tag + ": " + base + ", bf16-operand MFMA window attention (fp32 accumulate / softmax / FFN)"
    if args.gpus > 1 and args.batch == 4:
        return "BASELINE configs[3]: " + base + ", fp32"
    return "BASELINE configs[1]: " + base + ", fp32"


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))  # before any GPU call of this process
    from mssvt_amd import dist as mdist
    rank, world, local_rank = mdist.env_rank_world()
    if "WORLD_SIZE" in os.environ and world != args.gpus:
        # under a launcher (torchrun ... bench.py without --gpus) the environment is authoritative
        if args.gpus != 1:
            print("bench.py: --gpus %d but WORLD_SIZE=%d: following the launcher" % (args.gpus, world), file=sys.stderr)
        args.gpus = world
    assert torch.cuda.is_available(), "bench.py needs an MI355X (the hot path has no CPU fallback)"
    # MSSVT_BENCH_ONE_DEVICE=1 (debugging the N > 1 code path on a single-GPU box): every rank on cuda:0, gloo
    one_dev = os.environ.get("MSSVT_BENCH_ONE_DEVICE", "0") == "1"
    dev = torch.device("cuda", 0 if one_dev else local_rank)
    torch.cuda.set_device(dev)
    backend = "gloo" if one_dev else "nccl"
    dist = mdist.init(backend, dev)
    seen_world = dist.get_world_size() if dist else 1

    from mssvt_amd import config, roofline
    torch.manual_seed(0)
    cfg = config.load_yaml(args.cfg) if args.cfg else config.load_yaml(config.DEFAULT_CFG)
    net = config.build_backbone_from_cfg(cfg).to(dev)
    if args.impl:
        net.set_impl(args.impl)
    net.set_attn_dtype(args.attn_dtype)
    if args.ffn_arith:
        from mssvt_amd import fused as _fused
        _fused.FFN_ARITH = args.ffn_arith
    if args.arith == "f32":
        from mssvt_amd import fused as _fused
        _fused.FFN_ARITH = "f32"  # FFN tails + CompressBlock products
        _fused.ATTN_KV16 = _fused.ATTN_QO16 = False  # k_attn_q / k_attn_kv / k_attn_o on v_mfma_f32_16x16x4_f32
    # the steps rotate over `--frames` different frames, all resident in HBM before the timed region: replaying ONE frame
    # from the same addresses would keep its 38 MB of input in the Infinity Cache, which a stream of frames does not
    frames = [make_inputs(args.points, args.batch, rank, dev, frame=f) for f in range(max(args.frames, 1))]
    vc_np, feats_np, vc, feats = frames[0]
    turn = [0]

    def next_frame():
        f = frames[turn[0] % len(frames)]
        turn[0] += 1
        return f[2], f[3]

    step_alone = pipe = None
    det = None
    if args.train and args.detector:
        # the reference's training wrap (tools/train.py:118-119,143-144): SyncBatchNorm conversion of EVERY BatchNorm layer
        # (DynamicVFE's BatchNorm1d, the BEV backbone's and the head's BatchNorm2d), then DDP around the whole model
        from mssvt_amd import centerpoint, detector_data
        torch.manual_seed(0)
        det = centerpoint.build_detector(cfg).to(dev)
        det.backbone_3d.load_state_dict(net.state_dict())
        if args.impl:
            det.backbone_3d.set_impl(args.impl)
        if args.sync_bn:
            det = torch.nn.SyncBatchNorm.convert_sync_batchnorm(det)
        det.train()
        ddp = det
        if dist:
            ddp = torch.nn.parallel.DistributedDataParallel(det, device_ids=None if one_dev else [dev.index])
        opt = torch.optim.SGD(det.parameters(), lr=1e-4)
        scenes = [detector_data.make_scene(args.points, args.batch, rank, dev, frame=f) for f in range(max(args.frames, 1))]
        net = det.backbone_3d

        def step():
            opt.zero_grad(set_to_none=True)
            pts_, gt_ = scenes[turn[0] % len(scenes)]
            turn[0] += 1
            ret, tb, _ = ddp(dict(points=pts_, batch_size=args.batch, gt_boxes=gt_))
            ret["loss"].backward()  # gradients all-reduced here
            opt.step()
            return dict(ret, encoded_spconv_tensor=None)
    elif args.train:
        net.train()
        ddp = net
        if dist:
            ddp = torch.nn.parallel.DistributedDataParallel(net, device_ids=None if one_dev else [dev.index])
        opt = torch.optim.SGD(net.parameters(), lr=1e-4)

        def step():
            opt.zero_grad(set_to_none=True)
            vc_, feats_ = next_frame()
            out = ddp(dict(voxel_features=feats_, voxel_coords=vc_, batch_size=args.batch))
            out["encoded_spconv_tensor"].features.square().mean().backward()  # gradients all-reduced here
            opt.step()
            return out
    else:
        net.eval()

        def step_alone():
            vc_, feats_ = next_frame()
            with torch.no_grad():
                return net(dict(voxel_features=feats_, voxel_coords=vc_, batch_size=args.batch))
        step = step_alone
        if args.in_flight > 1 and not args.from_points:
            from mssvt_amd.pipeline import FramePipeline
            pipe = FramePipeline(net, depth=args.in_flight, device=dev)

            def step():
                vc_, feats_ = next_frame()
                # (the frames are resident and complete before the timed region: nothing on this stream to wait for)
                # (deferred: the frame's one host wait happens when its stream comes round again, not between two submissions)
                return pipe(dict(voxel_features=feats_, voxel_coords=vc_, batch_size=args.batch), inputs_ready=True, defer=True)
            for _ in range(args.in_flight):  # every stream's frame object and workspace exist before anything is timed
                step()
            pipe.synchronize()
    points_line = None
    if args.from_points and not args.train:
        import numpy as np
        from mssvt_amd import synthetic
        from mssvt_amd.dist import scene_seeds
        from mssvt_amd.dynamic_vfe import DynamicVFE
        from mssvt_amd.height_compression import HeightCompression
        torch.manual_seed(1)
        vfe = DynamicVFE(cfg.MODEL.VFE, 5, synthetic.VOXEL_SIZE, synthetic.GRID_SIZE, synthetic.POINT_CLOUD_RANGE).to(dev).eval()
        to_bev = HeightCompression(config.Config.wrap(dict(NUM_BEV_FEATURES=128, COMPRESS_LAYER_NUMS=0))).to(dev).eval()
        clouds = [torch.from_numpy(synthetic.make_batch_points(
            args.points, args.batch, seed0=scene_seeds(rank, args.batch)[0] + 7919 * f)).to(dev) for f in range(len(frames))]

        def step_points():
            pts = clouds[turn[0] % len(clouds)]
            turn[0] += 1
            with torch.no_grad():
                bd = vfe(dict(points=pts, batch_size=args.batch))
                bd = net(bd)
                return to_bev(bd)
        step = step_alone = step_points
        if args.in_flight > 1:  # the pipeline around the whole chain: VFE and BEV on the frame's stream, the backbone's host wait deferred
            from mssvt_amd.pipeline import FramePipeline
            pipe = FramePipeline(net, depth=args.in_flight, device=dev, pre=vfe, post=to_bev)

            def step():
                pts = clouds[turn[0] % len(clouds)]
                turn[0] += 1
                return pipe(dict(points=pts, batch_size=args.batch), inputs_ready=True)
            for _ in range(args.in_flight):
                step()
            pipe.synchronize()
        with torch.no_grad():
            bd0 = vfe(dict(points=clouds[0], batch_size=args.batch))
        n_vox, n_pts = int(bd0["voxel_coords"].shape[0]), int(clouds[0].shape[0])
        # algorithmic bytes of the two neighbours: the point rows read once + the voxel coordinates and the voxel feature rows
        # written (nothing requires the per-point layer outputs x1 / x2 or the point -> voxel index in memory: they are
        # intermediates of this implementation and are NOT counted -- round 5 counted them and flattered its fraction); the
        # dense (B, C, Z, Y, X) grid written once + the output rows read
        f_out = list(cfg.MODEL.VFE.NUM_FILTERS)
        vfe_bytes = n_pts * 4.0 * clouds[0].shape[1] + n_vox * (16.0 + 4.0 * f_out[-1])
        by_bb, _, _ = roofline.frame_algorithmic(net, bd0["voxel_coords"], bd0["voxel_features"], args.batch)
        points_line = dict(points=n_pts, voxels=n_vox, vfe_bytes=vfe_bytes, backbone_bytes=by_bb)
    impl = net.backbone[0].impl
    # which host path issued the timed frames: the whole-frame C call (mssvt_amd/frame.py) or the Python-driven path
    from mssvt_amd import frame as _frame
    host_calls = []
    _real_frame_forward = _frame.forward

    def _spy(*a, **k):
        r = _real_frame_forward(*a, **k)
        host_calls.append(r is not None)
        return r
    _frame.forward = _spy

    for _ in range(args.warmup):
        step()
    if host_calls:
        _frame.forward = _real_frame_forward  # (nothing extra inside the timed region; without warm-up steps the spy stays: ~1 us)
    host_path = lambda: ("mssvt_frame_forward: one C call per frame, persistent workspace (mssvt_amd/frame.py)"  # noqa: E731
                         if host_calls and all(host_calls) else "Python-driven entry points (mssvt_amd/fused.py)")
    # (with frames in flight a "sync" also finishes the host side of every submitted frame: the K steps are complete frames)
    full_sync = (lambda: (pipe.synchronize(), torch.cuda.synchronize())) if pipe is not None else None
    if pipe is not None:
        pipe.synchronize()
    elapsed, out = mdist.timed_steps(step, args.steps, dist, dev, sync=full_sync)
    if args.dump_outputs and rank == 0:  # before anything else runs on the frames' workspaces
        points_in = (args.from_points and not args.train) or (args.train and args.detector)
        inputs = {"points", "batch_size", "gt_boxes"} if points_in else {"voxel_features", "voxel_coords", "batch_size"}
        dump_outputs(output_arrays(out, inputs), args.dump_outputs)
    one = step_alone or step
    times = alone = live = None
    std = rank == 0 and impl == "fused" and not args.cfg and not args.train and not args.from_points
    if args.full:
        # SURVEY 8(d) protocol beside the driver's K-step clock: every step between two HIP events
        # (a training step is collective -- every rank takes part; the forward is not, rank 0 measures alone)
        # (one frame at a time on one stream: a step's duration = its latency; the pipelined steps overlap)
        times = per_step_times_ms(one, max(50, args.steps)) if (rank == 0 or args.train) else None
        if step_alone is not None and step is not step_alone and rank == 0:
            for _ in range(3):
                step_alone()
            alone, _ = mdist.timed_steps(step_alone, args.steps, None, dev)
        # live roofline: the same K steps once more on rank 0 with HIP events around every launch of the
        # dominant kernel (kept out of the timed region above: the event markers cost ~3 % of the frame rate)
        if std and not args.no_roofline:
            from mssvt_amd import fused
            fused.FFN_TIMER = []
            for _ in range(args.steps):
                one()
            torch.cuda.synchronize()
            live = fused.ffn_timer_summary(fused.FFN_TIMER)
            fused.FFN_TIMER = None

    if rank == 0:
        sp_out = None
        if args.train:
            sp_out = out["encoded_spconv_tensor"]
        elif args.full or points_line is not None:
            # frame 0 once more (outside every timed region): the output cpu_baseline checks against the oracle and the
            # --from-points byte count reads
            turn[0] = 0
            out = one()
            torch.cuda.synchronize()
            sp_out = out["encoded_spconv_tensor"]
        ms = 1e3 * elapsed / args.steps
        arith = arith_of(net) if not args.train else (
            "compact training path (mssvt_amd/train_path.py): pair attention on fp32 vector FMAs, linears on split-fp16 operands",
            "compact training path: split-fp16 linears (mssvt_linear_rows_h), fp32 MFMA weight gradients", None)
        n_bn = sum(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for m in det.modules()) if det is not None else 0
        n_sync = sum(isinstance(m, torch.nn.SyncBatchNorm) for m in det.modules()) if det is not None else 0
        res = {
            "metric": "frames/sec (MsSVT backbone %s, synthetic Waymo-shaped scenes)"
                      % ("DDP training step" if args.train else "forward"),
            "value": world * args.batch * args.steps / elapsed,
            "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16" if args.attn_dtype == "bf16" else "f32", "data": "synthetic",
            "config": {"workload": workload_name(args, bool(args.cfg)),
                       "impl": impl, "attn_dtype": args.attn_dtype, "attn_arith": arith[0], "ffn_arith": arith[1],
                       "arith_per_block": arith[2], "arith": args.arith, "host_path": host_path(),
                       "voxels_per_gpu": int(vc.shape[0]),
                       "frames_in_flight": 1 if (args.train or args.in_flight <= 1) else args.in_flight,
                       "streams": None if (args.train or args.in_flight <= 1) else {
                           "priority": "one high-priority framework stream per frame in flight (mssvt_amd/pipeline.py)",
                           "cumask": "one HIP stream per frame in flight, each on a hardware queue of its own (CU-mask streams)",
                           "pooled": "one pooled HIP stream per frame in flight"}[pipe.stream_kind],
                       "frames_rotated": len(frames), "voxels_per_frame": [int(f[2].shape[0]) for f in frames],
                       "output_voxels": int(sp_out.features.shape[0]) if sp_out is not None else None,
                       "detector": None if det is None else {
                           "model": "CenterPoint: DynamicVFE -> MixedScaleSparseTransformer -> HeightCompression -> BaseBEVBackbone -> "
                                    "CenterHead (targets + losses), the whole model under DDP", "loss": float(out["loss"]),
                           "batch_norm_layers": n_bn, "sync_batch_norm_layers": n_sync},
                       "parallelism": "scenes sharded over %d GPU(s), %s" % (
                           world, "DDP gradient all-reduce (%s)" % backend if args.train else "no data-path collective"),
                       "process_group": {"backend": backend if dist else None, "world_size": seen_world}},
        }
        if times is not None:
            res["timing"] = {"protocol": "each of %d further steps between two HIP events on the launching stream" % len(times),
                             "median_ms": times[len(times) // 2], "p10_ms": times[len(times) // 10],
                             "p90_ms": times[(len(times) * 9) // 10], "frames_per_s_at_median":
                                 args.batch / (times[len(times) // 2] * 1e-3)}
        if points_line is not None:
            bev = out["spatial_features"]
            dense_bytes = 4.0 * bev.numel() + 4.0 * sp_out.features.numel()
            tot = points_line["vfe_bytes"] + points_line["backbone_bytes"] + dense_bytes
            res["metric"] = "frames/sec (points -> voxelizer + DynamicVFE -> MsSVT backbone -> dense BEV, synthetic Waymo-shaped scenes)"
            res["config"]["workload"] = "points -> BEV (SURVEY 8 f1 + path + f2): " + res["config"]["workload"]
            res["from_points"] = dict(points_line, dense_bytes=dense_bytes, algorithmic_bytes=tot,
                                      hbm_floor_us=tot / (HBM_PEAK_GBS * 1e9) * 1e6,
                                      frac=tot / (HBM_PEAK_GBS * 1e9) * 1e3 / ms, bev_shape=list(bev.shape),
                                      note="DynamicVFE: device voxelizer (bitmap + popcount rank), points grouped by voxel, both PFN "
                                           "layers and their reductions in csrc/pfn_sorted.hip (ref dynamic_vfe.py:71-131); dense(): "
                                           "k_dense_bev4 (ref mssvt_utils.py:50-62, height_compression.py:41-50); frac = algorithmic "
                                           "bytes (VFE: point rows in, voxel coordinates + feature rows out -- no intermediates; "
                                           "backbone: SURVEY 8(d); dense: grid out + rows in) at 8 TB/s against ms_per_step")
        if alone is not None:
            res["one_frame_in_flight"] = {
                "value": args.batch * args.steps / alone, "ms_per_step": 1e3 * alone / args.steps,
                "note": "the same %d steps one at a time on one stream (what rounds 1-4 reported as value); the headline keeps %d "
                        "independent frames in flight, each on its own HIP stream and workspace (mssvt_amd/pipeline.py; every "
                        "frame bit-identical to the frame run alone: tests/test_pipeline_gpu.py)" % (args.steps, args.in_flight)}
        if std and args.full and not args.no_roofline:
            res["roofline"] = roofline.measure(net, vc, feats, args.batch, event_time_ms, HBM_PEAK_GBS, live=live,
                                               ms_per_step=ms)
        if std and args.full and not args.no_cpu_baseline and world == 1:
            res["cpu_baseline"] = cpu_baseline(net, cfg, vc_np, feats_np, args.batch, gpu_out=sp_out)
        print(json.dumps(res), flush=True)
    if pipe is not None:
        pipe.close()  # (workspaces back; the streams live until the process ends)
    if dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
