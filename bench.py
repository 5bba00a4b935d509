"""Benchmark of the geodesic ray-tracing hot path (BASELINE.json metric) on MI355X.

One "step" = one camera frame of the workload traced by libbhrt.so with every input already
on the device: the frame kernel launch, plus (N > 1) the frame's single RCCL collective and
its assembly on rank 0 (bhrt/dist_frame.py FramePipeline; the collective of frame i overlaps
the rendering of frame i+1, and the timed region ends after the last one). Consecutive frames
alternate between HIP streams, so the workgroups of frame i+1 take the CUs that frame i's tail
-- its last, longest rays draining -- leaves idle (tools/wave_tail.py: ~9% of a lone C2
launch): two streams, or four for short frames (--streams auto, the default: a frame under
0.6 ms, or too few rays to fill the chip's resident waves); --streams 1 runs them back to back.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--config C2] [--camera B]
                  [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K frames, writes the last timed frame with
--dump-outputs, and prints the JSON line: the headline rate with the figures that come out of
the timed frames themselves (kernel, roofline, dist). --full adds the legs that take runs of
their own after the timed frames: the display-only resident frames, the host-buffer frames and
batch calls (one of them in a fresh child process), and the CPU baseline with its parity check.

N > 1 is launched by torch.distributed.run, one process per GPU. Every frame is an image
split into cyclic row-block shards (block b -> shard b % S); rank r renders shard r and rank 0
assembles the colour image of the rendered shards from ONE RCCL gather (configs.Config.frame,
bhrt/dist_frame.py):
  * C5 (weak, "weak-shards"): the BASELINE 7680 x 4320 frame in 8 shards of 540 rows (cyclic
    6-row blocks). N GPUs render shards 0..N-1: N = 1 is shard 0, N = 8 the whole image.
  * C1-C3 (weak, "weak-tiles"): N x the configuration's pixels at its aspect and field of view
    (C2: 1920x1080 at N = 1, 2716x1528, 3840x2160, 5433x3056 at N = 2, 4, 8), N shards, so
    every GPU keeps one configuration frame's worth of rays.
  * C4 (strong): the one 3840 x 2160 image in N shards.
  --weak-mode samples (opt-in, C1-C3) instead supersamples the configuration frame: rank k
  traces it at the reference's Halton sub-pixel offset k and one RCCL reduce averages the
  colour (trace_pixel's sample average, raytracer.c:1096-1164).

--dump-outputs DIR writes what the last timed frame left on rank 0, as DIR/<field>.npy: every
field of its per-ray SoA (float64; rgba8 as float32 [rays, 4]) and, at N > 1, the gathered
image fields as DIR/image_<field>.npy. Above DUMP_BUDGET_BYTES in all, the same seeded sample
of rays is written for every field, its flat ray indices as DIR/sample_index.npy. The frame is
synthetic and deterministic, so two builds run with the same arguments compare ray for ray.

The JSON line also carries (cpu_baseline with --full only):
  roofline      FP64 VALU roofline of the trace kernel: algorithmic FLOPs (SURVEY.md 8(a):
                117 per RK4 iteration + 35 per a=0 derivative stage + 4 per far-field stage;
                368 per RKF45 attempt + the same stage costs; a Kerr stage's accelerations are
                identically zero, so the 3 velocity components it feeds are not credited:
                flops()) / the kernel's GPU time per launch: with overlapping frames the
                HIP-event busy span of the timed launches (first start to last end) /
                launches, else the per-launch HIP-event average. With a committed PMC
                summary (profiles/pmc_<config>.json) also the ISSUED FP64 rate: (2 FMA + MUL +
                ADD + TRANS) f64 wave instructions x 64 lanes per launch / the same duration.
  cpu_baseline  the compiled reference (oracle/_ref/libref.so, unmodified trace_ray under an
                OpenMP loop) on a row sample of the same frame, rank 0 at N = 1 only; its
                sampled rows double as the parity check "max |dhit|".
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))


def _launch_ranks():
    """`python bench.py --gpus N` (N > 1) with no launcher around it: start the N rank
    processes here, one per GPU, through torch.distributed.run (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set for every child), and exit with the
    launcher's exit code (the worst rank's). Rank 0's JSON line reaches stdout through the
    inherited descriptor. This runs BEFORE torch or libbhrt is imported: the parent never
    touches a GPU, so no process that initialised HIP ever starts another program. Returns
    only when no launch is needed (N = 1, or a launcher already set WORLD_SIZE)."""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--gpus", type=int, default=1)
    n = p.parse_known_args()[0].gpus
    if n <= 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={n}", "--master-addr=127.0.0.1", f"--master-port={port}",
           os.path.abspath(__file__), *sys.argv[1:]]
    rc = subprocess.call(cmd, env=dict(os.environ))
    if os.environ.get("BHRT_BENCH_DRYRUN"):  # tests: did this process ever load HIP?
        with open("/proc/self/maps") as f:
            hip = "libamdhip64" in f.read()
        print(json.dumps({"launcher": True, "rc": rc, "hip_loaded": hip,
                          "torch_imported": "torch" in sys.modules}), flush=True)
    sys.exit(rc)


if __name__ == "__main__":
    _launch_ranks()

# Hardware queues per process (HIP runtime knob, read when HIP initialises; the box's default is
# 4). Every HIP stream is bound to one queue, streams beyond the count share queues round robin,
# and work on one queue runs in order: with the torch default stream, the two render streams and
# RCCL's stream of an N-GPU run, a shared queue would put a frame's gather behind the next
# frame's trace kernel. 8 gives each of them a queue of its own.
# The effective value is recorded in the JSON line ("runtime"); BHRT_BENCH_HW_QUEUES=default
# keeps the runtime's own setting (the stock 4 on the box), for the rate a default-configured
# renderer process gets.
HWQ_ASKED = os.environ.get("GPU_MAX_HW_QUEUES")


def _hw_queues_wanted():
    """8, or 16 with more than four render streams (--streams 5..8): one queue per stream"""
    a = sys.argv[1:]
    for i, v in enumerate(a):
        n = v.split("=", 1)[1] if v.startswith("--streams=") else (
            a[i + 1] if v == "--streams" and i + 1 < len(a) else None)
        if n is not None and n.isdigit() and int(n) > 4:
            return 16
    return 8


if (os.environ.get("BHRT_BENCH_HW_QUEUES") != "default" and
        int(os.environ.get("GPU_MAX_HW_QUEUES", "0") or 0) < _hw_queues_wanted()):
    os.environ["GPU_MAX_HW_QUEUES"] = str(_hw_queues_wanted())

sys.path.insert(0, os.path.join(ROOT, "raytracing-engine-in-c_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from bhrt import abi, configs, lib  # noqa: E402
from bhrt.dist_frame import (DISPLAY_FIELD, RGB_FIELDS, FramePipeline,  # noqa: E402
                             padded_shard_rows, sample_offset, shard_row_count)

FP64_PEAK_TFLOPS = 78.6  # MI355X FP64 vector (and FP64 matrix) peak, AMD spec
METRIC = "Mrays/s (and RK4 steps/s) per GPU + per node; max |Δhit| vs CPU ref"
FIELDS = abi.SOA_FIELDS
# CPU-baseline row sample per config: ~1-3 s wall of the compiled reference on the GPU box's
# 16 host cores (15-50 core-seconds)
CPU_ROWS_STRIDE = {"C1": 1, "C2": 27, "C3": 27, "C4": 4, "C5": 3}
# --streams auto: four frames in flight instead of two when a frame is short or small. Same-box
# A/B (profiles/r04/session_f_streams/run2_warmed.txt): 4 streams C1 +6.5%, C3 +4.5%, the C4 8-GPU-plan
# shard 0.186 -> 0.157 ms; C2 -1%, C4 full frame -1%, C5 -2%.
AUTO_SHORT_MS = 0.6
# Sustained load right before the timed frames ("Clock ramp"): after an
# idle gap of a few ms the GPU's frame time falls over ~30 ms of continuous work (C4 one stream
# 1.20 -> 0.95 ms per frame, profiles/r05/clock_ramp.txt), so the untimed frames end with this
# many ms of back-to-back frames and the timed region follows after one sync.
WARM_MS = float(os.environ.get("BHRT_BENCH_WARM_MS", "200"))
AUTO_FILL_RAYS = 256 * 4 * 4 * 64  # 4 waves per SIMD x 4 SIMDs x 256 CUs x 64 lanes
# --dump-outputs: at most this many bytes of .npy data in all (a seeded ray sample above it)
DUMP_BUDGET_BYTES = 48 << 20
DUMP_SEED = 0


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--config", default="C2")
    p.add_argument("--camera", default="B")
    p.add_argument("--refill", type=int, default=None)
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed frames, write the last one as DIR/<field>.npy (rank "
                        "0's per-ray SoA, float64 / float32; at N > 1 also the gathered "
                        "image_<field>.npy), at most DUMP_BUDGET_BYTES in all: above that a "
                        "seeded sample of the rays, indices in DIR/sample_index.npy")
    p.add_argument("--full", action="store_true",
                   help="after the timed frames also run the side legs: display-only resident "
                        "frames, host-buffer frames and batch calls, the CPU baseline and its "
                        "parity check (--no-host-path / --no-cpu-baseline leave one out)")
    p.add_argument("--cpu-rows-stride", type=int, default=None,
                   help="--full: CPU baseline samples every k-th row of the rendered shard "
                        "(default per config, ~1-3 s on 16 cores: CPU_ROWS_STRIDE)")
    p.add_argument("--no-cpu-baseline", action="store_true",
                   help="--full without the CPU baseline")
    p.add_argument("--no-host-path", action="store_true",
                   help="--full without the host-buffer frames and the display-only resident "
                        "frames (their launches would mix into a profiler's per-launch kernel "
                        "averages)")
    p.add_argument("--fields", choices=("all", "display"), default="all",
                   help="what each timed frame writes: every SoA field + rgba8 (100 B/ray, "
                        "default; the CPU baseline compares them) or the visualizer's display "
                        "call, rgba8 alone (plus result / hit_x / hit_y where the colour is a "
                        "separate pass: Config.display_fields)")
    p.add_argument("--streams", default="auto",
                   help="consecutive frames alternate between this many HIP streams (1-4; "
                        "one frame buffer each), so the next frames' rays fill the CUs the tail "
                        "of the current frame frees; auto (default): 2, or 4 when calibration "
                        "frames after the warm-up take under AUTO_SHORT_MS or the frame has "
                        "fewer rays than AUTO_FILL_RAYS")
    p.add_argument("--claim-order", choices=("default", "prev-tiles"), default="default",
                   help="prev-tiles (opt-in): camera frames claim their 64-ray tiles longest "
                        "first by the previous frame's steps (bhrt_set_claim_order; a renderer's "
                        "temporal-coherence order -- optimistic here, where every frame is the "
                        "same image)")
    p.add_argument("--weak-mode", choices=("tiles", "samples"), default="tiles",
                   help="weak configs at N GPUs: tiles = N shards of a frame (default); "
                        "samples = N sub-pixel sample planes of the configuration frame "
                        "(C1-C3), colour averaged by one reduce")
    p.add_argument("--sample", type=int, default=None,
                   help="samples mode: trace sample plane K instead of this rank's (to time "
                        "each plane of an N-GPU run on one GPU)")
    p.add_argument("--shard", type=int, default=None,
                   help="tiles mode, N = 1: render shard K of the frame instead of shard 0 "
                        "(to time every shard of a node frame on one GPU)")
    p.add_argument("--plan-gpus", type=int, default=None,
                   help="N = 1 only: render a shard (--shard K, default 0) of the frame the "
                        "N-GPU run renders (configs.Config.frame(N): C2 at 8 is the 5433x3056 "
                        "frame in 8 shards, C4 the 3840x2160 image in 8, C5 its 8 shards), so "
                        "every rank's work of an N-GPU run can be timed on one GPU "
                        "(tools/plan_shards.sh)")
    p.add_argument("--batch-fresh-child", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--gather", choices=("rgba8", "image", "all"), default="rgba8",
                   help="fields gathered to rank 0 at N > 1: the rgba8 display buffer the "
                        "colour pass writes (4 B/ray, default), the f64 colour planes "
                        "(24 B/ray) or every SoA field (96 B/ray); every rank keeps its "
                        "shard's full f64 SoA resident either way")
    return p.parse_args()


# SURVEY.md 8(a) op model. An RK4 iteration is 117 ops (96 of them the stage combinations of
# the 6 live components) + its stages' derivative costs; an RKF45 attempt 368 (347 on the
# components). A Kerr stage sets d3..d5 = 0 (raytracer.c:131-138), so the combinations of the
# 3 velocity components it feeds (y + h * sum(b * 0)) are not work: each stage that is NOT a
# Kerr stage adds its share of those (96 / 2 / 4 = 12 per RK4 stage, 347 / 2 / 6 = 29 per
# RKF45 stage); the other half stays in the per-iteration base (69 and 194).
# Where EVERY stage is a Kerr stage (a != 0 without the far-field branch: C4, C5), the stage
# derivatives of components 0..2 are the ray's constant velocities, so their stage states are
# never read and their weighted stage sums are per-ray constants: only what each iteration
# must form from them is credited -- y + h * sum per component (2 ops; RKF45: y4 and y5, 4),
# RKF45's error, scale and quotient (7 per component) -- plus the 21 ops outside the
# components: 27 per RK4 iteration, 54 per RKF45 attempt. An RKF45 attempt that the host proved
# cannot be rejected (bhrt_stats.attempts_untested, DESIGN.md 2.3: C5) forms no y4, error, scale
# or quotient: y5 = y + h * sum (2 per component) plus the same 21, 27 like an RK4 iteration.
ZERO_ACCEL_OPS = {False: 27, True: 54}
ZERO_ACCEL_UNTESTED_OPS = 27


def flops(st, method):
    rkf = method == abi.INTEGRATOR_RKF45
    per_iter = 6 if rkf else 4
    if st["iterations"] > 0 and st["stages_kerr"] == per_iter * st["iterations"]:
        untested = st.get("attempts_untested", 0) if rkf else 0
        return (ZERO_ACCEL_OPS[rkf] * (st["iterations"] - untested) +
                ZERO_ACCEL_UNTESTED_OPS * untested)
    base, per_live_stage = (194, 29) if rkf else (69, 12)
    live = st["stages_full"] + st["stages_far"]
    return (base * st["iterations"] + per_live_stage * live + 35 * st["stages_full"] +
            4 * st["stages_far"])


def main():
    args = parse()
    if args.batch_fresh_child:
        return batch_fresh_child(args)
    if not args.full:  # a plain run: the timed frames only, none of the side legs
        args.no_host_path = args.no_cpu_baseline = True
    world =int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    auto = args.streams == "auto"
    if not auto and args.streams not in ("1", "2", "3", "4", "5", "6", "7", "8"):
        raise SystemExit("--streams must be 1..8 or auto")
    nstreams = 2 if auto else int(args.streams)  # FramePipeline keeps one buffer slot per stream
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # rehearsal of the N-GPU path on a one-GPU box: every rank on GPU 0, gloo collectives
    # (RCCL refuses two ranks on one device); the product N-GPU run never sets this
    shared = os.environ.get("BHRT_BENCH_SHARE_DEVICE") == "1"
    if os.environ.get("BHRT_BENCH_DRYRUN"):  # tests: the rank environment, no GPU call
        print(json.dumps({"rank": rank, "local_rank": local, "world_size": world,
                          "master_addr": os.environ.get("MASTER_ADDR"),
                          "master_port": os.environ.get("MASTER_PORT"),
                          "device": 0 if shared else local}), flush=True)
        return
    c0 = configs.CONFIGS[args.config]
    fresh = None
    if (world == 1 and not args.no_host_path and args.fields == "all" and
            c0.method == abi.INTEGRATOR_RK4 and c0.frame(1).shards == 1 and args.shard is None and
            args.plan_gpus is None):
        # the drop-in batch API as the FIRST GPU work of a fresh process,
        # started before this process touches the GPU
        fresh = batch_fresh_rate(args)
    dev_index = 0 if shared else local
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        # RCCL times each collective on its own stream (Work.get_duration): the gather's GPU
        # time per frame goes into the JSON line ("dist")
        os.environ.setdefault("TORCH_NCCL_ENABLE_TIMING", "1")
        if shared:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)
    L = lib.load()
    if args.refill:
        L.bhrt_set_refill_threshold(args.refill)

    c = configs.CONFIGS[args.config]
    bh, dk, cfg = c.scene()
    cam = configs.camera(args.camera)
    samples = args.weak_mode == "samples" and c.scaling != "strong"
    plan_n = world
    if args.plan_gpus is not None:
        if world != 1 or samples or args.plan_gpus < 1:
            raise SystemExit("--plan-gpus N times one shard of the N-GPU plan at --gpus 1")
        plan_n = args.plan_gpus
        if args.shard is not None and not 0 <= args.shard < c.frame(plan_n).shards:
            raise SystemExit(f"--shard {args.shard}: the {plan_n}-GPU plan has "
                             f"{c.frame(plan_n).shards} shards")
    plan = c.frame(1 if samples else plan_n)
    W, H, S, B = plan.width, plan.height, plan.shards, plan.row_block
    if samples:
        if S != 1:
            raise SystemExit(f"--weak-mode samples needs a one-shard frame ({c.name} is not)")
        shard, rows, n = 0, None, W * H
        off = sample_offset(rank if args.sample is None else args.sample)
        if off is not None:
            cam.use_offset, cam.offset_x, cam.offset_y = 1, off[0], off[1]
        rays_frame = W * H * world
    else:
        shard = rank if args.shard is None or world > 1 else args.shard
        rows = plan.rows(shard)
        n = padded_shard_rows(H, B, S) * W  # this rank fills its shard_row_count rows
        rays_frame = sum(shard_row_count(H, B, r, S) for r in range(world)) * W
        if args.shard is not None and world == 1:
            rays_frame = shard_row_count(H, B, shard, S) * W
    if samples and args.gather == "rgba8":
        args.gather = "image"  # (samples mode averages the f64 colour planes)
    gather = {"all": None, "image": RGB_FIELDS, "rgba8": DISPLAY_FIELD}[args.gather]
    fields = FIELDS + DISPLAY_FIELD if args.gather == "rgba8" else FIELDS
    if args.fields == "display":
        if samples:
            raise SystemExit("--fields display: tiles mode only (samples average f64 colour)")
        fields, gather = c.display_fields(), DISPLAY_FIELD
        args.no_cpu_baseline = True  # (no hit fields to compare)
    pipe = FramePipeline(n, device, world, rank, "samples" if samples else "shards", H, W, B,
                         fields, shards=S, gather=gather, first_shard=shard - rank,
                         slots=4 if auto else nstreams)
    streams = ([torch.cuda.current_stream()] if nstreams <= 1 else
               [render_stream(device) for _ in range(4 if auto else nstreams)])
    active = [nstreams]
    frame_no = [0]

    def step():
        # Frame k renders on streams[k % S]. A persistent k_trace launch ends with a tail in
        # which its last (up to max_steps-iteration) rays drain and CUs fall idle; with S > 1
        # the next frame's workgroups take those CUs (tools/wave_tail.py measures the tail).
        # A frame buffer slot is reused `streams` frames later (two with one stream), on the
        # same stream.
        s = streams[frame_no[0] % active[0]]
        frame_no[0] += 1
        with torch.cuda.stream(s):
            fb = pipe.next_buffer()
            lib.render_frame_device(bh, dk, cfg, cam, W, H, rows, c.method, c.flags, fb.soa(),
                                    s.cuda_stream)
            pipe.submit()

    # every stream renders at least one untimed frame: a stream's first launch (its hardware
    # queue set up on first use, the slot's assembly views built) stays out of the timed region
    # even when --warmup is below --streams (then "warmup" reports the frames actually run)
    warmup = max(args.warmup, nstreams)
    for _ in range(warmup):
        step()
    pipe.finish()
    calib_ms = None
    if auto:
        # calibration: 4 frames on 2 streams (untimed); the ranks agree on the slowest
        torch.cuda.synchronize()
        tc = time.perf_counter()
        for _ in range(4):
            step()
        pipe.finish()
        torch.cuda.synchronize()
        calib_ms = (time.perf_counter() - tc) / 4 * 1e3
        if world > 1:
            t = torch.tensor([calib_ms], dtype=torch.float64,
                             device="cpu" if shared else device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            calib_ms = t.item()
        if calib_ms < AUTO_SHORT_MS or rays_frame // max(world, 1) < AUTO_FILL_RAYS:
            # four streams; slot k of the pipeline stays on stream k from here on (frame_no
            # and the pipeline's frame count advance together, and all work above is done)
            active[0] = 4
            for _ in range(4):  # each new stream's first launch, untimed
                step()
            pipe.finish()
        warmup += 4 + (4 if active[0] == 4 else 0)
    order_keep = None
    if args.claim_order == "prev-tiles" and not samples:
        order_keep = prev_tiles_order(pipe, frame_no[0] - 1, H, W, B, S, shard)
        if order_keep is not None:
            for _ in range(len(streams)):  # untimed frames in the new order
                step()
            pipe.finish()
            warmup += len(streams)
    sustained = 0
    if WARM_MS > 0:
        # (frame time from one untimed round on the active streams, then frames back to back)
        torch.cuda.synchronize()
        tw = time.perf_counter()
        for _ in range(active[0]):
            step()
        pipe.finish()
        torch.cuda.synchronize()
        est_ms = (time.perf_counter() - tw) / active[0] * 1e3
        extra = min(int(WARM_MS / max(est_ms, 1e-3)) + 1, 4000)
        if world > 1:  # every rank the same frames, started together: they end together, and
            # the barrier below leaves no rank idle for long before its timed frames
            t = torch.tensor([extra], dtype=torch.float64, device="cpu" if shared else device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            extra = int(t.item())
            dist.barrier()
        sustained = active[0] + extra
        for _ in range(extra):
            step()
        pipe.finish()
        warmup += sustained
    torch.cuda.synchronize()
    t_idle = time.perf_counter()  # the GPU is idle from here to the first timed launch
    lib.stats_discard()
    pipe.reset_timing()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    t_issue = time.perf_counter() - t0  # host time to issue the K frames (no GPU wait)
    frame = pipe.finish()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    pipe.collect_timing()  # (the collectives' own GPU time, read after the sync)
    elapsed_rank = elapsed
    st = lib.stats(reset=True)
    if world > 1:
        red = "cpu" if shared else device  # (gloo reduces host tensors)
        t = torch.tensor([elapsed], dtype=torch.float64, device=red)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
        tot = torch.tensor([st["iterations"]], dtype=torch.float64, device=red)
        dist.all_reduce(tot)
        iterations_all = tot.item()
        # per rank: trace-kernel GPU time per frame, its own wall time, the gather's GPU time
        nl = max(st["launches"], 1)
        cms = pipe.collective_ms
        mine = torch.tensor([st["span_ms"] / nl, st["kernel_ms"] / nl, elapsed_rank,
                             sum(cms) / len(cms) if cms else float("nan"), len(cms)],
                            dtype=torch.float64, device=red)
        per_rank = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(per_rank, mine)
        per_rank = torch.stack(per_rank).cpu().numpy()
    else:
        iterations_all = st["iterations"]
        per_rank = None

    if rank != 0:
        dist.destroy_process_group()
        return

    if order_keep is not None:
        lib.set_claim_order(None, 0)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, frame, world)
    rays_all =float(rays_frame) * args.steps
    mrays = rays_all / elapsed / 1e6
    launches = max(st["launches"], 1)
    kern_ms = st["kernel_ms"] / launches
    # GPU time per trace launch: the per-launch HIP-event duration when frames run one after
    # another; with frames alternating between two streams consecutive launches overlap (the
    # next frame fills the CUs the current one's tail frees) and each launch's own start..end
    # interval double-counts the overlap, so the busy span of all timed launches / launches
    span_ms = st["span_ms"] / launches
    dur_ms = span_ms if active[0] > 1 else kern_ms
    f_launch = flops(st, c.method) / launches
    achieved = f_launch / (dur_ms * 1e-3) / 1e12
    prof = pmc_profile(args.config)
    if samples:
        parallelism = (f"dp{world}: one sub-pixel sample plane of the frame per GPU ({world} "
                       "samples/pixel), one RCCL reduce of the colour planes to rank 0 per frame "
                       "(the sample average, overlapped with the next frame)")
    else:
        parallelism = (f"{'single GPU' if world == 1 else f'dp{world}'}: rank r renders shard r "
                       f"of {S} (cyclic {B}-row blocks)" +
                       ("" if world == 1 else
                        f", one {'RCCL' if dist.get_backend() == 'nccl' else dist.get_backend()} "
                        f"gather of the {args.gather} fields to rank 0 per frame "
                        "(overlapped with the next frame)"))
    out = {
        "metric": METRIC,
        "value": round(mrays, 3),
        "unit": "Mrays/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 6),
        "higher_is_better": True,
        "scaling": "strong" if c.scaling == "strong" else "weak",
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic (deterministic camera-B frame, no input data)",
        "config": {
            "workload": (f"{c.name}: {c.note}; " +
                         (f"{W}x{H} frame, sample planes 0..{world - 1}" if samples else
                          f"{W}x{H} shard {shard}/{S}" if world == 1 and S > 1 else
                          plan.note)),
            "camera": args.camera,
            "sample_plane": (rank if args.sample is None else args.sample) if samples else None,
            "width": W,
            "height": H,
            "plan_gpus": plan_n,
            "shard": None if samples else shard,
            "shards": S,
            "row_block": B,
            "rays_per_frame": rays_frame,
            "rays_per_gpu": rays_frame // world if not samples else W * H,
            "fields": list(fields),
            "parallelism": parallelism,
        },
        "rk4_steps_per_s": round(iterations_all * (1.0 / elapsed), 1),
        "per_gpu_mrays_s": round(mrays / world, 3),
        "kernel": {
            "name": "k_trace (persistent, wave refill)",
            "avg_ms": round(dur_ms, 4),
            "duration": ("busy span of the timed launches (HIP events, first start to last "
                         f"end) / launches: frames alternate between {active[0]} streams and "
                         "overlap" if active[0] > 1 else "per-launch HIP-event duration, "
                         "averaged"),
            "event_avg_ms": round(kern_ms, 4),
            "streams": active[0],
            "claim_order": args.claim_order if order_keep is not None else "default",
            "streams_policy": (f"auto: calibration frame {calib_ms:.3f} ms (4 streams under "
                               f"{AUTO_SHORT_MS} ms or under {AUTO_FILL_RAYS} rays per GPU)"
                               if auto else "fixed (--streams)"),
            "iterations_per_launch": st["iterations"] / max(st["launches"], 1),
            "host_issue_ms_per_step": round(t_issue / args.steps * 1e3, 4),
            "sustained_warmup": {"frames": sustained, "ms_asked": WARM_MS,
                                 "idle_before_timed_ms": round((t0 - t_idle) * 1e3, 3)},
            "mean_iterations_per_ray": st["iterations"] / max(st["rays"], 1),
            "frame_latency_ms": frame_latency(st, dur_ms),
        },
        "roofline": {
            "bound": "valu-fp64",
            "achieved": round(achieved, 4),
            "peak": FP64_PEAK_TFLOPS,
            "unit": "TFLOP/s",
            "frac": round(achieved / FP64_PEAK_TFLOPS, 5),
            "flops_per_launch": f_launch,
            "traffic": prof.get("hbm_bytes_per_launch") if prof else None,
        },
    }
    if prof and "issued_fp64_flops_per_launch" in prof:
        issued = prof["issued_fp64_flops_per_launch"] / (dur_ms * 1e-3) / 1e12
        out["roofline"].update(
            issued_fp64_achieved=round(issued, 4),
            issued_fp64_frac=round(issued / FP64_PEAK_TFLOPS, 5),
            valu_issue_busy=prof.get("valu_issue_busy"),
            pmc=f"profiles/pmc_{args.config}.json")
    out["runtime"] = {
        "GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"),
        "hw_queues_set_by_bench": os.environ.get("GPU_MAX_HW_QUEUES") != HWQ_ASKED,
        "note": (f"bench.py set HIP's hardware queues per process to "
                 f"{os.environ.get('GPU_MAX_HW_QUEUES')} (8, or 16 with more than four render "
                 "streams) unless BHRT_BENCH_HW_QUEUES=default (the box's stock value is 4): with "
                 "the render streams, torch's default stream and RCCL's, 4 queues would put a "
                 "frame's collective behind the next frame's trace kernel"
                 if os.environ.get("GPU_MAX_HW_QUEUES") != HWQ_ASKED else
                 "the runtime's own hardware-queue setting (not changed by bench.py)")}
    if per_rank is not None:
        cms = per_rank[:, 3]
        out["dist"] = {
            "world_size": dist.get_world_size(),
            "backend": dist.get_backend(),
            "rccl_version": (".".join(str(v) for v in torch.cuda.nccl.version())
                             if dist.get_backend() == "nccl" else None),
            "trace_ms_per_frame": {"max": round(float(per_rank[:, 0].max()), 4),
                                   "mean": round(float(per_rank[:, 0].mean()), 4),
                                   "per_rank": [round(float(v), 4) for v in per_rank[:, 0]]},
            "rank_wall_ms_per_frame": {
                "max": round(float(per_rank[:, 2].max()) / args.steps * 1e3, 4),
                "min": round(float(per_rank[:, 2].min()) / args.steps * 1e3, 4)},
            "gather_ms_per_frame": ({"max": round(float(np.nanmax(cms)), 4),
                                     "mean": round(float(np.nanmean(cms)), 4),
                                     "per_rank": [round(float(v), 4) for v in cms]}
                                    if np.isfinite(cms).any() else None),
            "gather_timing_error": pipe.timing_error,
            "gather": (f"one {dist.get_backend()} gather of the {args.gather} fields to rank 0 "
                       "per frame, overlapped with the next frame; its GPU time from the "
                       "process group's own events (TORCH_NCCL_ENABLE_TIMING; not measured "
                       "with gloo)"),
        }
    if world == 1 and not args.no_host_path and args.fields == "all":
        out["display_resident"] = display_resident_rate(
            c, bh, dk, cfg, cam, W, H, rows, n, rays_frame, streams[:active[0]], device,
            args.steps, elapsed / args.steps * 1e3)
    if world == 1 and not args.no_host_path and S == 1:  # (bhrt_render_frame: whole images)
        out["host_path"] = host_path_rate(c, bh, dk, cfg, cam, W, H)
        if fresh is not None:
            out["host_path"]["trace_rays_batch_fresh"] = fresh
            out["host_path"]["trace_rays_batch_fresh_mrays_s"] = fresh.get("mrays_s")
    if world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"], out["max_rel_dhit"], out["class_mismatch"] = cpu_baseline(
            args, c, bh, dk, cfg, cam, frame, H)
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


def dump_outputs(directory, frame, world):
    """The last timed frame as rank 0 holds it (dist_frame.Assembled), one .npy per field:
    `local` (the per-ray SoA of rank 0's shard, every field the frame wrote) as <field>.npy and,
    at N > 1, `image` (the gathered fields, [H, W]) as image_<field>.npy. Doubles and the int32
    fields as float64 (exact), rgba8 as float32 [rays, 4]. Over DUMP_BUDGET_BYTES in all, every
    field keeps the same DUMP_SEED sample of its rays (sorted flat indices: sample_index.npy for
    `local`, image_sample_index.npy for `image`), the budget split by the two sets' sizes."""
    os.makedirs(directory, exist_ok=True)
    sets = [("", frame.local)] + ([("image_", frame.image)] if world > 1 else [])

    def ray_bytes(t):  # per ray, as written
        return 4 * t.shape[-1] if t.dtype == torch.uint8 else 8

    def rays_of(fields):
        t = next(iter(fields.values()))
        return t.shape[0] * t.shape[1]

    total = sum(rays_of(fs) * sum(ray_bytes(t) for t in fs.values()) for _, fs in sets)
    keep = min(1.0, DUMP_BUDGET_BYTES / max(total, 1))
    for prefix, fs in sets:
        n = rays_of(fs)
        idx = None
        if keep < 1.0:
            per_ray = sum(ray_bytes(t) for t in fs.values())
            count = int(n * keep * per_ray / (per_ray + 8))  # (+ 8: the index itself)
            pick = np.sort(np.random.default_rng(DUMP_SEED).choice(n, count, replace=False))
            np.save(os.path.join(directory, prefix + "sample_index.npy"),
                    pick.astype(np.float64))
            idx = torch.from_numpy(pick).to(next(iter(fs.values())).device)
        for f, t in fs.items():
            flat = t.reshape(n, -1) if t.dtype == torch.uint8 else t.reshape(n)
            if idx is not None:
                flat = flat.index_select(0, idx)
            a = flat.cpu().numpy()
            np.save(os.path.join(directory, prefix + f + ".npy"),
                    a.astype(np.float32 if a.dtype == np.uint8 else np.float64))


def render_stream(device):
    """One render stream. BHRT_BENCH_RENDER_STREAMS (A/B): torch (default: torch's stream pool),
    prio (torch's high-priority pool), cumask (a HIP stream with a full CU mask: a hardware queue
    of its own)."""
    mode = os.environ.get("BHRT_BENCH_RENDER_STREAMS", "torch")
    if mode == "prio":
        return torch.cuda.Stream(device, priority=-1)
    if mode == "cumask":
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        words = (cus + 31) // 32
        mask = (ctypes.c_uint32 * words)(*[0xFFFFFFFF] * words)
        if cus % 32:
            mask[words - 1] = (1 << (cus % 32)) - 1
        h = ctypes.c_void_p()
        if hip.hipExtStreamCreateWithCUMask(ctypes.byref(h), ctypes.c_uint32(words), mask) != 0:
            raise SystemExit("hipExtStreamCreateWithCUMask failed")
        return torch.cuda.ExternalStream(h.value, device=device)
    return torch.cuda.Stream(device)


def frame_latency(st, span_ms):
    """Completion latency of the timed frames. `mean` / `max`: each frame's
    execution window on the GPU's wall clock, stamped by the kernels themselves (bhrt_stats
    frame_ms: the first trace wave's start to the frame's last store -- the trace kernel's last
    wave, or a separate colour pass's last workgroup), against the busy span per frame (the GPU
    time a frame costs when frames overlap): ratio = mean / span. (From enqueue to done a frame
    also waits for the frames in flight ahead of it to free the CUs: two deep, ~2 spans.)"""
    if not st.get("frames_timed"):
        return None
    mean = st["frame_ms"] / st["frames_timed"]
    out = {"mean": round(mean, 4), "max": round(st["frame_ms_max"], 4),
           "ratio_to_busy_span": round(mean / span_ms, 3), "frames": st["frames_timed"],
           "note": "kernel-stamped execution window per frame: first trace wave start -> "
                   "last store (colour included)"}
    return out


def prev_tiles_order(pipe, last, H, W, B, S, shard):
    """The claim order (device int32 permutation of the shard's rays) that visits the 64-ray
    tiles of the kernel's own tiling (8x8, else 16x4, else 32x2: bhrt_api.c claim_tiles) in
    decreasing order of their longest ray's steps in frame `last`, each tile's rays in the
    kernel's in-tile order; installed with bhrt_set_claim_order. None if no tiling fits."""
    nrows = shard_row_count(H, B, shard, S)
    shape = next(((tw, th) for tw, th in ((8, 8), (16, 4), (32, 2))
                  if W % tw == 0 and nrows % th == 0), None)
    if shape is None:
        return None
    tw, th = shape
    fb = pipe.bufs[last % pipe.nslots]
    steps = fb.views["steps"].view(-1, W)[:nrows]
    cost = steps.view(nrows // th, th, W // tw, tw).amax(dim=(1, 3)).flatten()
    order = torch.argsort(-cost.to(torch.int64), stable=True)
    tc = W // tw
    base = (order // tc) * (th * W) + (order % tc) * tw
    w = torch.arange(64, device=steps.device)
    offs = (w // tw) * W + (w % tw)
    perm = (base[:, None] + offs[None, :]).flatten().to(torch.int32).contiguous()
    torch.cuda.synchronize()
    lib.set_claim_order(perm.data_ptr(), nrows * W)
    return perm


def display_resident_rate(c, bh, dk, cfg, cam, W, H, rows, n, rays, streams, device, frames,
                          frame_ms):
    """The same frames as the timed region, on the same streams, writing only the display
    call's device fields (Config.display_fields: 4 B/ray on C3/C4, 24 B/ray elsewhere)
    instead of every SoA field: the resident rate of a renderer that only shows the image.
    Reported beside `value`, never as it."""
    fields = c.display_fields()
    nb = max(2, len(streams))
    bufs = [{f: torch.empty((n, 4) if f == "rgba8" else (n,),
                            dtype={"rgba8": torch.uint8, "result": torch.int32}.get(
                                f, torch.float64), device=device) for f in fields}
            for _ in range(nb)]
    soas = [lib.soa_from_tensors(b) for b in bufs]
    torch.cuda.synchronize()

    def issue(k):  # buffer k % nb is only ever used on stream k % len(streams)
        s = streams[k % len(streams)]
        lib.render_frame_device(bh, dk, cfg, cam, W, H, rows, c.method, c.flags, soas[k % nb],
                                s.cuda_stream)

    for k in range(max(2 * nb, int(WARM_MS / max(frame_ms, 1e-3)) + 1)):  # (sustained: WARM_MS)
        issue(k)
    torch.cuda.synchronize()
    lib.stats_discard()
    t0 = time.perf_counter()
    for k in range(frames):
        issue(k)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / frames
    st = lib.stats(reset=True)
    return {"mrays_s": round(rays / dt / 1e6, 3), "ms_per_frame": round(dt * 1e3, 3),
            "fields": list(fields),
            "bytes_per_ray": sum(4 if f in ("rgba8", "result") else 8 for f in fields),
            "kernel_span_ms_per_frame": round(st["span_ms"] / max(st["launches"], 1), 4),
            "streams": len(streams),
            "note": "device-resident frames like the timed ones, writing only the display "
                    "call's fields (bench.py --fields display times them as the main line)"}


def host_path_rate(c, bh, dk, cfg, cam, W, H, frames=6):
    """bhrt_render_frame into host SoA arrays (allocated and touched once, reused every frame
    as a render loop does): the PCIe-inclusive rate a C caller of the host API sees, one
    synchronous call per frame, and with bhrt_render_frame_async three frames in flight (three
    sets of host arrays; frame i+1 traces while frame i is copied) -- for every SoA field (96
    B/ray) and for the visualizer's display call, the rgba8 buffer alone (4 B/px,
    INTEGRATION.md). Also the reference batch API and the latency of one drop-in trace_ray
    call. Reported beside `value`, never as it."""
    import ctypes as C
    L = lib.load()
    depth = 3  # frames in flight (bhrt_render_frame_async keeps up to 3 per thread)
    args = (C.byref(bh), C.byref(dk) if dk else None, C.byref(cfg), C.byref(cam), W, H,
            c.method, c.flags)

    def leg(fields):
        sets = [abi.alloc_soa(W * H, fields) for _ in range(depth)]
        for arrays, _ in sets:
            for a in arrays.values():
                a[...] = 0

        def sync_frame():
            if L.bhrt_render_frame(*args, C.byref(sets[0][1])) != 0:
                raise RuntimeError(lib.last_error())

        def issue(i):
            t = C.c_int(0)
            if L.bhrt_render_frame_async(*args, C.byref(sets[i % depth][1]), C.byref(t)) != 0:
                raise RuntimeError(lib.last_error())
            return t.value

        def wait(t):
            if L.bhrt_frame_wait(t) != 0:
                raise RuntimeError(lib.last_error())

        sync_frame()  # the slot's buffers and pinned staging allocated on first use
        t0 = time.perf_counter()
        for _ in range(frames):
            sync_frame()
        dt = (time.perf_counter() - t0) / frames
        for t in [issue(i) for i in range(depth)]:  # every slot warm
            wait(t)
        t0 = time.perf_counter()
        pending = [issue(i) for i in range(depth - 1)]
        for i in range(depth - 1, frames + depth - 1):
            if i < frames:
                pending.append(issue(i))
            wait(pending.pop(0))
        dta = (time.perf_counter() - t0) / frames
        return dt, dta, sum(a.nbytes for a in sets[0][0].values())

    # the reference's batch API (trace_rays_batch: Ray[] in, 160-byte RayTraceHit[] out, only
    # the fields trace_ray writes) on the frame's camera rays, arrays reused -- measured before
    # the host-frame legs and again after them. In this process both read ~30% below a fresh
    # process's calls (tools/batch_probe.py), GPU-side, for a reason not found (DESIGN.md
    # section 4, "Host-buffer ray batches")
    def batch_rate():
        if c.method != abi.INTEGRATOR_RK4:  # (trace_rays_batch is trace_ray, RK4)
            return None
        rays = configs.camera_rays(cam, W, H)
        hits = np.zeros(W * H, dtype=abi.HIT_DTYPE)
        bargs = (rays.ctypes.data, W * H, C.byref(bh), C.byref(dk) if dk else None, C.byref(cfg),
                 hits.ctypes.data, 0)
        if L.trace_rays_batch(*bargs) != 0:
            raise RuntimeError(lib.last_error())
        t0 = time.perf_counter()
        for _ in range(3):
            L.trace_rays_batch(*bargs)
        return round(W * H / ((time.perf_counter() - t0) / 3) / 1e6, 3)

    batch = batch_rate()
    dt, dta, nbytes = leg(FIELDS)
    dt8, dta8, nbytes8 = leg(("rgba8",))
    batch_after = batch_rate()
    # one drop-in trace_ray call (the camera's forward ray), host round trip included
    ray = abi.Ray(cam.position, cam.direction)
    hit = abi.RayTraceHit()
    lat = []
    for _ in range(12):
        t = time.perf_counter()
        L.trace_ray(C.byref(ray), C.byref(bh), C.byref(dk) if dk else None, C.byref(cfg),
                    C.byref(hit))
        lat.append(time.perf_counter() - t)
    lib.stats(reset=True)
    return {"mrays_s": round(W * H / dt / 1e6, 3), "ms_per_frame": round(dt * 1e3, 3),
            "async_mrays_s": round(W * H / dta / 1e6, 3),
            "async_ms_per_frame": round(dta * 1e3, 3),
            "bytes_to_host_per_frame": nbytes,
            "rgba8_mrays_s": round(W * H / dt8 / 1e6, 3),
            "rgba8_ms_per_frame": round(dt8 * 1e3, 3),
            "rgba8_async_mrays_s": round(W * H / dta8 / 1e6, 3),
            "rgba8_bytes_to_host_per_frame": nbytes8,
            "trace_rays_batch_mrays_s": batch,
            "trace_rays_batch_after_frames_mrays_s": batch_after,
            "trace_ray_latency_ms": round(sorted(lat[2:])[len(lat[2:]) // 2] * 1e3, 3),
            "note": "bhrt_render_frame into reused host arrays (every field; pinned staging, "
                    "host un-permute by up to 16 threads); async = bhrt_render_frame_async with "
                    "three frames in flight; rgba8 = the same calls with only the display buffer "
                    "(the visualizer's call, INTEGRATION.md); trace_rays_batch = the reference "
                    "batch API on the frame's camera rays (RayTraceHit[] out), measured before "
                    "the host-frame legs and again after them; trace_ray = median "
                    "of one drop-in call, PCIe round trip included"}


def batch_fresh_rate(args):
    """trace_rays_batch of the frame's camera rays in a fresh child process whose first GPU work
    it is (this process has not touched the GPU yet): the first call's wall time (code object
    load, pinned staging, first-touch) and the rate of the next calls, to compare with
    host_path.trace_rays_batch_after_frames_mrays_s of this process."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--batch-fresh-child", "--config",
           args.config, "--camera", args.camera]
    try:
        env = dict(os.environ)  # the runtime's own hardware-queue setting, as a C caller has
        if HWQ_ASKED is None:
            env.pop("GPU_MAX_HW_QUEUES", None)
        else:
            env["GPU_MAX_HW_QUEUES"] = HWQ_ASKED
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
        return json.loads(r.stdout.strip().splitlines()[-1])
    except Exception as e:  # (reported, never fatal: a side leg)
        return {"error": repr(e)[:300]}


def batch_fresh_child(args):
    import ctypes as C
    c = configs.CONFIGS[args.config]
    bh, dk, cfg = c.scene()
    cam = configs.camera(args.camera)
    W, H = c.frame(1).width, c.frame(1).height
    rays = configs.camera_rays(cam, W, H)
    hits = np.zeros(W * H, dtype=abi.HIT_DTYPE)
    L = lib.load()
    bargs = (rays.ctypes.data, W * H, C.byref(bh), C.byref(dk) if dk else None, C.byref(cfg),
             hits.ctypes.data, 0)
    ms = []
    for _ in range(5):
        t = time.perf_counter()
        if L.trace_rays_batch(*bargs) != 0:
            raise RuntimeError(lib.last_error())
        ms.append((time.perf_counter() - t) * 1e3)
    later = sorted(ms[1:])
    med = (later[1] + later[2]) / 2
    print(json.dumps({"first_call_ms": round(ms[0], 2), "calls_ms": [round(v, 3) for v in ms],
                      "mrays_s": round(W * H / med / 1e3, 3),
                      "note": "fresh child process, trace_rays_batch is its first GPU work; "
                              "mrays_s from the median of calls 2-5"}), flush=True)


def pmc_profile(config):
    """The committed rocprofv3 PMC summary of the config's trace kernel (tools/pmc_summary.py):
    HBM bytes per launch (FETCH_SIZE x2 per the gfx950 correction + WRITE_SIZE,
    MI355X_MICROARCH.md 'HBM') and issued FP64 work per launch, or None."""
    p = os.path.join(ROOT, "profiles", f"pmc_{config}.json")
    if not os.path.exists(p):
        return None
    with open(p) as f:
        return json.load(f)


def cpu_baseline(args, c, bh, dk, cfg, cam, frame, H):
    """The compiled reference (or, if it was not built, the oracle restatement) on every k-th
    row of rank 0's shard of the same frame; also the parity of those rows against the GPU's."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as orc
    try:
        checker, kind = orc.reference(), "reference"
    except (FileNotFoundError, OSError):
        checker, kind = orc.oracle(), "port"
    threads = int(os.environ.get("OMP_NUM_THREADS", "0")) or min(16, os.cpu_count() or 1)
    W = frame.local["result"].shape[1]
    stride = args.cpu_rows_stride or CPU_ROWS_STRIDE.get(c.name, 27)
    local = list(range(0, len(frame.local_rows), stride))
    rows = [int(frame.local_rows[j]) for j in local]
    got = {f: frame.local[f].cpu().numpy()[local] for f in FIELDS}
    t0 = time.perf_counter()
    want = []
    for r in rows:
        want.append(checker.render_frame(bh, dk, cfg, cam, W, H, c.method, c.flags,
                                         rows=abi.Rows(1, r, H), threads=threads))
    dt = time.perf_counter() - t0
    nrays = len(rows) * W
    want = {f: np.stack([w[f] for w in want]) for f in FIELDS}
    mism = int((got["result"] != want["result"]).sum() + (got["steps"] != want["steps"]).sum())
    worst = 0.0
    for f in ("hit_x", "hit_y", "hit_z", "distance", "time_dilation", "rgb_r", "rgb_g", "rgb_b"):
        a, b = got[f], want[f]
        ok = ~(np.isnan(a) | np.isnan(b))
        if ok.any():
            worst = max(worst, float(np.max(np.abs(a[ok] - b[ok]) /
                                            np.maximum(np.abs(b[ok]), 1e-9))))
    base = {"value": round(nrays / dt / 1e6, 5), "unit": "Mrays/s", "cores": threads,
            "kind": kind,
            "sample": f"every {stride}th row of the {W}x{H} frame's rendered "
                      f"shard ({nrays} rays, "
                      f"{dt:.1f} s wall, OpenMP over rays; the reference integrates every ray "
                      f"to its full step budget before the disk scan)"}
    return base, worst, mism


if __name__ == "__main__":
    main()
