"""Adaptive physical-geodesic frames (bhrt_kerr_rk45_frame_device) timed beside the fixed-step
frames (bhrt_kerr_frame_device) in the same process: one JSON line per leg, printed and written
to profiles/kerr_rk45/bench_kerr_rk45.jsonl.

tools/bench_kerr.py's scene and windows: spin 0.9 with its disk and Doppler colours, camera at
(0, -18, 4), fov 40 degrees, max distance 60, 2000 steps, rgba8 out, at 1920x1080 and 3840x2160.
The legs per size are RK4 at time_step 0.25 and Dormand-Prince 5(4) at tolerance 1e-6 and 1e-8
(first trial step 0.25). The legs are timed in alternating windows after a warm-up, frames issued
back to back on one stream with one frame in flight; a window is a host clock around frames, at
least --window seconds long, and a leg's figure is the median over --reps windows with the
smallest and largest beside it. attempts is bhrt_stats.iterations of one frame (RK4: its steps);
an adaptive leg's speedup is the RK4 leg's frame time of the same run over its own -- never a
figure of another run.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing-engine-in-c_amd"))
from bhrt import abi, lib  # noqa: E402

SPIN, DISK = 0.9, (2.4, 12.0)
OUT = os.path.join(ROOT, "profiles", "kerr_rk45", "bench_kerr_rk45.jsonl")


def bench_size(torch, W, H, window, reps, warmup):
    n = W * H
    stream = torch.cuda.Stream()
    out8 = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    rej = torch.zeros(n, dtype=torch.int32, device="cuda")
    soa8 = abi.FrameSoA(rgba8=out8.data_ptr())
    bh, dk = abi.black_hole(1.0, SPIN), abi.disk(*DISK)
    cam = abi.Camera(abi.v3(0.0, -18.0, 4.0), abi.v3(0.0, 18.0, -4.0), abi.v3(0.0, 0.0, 1.0), 40.0)
    torch.cuda.synchronize()

    def rk4():
        cfg = abi.sim_config(0.25, 60.0, 2000)
        return lambda diag=None: lib.kerr_frame_device(bh, dk, cfg, cam, W, H, None,
                                                       abi.BHRT_FLAG_DOPPLER, soa8, None,
                                                       stream.cuda_stream)

    def rk45(tol):
        cfg = abi.sim_config(0.25, 60.0, 2000, tol)
        return lambda diag=None: lib.kerr_rk45_frame_device(bh, dk, cfg, cam, W, H, None,
                                                            abi.BHRT_FLAG_DOPPLER, soa8, diag,
                                                            stream.cuda_stream)

    legs = {"rk4 time_step 0.25": rk4(), "rk45 tol 1e-6": rk45(1e-6), "rk45 tol 1e-8": rk45(1e-8)}

    def run_window(frame, seconds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = 0
        while k == 0 or time.perf_counter() - t0 < seconds:
            frame()
            stream.synchronize()
            k += 1
        return (time.perf_counter() - t0) / k

    # one frame of each leg for its attempts and rejected attempts
    attempts, rejected = {}, {}
    for name, frame in legs.items():
        stream.synchronize()
        lib.stats(reset=True)
        rej.zero_()
        torch.cuda.synchronize()
        frame(abi.KerrRk45Diag(None, None, rej.data_ptr()))
        stream.synchronize()
        attempts[name] = int(lib.stats(reset=True)["iterations"])
        rejected[name] = int(rej.sum().item())
    for frame in legs.values():
        for _ in range(warmup):
            frame()
        stream.synchronize()
    lib.stats_discard()
    times = {name: [] for name in legs}
    for _ in range(reps):
        for name, frame in legs.items():
            times[name].append(run_window(frame, window))
        lib.stats_discard()
    base = statistics.median(times["rk4 time_step 0.25"])
    lines = []
    for name in legs:
        med = statistics.median(times[name])
        lines.append({"leg": name, "width": W, "height": H,
                      "scene": f"kerr spin {SPIN} disk {list(DISK)} doppler rgba8",
                      "window_s": window, "reps": reps,
                      "frame_ms": round(med * 1e3, 4),
                      "frame_ms_min_max": [round(min(times[name]) * 1e3, 4),
                                           round(max(times[name]) * 1e3, 4)],
                      "attempts_per_frame": attempts[name],
                      "gattempts_per_s": round(attempts[name] / med / 1e9, 3),
                      "rejected_share": round(rejected[name] / attempts[name], 4),
                      "speedup_vs_rk4": round(base / med, 3)})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--window", type=float, default=0.6, help="seconds per timed window")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3, help="untimed frames of every leg")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_kerr_rk45.py needs a HIP device (no CPU path)")
    lib.load()
    lines = []
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for line in bench_size(torch, W, H, args.window, args.reps, args.warmup):
            print(json.dumps(line), flush=True)
            lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
