"""Kerr disk-emission frames (bhrt_kerr_emit_frame_device) timed beside the adaptive frame they are
built on (bhrt_kerr_rk45_frame_device) in the same process: one JSON line per leg, printed and
written to profiles/kerr_emit/bench_kerr_emit.jsonl.

tools/bench_kerr_rk45.py's 1920x1080 scene at tolerance 1e-8: spin 0.9 with its disk, camera at
(0, -18, 4), fov 40 degrees, max distance 60, 2000 attempts, rgba8 out. The legs:
  rk45          the adaptive frame as that tool times it (BHRT_FLAG_DOPPLER): the yardstick;
  emit K=1      the emission frame with one crossing per ray, rgba8 and intensity;
  emit K=4      the emission frame with four crossings, rgba8 and every emission output.
The legs are timed in alternating windows after a warm-up, frames issued back to back on one stream
with one frame in flight; a window is a host clock around frames, at least --window seconds long,
and a leg's figure is the median over --reps windows with the smallest and largest beside it.
attempts is bhrt_stats.iterations of one frame. Ratios are of frame times of the same run: K=1
over rk45 (what recording costs a ray that ends where it did before), and K=4 over K=1 beside the
ratio of their attempts (the count-based bound: a ray that goes on costs its further attempts).
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

SPIN, DISK, TOL = 0.9, (2.4, 12.0), 1e-8
Q, GAIN = 3.0, 0.25
OUT = os.path.join(ROOT, "profiles", "kerr_emit", "bench_kerr_emit.jsonl")


def bench_size(torch, W, H, window, reps, warmup):
    n = W * H
    K = abi.EMIT_MAX_CROSSINGS
    stream = torch.cuda.Stream()
    out8 = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    planes = torch.zeros((2, K, n), dtype=torch.float64, device="cuda")
    inten = torch.zeros(n, dtype=torch.float64, device="cuda")
    soa8 = abi.FrameSoA(rgba8=out8.data_ptr())
    bh, dk = abi.black_hole(1.0, SPIN), abi.disk(*DISK)
    cfg = abi.sim_config(0.25, 60.0, 2000, TOL)
    cam = abi.Camera(abi.v3(0.0, -18.0, 4.0), abi.v3(0.0, 18.0, -4.0), abi.v3(0.0, 0.0, 1.0), 40.0)
    torch.cuda.synchronize()

    def rk45():
        lib.kerr_rk45_frame_device(bh, dk, cfg, cam, W, H, None, abi.BHRT_FLAG_DOPPLER, soa8, None,
                                   stream.cuda_stream)

    def emit(k, eo):
        ep = abi.KerrEmitParams(k, Q, GAIN)
        return lambda: lib.kerr_emit_frame_device(bh, dk, cfg, cam, W, H, None, 0, soa8, ep, eo,
                                                  None, stream.cuda_stream)

    legs = {"rk45": rk45,
            "emit K=1": emit(1, abi.KerrEmitOut(intensity=inten.data_ptr())),
            "emit K=4": emit(K, abi.KerrEmitOut(count.data_ptr(), planes[0].data_ptr(),
                                                planes[1].data_ptr(), inten.data_ptr()))}

    def run_window(frame, seconds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = 0
        while k == 0 or time.perf_counter() - t0 < seconds:
            frame()
            stream.synchronize()
            k += 1
        return (time.perf_counter() - t0) / k

    attempts = {}
    for name, frame in legs.items():
        stream.synchronize()
        lib.stats(reset=True)
        frame()
        stream.synchronize()
        attempts[name] = int(lib.stats(reset=True)["iterations"])
    crossings = torch.bincount(count, minlength=K + 1).tolist()
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
    med = {name: statistics.median(times[name]) for name in legs}
    lines = []
    for name in legs:
        line = {"leg": name, "width": W, "height": H,
                "scene": f"kerr spin {SPIN} disk {list(DISK)} tol {TOL:g} rgba8",
                "window_s": window, "reps": reps,
                "frame_ms": round(med[name] * 1e3, 4),
                "frame_ms_min_max": [round(min(times[name]) * 1e3, 4),
                                     round(max(times[name]) * 1e3, 4)],
                "attempts_per_frame": attempts[name],
                "gattempts_per_s": round(attempts[name] / med[name] / 1e9, 3)}
        if name == "emit K=1":
            line["time_over_rk45"] = round(med[name] / med["rk45"], 3)
            line["attempts_over_rk45"] = round(attempts[name] / attempts["rk45"], 4)
        if name == "emit K=4":
            line["time_over_k1"] = round(med[name] / med["emit K=1"], 3)
            line["attempts_over_k1"] = round(attempts[name] / attempts["emit K=1"], 4)
            line["rays_by_crossings"] = crossings
        lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080")
    ap.add_argument("--window", type=float, default=0.6, help="seconds per timed window")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3, help="untimed frames of every leg")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_kerr_emit.py needs a HIP device (no CPU path)")
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
