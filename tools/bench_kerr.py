"""Physical-geodesic frames (bhrt_kerr_frame_device) timed beside the parity path's plain frames:
one JSON line per frame size.

Per size, a Kerr spin-0.9 frame with its disk and Doppler colours (the tests' scene: camera at
(0, -18, 4), fov 40 degrees, time_step 0.25, max distance 60, 2000 steps, disk [2.4, 12]) into an
rgba8 array, and the parity path's C2 and C4 frames (camera B, rgba8 out) for scale -- the trace
kernel is the parent revision's, instruction for instruction, so these are its figures on the
same box in the same process. Each way is timed in alternating windows after a warm-up, frames
issued back to back on one stream with one frame and with --depth frames in flight (the host
waits only for the frame that many back). A window is a host clock around frames, at least
--window seconds long; a way's figure is the median over --reps windows with the smallest and
largest beside it. steps/s counts RK4 steps (bhrt_stats.iterations of one frame).
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing-engine-in-c_amd"))
from bhrt import abi, configs, lib  # noqa: E402

SPIN, DISK = 0.9, (2.4, 12.0)


def bench_size(torch, np, W, H, window, reps, warmup, depth):
    n = W * H
    stream = torch.cuda.Stream()
    out8 = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    res = torch.zeros(n, dtype=torch.int32, device="cuda")
    soa8 = abi.FrameSoA(rgba8=out8.data_ptr())
    bh, dk = abi.black_hole(1.0, SPIN), abi.disk(*DISK)
    cfg = abi.sim_config(0.25, 60.0, 2000)
    cam = abi.Camera(abi.v3(0.0, -18.0, 4.0), abi.v3(0.0, 18.0, -4.0), abi.v3(0.0, 0.0, 1.0), 40.0)
    camB = configs.camera("B")
    torch.cuda.synchronize()

    def kerr():
        lib.kerr_frame_device(bh, dk, cfg, cam, W, H, None, abi.BHRT_FLAG_DOPPLER, soa8, None,
                              stream.cuda_stream)

    def parity(name):
        c = configs.CONFIGS[name]
        sbh, sdk, scfg = c.scene()
        return lambda: lib.render_frame_device(sbh, sdk, scfg, camB, W, H, None, c.method, c.flags,
                                               soa8, stream.cuda_stream)

    ways = {"kerr": kerr, "C2": parity("C2"), "C4": parity("C4")}

    def run_window(frame, seconds, in_flight):
        torch.cuda.synchronize()
        pending = collections.deque()
        t0 = time.perf_counter()
        k = 0
        while k == 0 or time.perf_counter() - t0 < seconds:
            frame()
            ev = torch.cuda.Event()
            ev.record(stream)
            pending.append(ev)
            if len(pending) >= in_flight:
                pending.popleft().synchronize()
            k += 1
        stream.synchronize()
        return (time.perf_counter() - t0) / k, k

    # one frame of each way for its step count (and the Kerr frame's classes)
    steps = {}
    for w, frame in ways.items():
        stream.synchronize()
        lib.stats(reset=True)
        frame()
        stream.synchronize()
        steps[w] = int(lib.stats(reset=True)["iterations"])
    lib.kerr_frame_device(bh, dk, cfg, cam, W, H, None, abi.BHRT_FLAG_DOPPLER,
                          abi.FrameSoA(result=res.data_ptr()), None, stream.cuda_stream)
    stream.synchronize()
    classes = np.bincount(res.cpu().numpy(), minlength=6).tolist()
    for frame in ways.values():
        for _ in range(warmup):
            frame()
        stream.synchronize()
    lib.stats_discard()
    out = {"width": W, "height": H, "scene": f"kerr spin {SPIN} disk {list(DISK)} doppler",
           "window_s": window, "reps": reps, "classes": classes}
    for in_flight in (1, depth):
        times = {w: [] for w in ways}
        for _ in range(reps):
            for w, frame in ways.items():
                t, _k = run_window(frame, window, in_flight)
                times[w].append(t)
            lib.stats_discard()
        for w in ways:
            med = statistics.median(times[w])
            out.setdefault(w, {"steps_per_frame": steps[w]})[f"in_flight_{in_flight}"] = {
                "frame_ms": round(med * 1e3, 4),
                "frame_ms_min_max": [round(min(times[w]) * 1e3, 4), round(max(times[w]) * 1e3, 4)],
                "mrays_per_s": round(n / med / 1e6, 2),
                "gsteps_per_s": round(steps[w] / med / 1e9, 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--window", type=float, default=0.6, help="seconds per timed window")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3, help="untimed frames of every way")
    ap.add_argument("--depth", type=int, default=3, help="frames in flight of the second figure")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_kerr.py needs a HIP device (no CPU path)")
    lib.load()
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        print(json.dumps(bench_size(torch, np, W, H, args.window, args.reps, args.warmup,
                                    args.depth)), flush=True)


if __name__ == "__main__":
    main()
