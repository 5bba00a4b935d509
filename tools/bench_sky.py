"""Sky-map frames (BHRT_FLAG_SKY) against the same frames without the flag: one JSON line per
scene.

Per scene (camera B, rgba8 out, one device), the plain frame and the frame that looks a
--sky WxH RGB32F map up where rays leave the scene, timed in ONE process in alternating windows
after a warm-up, frames issued back to back on one stream with --depth in flight (the host waits
only for the frame --depth frames back). A window is a host clock around frames, at least
--window seconds long; a way's figure is the median over --reps windows with the smallest and
largest beside it (the spread). The cost of the map is the ratio sky / plain of the same run.

The map is random noise (every tap a different value: nothing for a cache to dedupe); its
footprint -- 16 bytes per texel on the device -- is printed against the L2 of one XCD (4 MiB)
and the MALL (256 MiB) of an MI355X, with the share of the frame's rays that look it up.
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

L2_XCD_MIB, MALL_MIB = 4, 256


def bench_scene(torch, np, name, W, H, window, reps, warmup, depth):
    c = configs.CONFIGS[name]
    bh, dk, cfg = c.scene()
    n = W * H
    cam = configs.camera("B")
    stream = torch.cuda.Stream()
    out8 = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    res = torch.zeros(n, dtype=torch.int32, device="cuda")
    soa8 = abi.FrameSoA(rgba8=out8.data_ptr())
    torch.cuda.synchronize()

    def frame_plain():
        lib.render_frame_device(bh, dk, cfg, cam, W, H, None, c.method, c.flags, soa8,
                                stream.cuda_stream)

    def frame_sky():
        lib.render_frame_device(bh, dk, cfg, cam, W, H, None, c.method,
                                c.flags | abi.BHRT_FLAG_SKY, soa8, stream.cuda_stream)

    def run_window(frame, seconds):
        torch.cuda.synchronize()
        pending = collections.deque()
        t0 = time.perf_counter()
        k = 0
        while k == 0 or time.perf_counter() - t0 < seconds:
            frame()
            ev = torch.cuda.Event()
            ev.record(stream)
            pending.append(ev)
            if len(pending) > depth:
                pending.popleft().synchronize()
            k += 1
        stream.synchronize()
        return (time.perf_counter() - t0) / k, k

    # the share of rays that look the map up, from one frame's classes
    lib.render_frame_device(bh, dk, cfg, cam, W, H, None, c.method, c.flags | abi.BHRT_FLAG_SKY,
                            abi.FrameSoA(result=res.data_ptr(), rgba8=out8.data_ptr()),
                            stream.cuda_stream)
    stream.synchronize()
    classes = np.bincount(res.cpu().numpy(), minlength=6)
    ways = {"plain": frame_plain, "sky": frame_sky}
    for frame in ways.values():
        for _ in range(warmup):
            frame()
        stream.synchronize()
    lib.stats_discard()
    times = {w: [] for w in ways}
    frames = {w: 0 for w in ways}
    for _ in range(reps):
        for w, frame in ways.items():
            t, k = run_window(frame, window)
            times[w].append(t)
            frames[w] += k
        lib.stats_discard()
    out = {"scene": name, "width": W, "height": H, "camera": "B", "window_s": window, "reps": reps,
           "depth": depth, "classes": classes.tolist(),
           "lookup_share": round(float(classes[abi.RAY_MAX_DISTANCE] + classes[abi.RAY_MAX_STEPS]) / n, 4),
           "chord_share": round(float(classes[abi.RAY_MAX_DISTANCE]) / n, 4)}
    for w in ways:
        med = statistics.median(times[w])
        out[w] = {"frame_ms": round(med * 1e3, 4),
                  "frame_ms_min_max": [round(min(times[w]) * 1e3, 4), round(max(times[w]) * 1e3, 4)],
                  "mrays_per_s": round(n / med / 1e6, 2), "frames_timed": frames[w]}
    out["sky_over_plain"] = round(out["sky"]["frame_ms"] / out["plain"]["frame_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="C4:3840x2160,C5:3840x2160,C2:1920x1080")
    ap.add_argument("--sky", default="4096x2048", help="the map's size")
    ap.add_argument("--window", type=float, default=0.6, help="seconds per timed window (>= 0.6)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=4, help="untimed frames of either way")
    ap.add_argument("--depth", type=int, default=3, help="frames in flight")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sky.py needs a HIP device (no CPU path)")
    lib.load()
    sw, sh = (int(v) for v in args.sky.split("x"))
    sky = lib.sky_create(np.random.default_rng(1).random((sh, sw, 3), dtype=np.float32))
    lib.set_sky(sky)
    mib = sw * sh * 16 / 2 ** 20
    print(json.dumps({"sky": args.sky, "format": "rgb32f", "device_mib": round(mib, 1),
                      "times_l2_of_one_xcd": round(mib / L2_XCD_MIB, 2),
                      "share_of_mall": round(mib / MALL_MIB, 3)}), flush=True)
    try:
        for spec in args.scenes.split(","):
            name, size = spec.split(":")
            W, H = (int(v) for v in size.split("x"))
            print(json.dumps(bench_scene(torch, np, name, W, H, args.window, args.reps, args.warmup,
                                         args.depth)), flush=True)
    finally:
        torch.cuda.synchronize()
        lib.sky_destroy(sky)


if __name__ == "__main__":
    main()
