"""Batched photon paths (bhrt_trace_paths_device) against the ways the same rays could be had
before: one JSON line per batch.

A batch is --rays camera-B rays of a BASELINE scene, taken at a fixed stride over the scene's
whole frame (so it holds the frame's mix of short and budget-long rays), with P = max_steps + 1
positions per ray. Timed in one process on one stream, in alternating windows after a warm-up:
  paths    bhrt_trace_paths_device, for both store forms (BHRT_PATHS_STORE=direct|staged),
           every in {1, 8}, into xyz + count and into xyz32 + count, without hit records;
           `+hits` adds them (the trace launch behind the path launch);
  trace    bhrt_trace_rays_device on the same rays, recording nothing: the price of recording
           is paths / trace;
  loop     the same rays one by one through integrate_photon_path with a path array: the only
           way to record them before (it has no disk, so its rays run on where trace_ray's
           view ends at the disk: its stored points are counted as it stores them).
A window is a host clock around calls issued back to back and one device synchronise, at least
--window seconds long; the figure of a way is the median over --reps windows with the smallest
and largest beside it. The loop is timed over --loop-rays rays per repetition.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing-engine-in-c_amd"))
from bhrt import abi, configs, lib  # noqa: E402


def batch_rays(c, n):
    rays = configs.camera_rays(configs.camera("B"), c.width, c.height)
    stride = len(rays) // n
    return np.ascontiguousarray(rays[stride // 2::stride][:n])


def bench_batch(torch, name, n, window, reps, warmup, loop_rays):
    c = configs.CONFIGS[name]
    bh, dk, cfg = c.scene()
    rays = batch_rays(c, n)
    P = cfg.max_integration_steps + 1
    d_rays = torch.from_numpy(rays.view(np.uint8)).cuda()
    xyz = torch.zeros((n, P, 3), dtype=torch.float64, device="cuda")
    xyz32 = torch.zeros((n, P, 3), dtype=torch.float32, device="cuda")
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    hits = {f: torch.zeros(n, dtype=torch.int32 if f in ("result", "steps") else torch.float64,
                           device="cuda") for f in abi.PATH_HIT_FIELDS}
    soa = lib.soa_from_tensors(hits)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()

    def paths_call(form, every, f32, with_hits):
        p = abi.Paths(xyz=None if f32 else xyz.data_ptr(), xyz32=xyz32.data_ptr() if f32 else None,
                      count=count.data_ptr())

        def call():
            os.environ["BHRT_PATHS_STORE"] = form
            lib.trace_paths_device(d_rays.data_ptr(), n, bh, dk, cfg, c.method, P, every, p,
                                   soa if with_hits else None, st.cuda_stream)
        return call

    def trace_call():
        L = lib.load()
        rc = L.bhrt_trace_rays_device(d_rays.data_ptr(), n, C.byref(bh), C.byref(dk) if dk else None,
                                      C.byref(cfg), c.method, 0, C.byref(soa),
                                      C.c_void_p(st.cuda_stream))
        assert rc == 0, lib.last_error()

    ways = {}
    for form in ("direct", "staged"):
        for every in (1, 8):
            ways[f"paths_{form}_every{every}_xyz"] = paths_call(form, every, False, False)
            ways[f"paths_{form}_every{every}_xyz32"] = paths_call(form, every, True, False)
        ways[f"paths_{form}_every1_xyz+hits"] = paths_call(form, 1, False, True)
    ways["trace"] = trace_call

    def run_window(call, seconds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = 0
        while True:
            for _ in range(4):
                call()
            k += 4
            st.synchronize()
            if time.perf_counter() - t0 >= seconds:
                break
        return (time.perf_counter() - t0) / k, k

    stored = {}
    for w, call in ways.items():
        for _ in range(warmup):
            call()
        torch.cuda.synchronize()
        if w != "trace":
            stored[w] = int(count.sum().item())
    lib.stats_discard()
    times = {w: [] for w in ways}
    calls = {w: 0 for w in ways}
    for _ in range(reps):
        for w, call in ways.items():
            t, k = run_window(call, window)
            times[w].append(t)
            calls[w] += k
        lib.stats_discard()
    os.environ.pop("BHRT_PATHS_STORE", None)

    # the loop of single-ray calls, as a caller had to write it before
    L = lib.load()
    m = min(loop_rays, n)
    path = np.zeros((P, 3))
    loop_t, loop_pts = [], 0
    for _ in range(max(2, reps // 2 + 1)):
        pts = 0
        t0 = time.perf_counter()
        for ray in rays[:: n // m][:m]:
            num = C.c_int(0)
            o, d = ray["origin"], ray["direction"]
            L.integrate_photon_path(C.byref(abi.Vector4D(0.0, o[0], o[1], o[2])),
                                    C.byref(abi.Vector3D(d[0], d[1], d[2])), C.byref(bh),
                                    C.byref(cfg), c.method, path.ctypes.data, P, C.byref(num), None)
            pts += num.value
        loop_t.append((time.perf_counter() - t0) / m)
        loop_pts = pts
    out = {"scene": name, "rays": n, "camera": "B", "max_positions": P, "window_s": window,
           "reps": reps, "lib": os.path.basename(lib.LIB_PATH)}
    for w in ways:
        med = statistics.median(times[w])
        r = {"call_ms": round(med * 1e3, 4),
             "call_ms_min_max": [round(min(times[w]) * 1e3, 4), round(max(times[w]) * 1e3, 4)],
             "Mpaths_per_s": round(n / med / 1e6, 4), "calls_timed": calls[w]}
        if w in stored:
            r["points_stored"] = stored[w]
            r["Mpoints_per_s"] = round(stored[w] / med / 1e6, 2)
        out[w] = r
    med = statistics.median(loop_t)
    out["loop"] = {"ray_ms": round(med * 1e3, 4),
                   "ray_ms_min_max": [round(min(loop_t) * 1e3, 4), round(max(loop_t) * 1e3, 4)],
                   "Mpaths_per_s": round(1.0 / med / 1e6, 6), "rays_timed": m,
                   "points_stored": loop_pts, "Mpoints_per_s": round(loop_pts / m / med / 1e6, 3)}
    for form in ("direct", "staged"):
        k = f"paths_{form}_every1_xyz"
        out[f"{form}_over_loop"] = round(out[k]["Mpaths_per_s"] / out["loop"]["Mpaths_per_s"], 1)
        out[f"{form}_over_trace_time"] = round(out[k]["call_ms"] / out["trace"]["call_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="C2,C4")
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (>= 0.5)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of every way")
    ap.add_argument("--loop-rays", type=int, default=512)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_paths.py needs a HIP device (no CPU path)")
    lib.load()
    for name in args.scenes.split(","):
        print(json.dumps(bench_batch(torch, name, args.rays, args.window, args.reps, args.warmup,
                                     args.loop_rays)), flush=True)


if __name__ == "__main__":
    main()
