"""Physical photon paths (bhrt_kerr_paths_device) timed: one JSON line.

Input: 4096 rays at a fixed pixel stride over the 1920x1080 frame of bench_kerr.py's scene (Kerr
spin 0.9, disk [2.4, 12], camera at (0, -18, 4), fov 40 degrees, time_step 0.25, max distance 60,
2000 steps), 512 positions per ray. The tool first checks, on its own rays, that 512 positions
hold every path (the longest count of the every-1 call is reported, and a truncated ray is an
error).

Ways, all on one stream, device arrays only:
  xyz_every1    xyz and count, every point
  xyz_every8    xyz and count, every 8th point and the last
  xyz32_every1  xyz32 and count
  xyz_hits      xyz, count and the hit records (result, steps, hit_x/y/z, distance): two launches
  rays_result   bhrt_kerr_rays_device of the same rays writing `result` only: nothing recorded
  single_ray    the path call with n = 1 in a loop over 64 of the rays (xyz and count): the
                single-ray alternative; its figures are per 64 rays
Protocol: each way is timed in alternating windows after a warm-up, calls issued back to back with
one call in flight (the host waits for each call's end). A window is a host clock around calls, at
least --window seconds long; a way's figure is the median over --reps windows with the smallest
and largest beside it. Per way: ms per call, paths/s, stored points/s, steps/s (RK4 steps:
bhrt_stats.iterations of one call). There is no CPU path: without a HIP device the tool fails.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing-engine-in-c_amd"))
from bhrt import abi, lib  # noqa: E402

SPIN, DISK = 0.9, (2.4, 12.0)
W, H, N, P = 1920, 1080, 4096, 512
SINGLE = 64


def frame_rays(np):
    """N rays of the W x H frame at a fixed pixel stride (calculate_ray_direction's mapping)."""
    pos, look, up0 = np.array([0.0, -18.0, 4.0]), np.array([0.0, 18.0, -4.0]), np.array([0.0, 0.0, 1.0])
    fwd = look / np.linalg.norm(look)
    right = np.cross(fwd, up0)
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    plane_h = 2.0 * math.tan(math.radians(40.0) / 2.0)
    plane_w = plane_h * W / H
    pix = np.arange(N) * ((W * H) // N)
    px, py = pix % W, pix // W
    ndcx = (2.0 * ((px + 0.5) / W) - 1.0) * plane_w
    ndcy = (1.0 - 2.0 * ((py + 0.5) / H)) * plane_h
    d = fwd[None, :] + right[None, :] * ndcx[:, None] + up[None, :] * ndcy[:, None]
    rays = np.zeros(N, dtype=abi.RAY_DTYPE)
    rays["origin"] = pos
    rays["direction"] = d / np.linalg.norm(d, axis=1)[:, None]
    return rays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window (>= 0.5)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3, help="untimed calls of every way")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_kerr_paths.py needs a HIP device (no CPU path)")
    lib.load()
    window = max(args.window, 0.5)
    stream = torch.cuda.Stream()
    st = stream.cuda_stream
    bh, dk, cfg = abi.black_hole(1.0, SPIN), abi.disk(*DISK), abi.sim_config(0.25, 60.0, 2000)
    rays = frame_rays(np)
    d_rays = torch.from_numpy(rays.view(np.float64).reshape(-1, 6)).cuda()
    xyz = torch.zeros((N, P, 3), dtype=torch.float64, device="cuda")
    xyz32 = torch.zeros((N, P, 3), dtype=torch.float32, device="cuda")
    count = torch.zeros(N, dtype=torch.int32, device="cuda")
    i32 = {f: torch.zeros(N, dtype=torch.int32, device="cuda") for f in ("result", "steps")}
    f64 = {f: torch.zeros(N, dtype=torch.float64, device="cuda")
           for f in ("hit_x", "hit_y", "hit_z", "distance")}
    hits = abi.FrameSoA(**{f: v.data_ptr() for f, v in {**i32, **f64}.items()})
    only_result = abi.FrameSoA(result=i32["result"].data_ptr())
    p_xyz = abi.Paths(xyz.data_ptr(), None, count.data_ptr())
    p_x32 = abi.Paths(None, xyz32.data_ptr(), count.data_ptr())
    ray_bytes = rays.dtype.itemsize
    torch.cuda.synchronize()

    def paths(p, every, h=None):
        return lambda: lib.kerr_paths_device(d_rays.data_ptr(), N, bh, dk, cfg, P, every, 0, p, h,
                                             None, st)

    def single():
        for i in range(SINGLE):
            k = i * (N // SINGLE)
            lib.kerr_paths_device(d_rays.data_ptr() + k * ray_bytes, 1, bh, dk, cfg, P, 1, 0,
                                  abi.Paths(xyz.data_ptr() + k * P * 24, None,
                                            count.data_ptr() + k * 4), None, None, st)

    ways = {"xyz_every1": paths(p_xyz, 1), "xyz_every8": paths(p_xyz, 8),
            "xyz32_every1": paths(p_x32, 1), "xyz_hits": paths(p_xyz, 1, hits),
            "rays_result": lambda: lib.kerr_rays_device(d_rays.data_ptr(), N, bh, dk, cfg, 0,
                                                        only_result, None, st),
            "single_ray": single}
    n_paths = {w: N for w in ways}
    n_paths["single_ray"] = SINGLE

    # one call of each way: its steps and its stored points; the every-1 call's longest path
    steps, points = {}, {}
    for w, call in ways.items():
        count.zero_()
        torch.cuda.synchronize()
        lib.stats(reset=True)
        call()
        stream.synchronize()
        s = lib.stats(reset=True)
        steps[w] = int(s["iterations"]) // (2 if w == "xyz_hits" else 1)
        c = count.cpu().numpy()
        points[w] = 0 if w == "rays_result" else int(c.sum())
        if w == "xyz_every1":
            longest = int(c.max())
            lib.kerr_rays_device(d_rays.data_ptr(), N, bh, dk, cfg, 0,
                                 abi.FrameSoA(result=i32["result"].data_ptr(),
                                              steps=i32["steps"].data_ptr()), None, st)
            stream.synchronize()
            ray_steps = i32["steps"].cpu().numpy()
            classes = np.bincount(i32["result"].cpu().numpy(), minlength=6).tolist()
            if longest >= P or not np.array_equal(c, ray_steps + 1):
                raise SystemExit(f"bench_kerr_paths.py: {P} positions do not hold every path "
                                 f"(longest count {longest}, longest ray {int(ray_steps.max())} steps)")

    def run_window(call, seconds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = 0
        while k == 0 or time.perf_counter() - t0 < seconds:
            call()
            stream.synchronize()
            k += 1
        return (time.perf_counter() - t0) / k

    for call in ways.values():
        for _ in range(args.warmup):
            call()
        stream.synchronize()
    lib.stats_discard()
    times = {w: [] for w in ways}
    for _ in range(args.reps):
        for w, call in ways.items():
            times[w].append(run_window(call, window))
        lib.stats_discard()
    out = {"rays": N, "max_positions": P, "frame": f"{W}x{H} stride {(W * H) // N}",
           "scene": f"kerr spin {SPIN} disk {list(DISK)}", "window_s": window, "reps": args.reps,
           "classes": classes, "longest_count": longest, "single_ray_rays": SINGLE, "ways": {}}
    for w in ways:
        med = statistics.median(times[w])
        out["ways"][w] = {"ms_per_call": round(med * 1e3, 4),
                          "ms_min_max": [round(min(times[w]) * 1e3, 4), round(max(times[w]) * 1e3, 4)],
                          "paths_per_s": round(n_paths[w] / med, 1),
                          "stored_points_per_s": round(points[w] / med, 1),
                          "steps_per_s": round(steps[w] / med, 1),
                          "steps_per_call": steps[w], "stored_points_per_call": points[w]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
