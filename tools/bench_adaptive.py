"""Adaptive supersampled frames (bhrt_render_frame_adaptive_device) against the supersampled
frame they approximate and the one-sample frame they extend: one JSON line per scene and
threshold.

Per scene (camera B, regular grid, B = 1, M = --samples, rgba8 only), four ways to spend the GPU,
timed in one process in alternating windows after a warm-up:
  adaptive  bhrt_render_frame_adaptive_device at the threshold;
  ss        bhrt_render_frame_ss_device with M samples at every pixel;
  single    the one-sample frame (bhrt_render_frame_device);
  extra     the adaptive frame's extra rays alone -- its E edge pixels at samples B..M-1 -- as
            one ray-array launch (bhrt_trace_rays_device): what the second pass costs by itself.
The adaptive call waits on the host for its base pass (the edge count decides the second
launch's size), so one thread cannot keep two such frames in flight; every way is therefore
timed ONE FRAME AT A TIME on one stream: a window is a host clock around frames each followed by
a stream synchronise, at least --window seconds long. The figure of a way is the median over
--reps windows, with the smallest and largest beside it (the spread). call_ms is the host time
inside the adaptive call (base pass, count copy, wait, second pass queued) and host_blocked_share
its share of the frame. The adaptive and ss images are compared once: the rgba8 pixels that differ,
how many of them are not edge pixels, and the largest byte step there (an edge pixel is the ss
frame's pixel bit for bit).

--profile runs a few adaptive frames, one at a time, and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the time of k_ad_rays, the two traces, k_ad_edges and
k_ad_resolve.
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
from bhrt import abi, configs, lib  # noqa: E402


def extra_rays(torch, cam, W, H, pixels, offsets):
    """AoS Ray[len(offsets) * len(pixels)] on the device: calculate_ray_direction
    (raytracer.c:999-1039) of the image pixels `pixels` at each offset, sample-major."""
    v = lambda a: torch.tensor([a.x, a.y, a.z], dtype=torch.float64, device="cuda")
    fwd = v(cam.direction)
    fwd = fwd / fwd.norm()
    right = torch.linalg.cross(fwd, v(cam.up))
    right = right / right.norm()
    up = torch.linalg.cross(right, fwd)
    plane_h = 2.0 * math.tan(cam.fov_deg * math.pi / 180.0 / 2.0)
    plane_w = plane_h * (W / H)
    px, py = (pixels % W).double(), (pixels // W).double()
    rays = torch.zeros((len(offsets) * len(pixels), 6), dtype=torch.float64, device="cuda")
    rays[:, 0:3] = v(cam.position)
    for s, (ox, oy) in enumerate(offsets):
        ndcx = (2.0 * ((px + float(ox)) / W) - 1.0) * plane_w
        ndcy = (1.0 - 2.0 * ((py + float(oy)) / H)) * plane_h
        d = fwd[None, :] + right[None, :] * ndcx[:, None] + up[None, :] * ndcy[:, None]
        rays[s * len(pixels):(s + 1) * len(pixels), 3:6] = d / d.norm(dim=1, keepdim=True)
    return rays


def bench_scene(torch, name, W, H, M, threshold, window, reps, warmup, profile):
    c = configs.CONFIGS[name]
    bh, dk, cfg = c.scene()
    n, B = W * H, 1
    ss = abi.SupersamplingParams(M, abi.JITTER_REGULAR_GRID, 1.0)
    as_ = abi.AdaptiveSamplingParams(1, B, M, 0.0, threshold)
    cam = configs.camera("B")
    stream = torch.cuda.Stream()
    out8 = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    samples = torch.zeros(n, dtype=torch.int32, device="cuda")
    soa8 = abi.FrameSoA(rgba8=out8.data_ptr())
    torch.cuda.synchronize()
    call_s = []

    def frame_adaptive():
        t0 = time.perf_counter()
        info = lib.render_frame_adaptive_device(bh, dk, cfg, cam, W, H, None, c.method, c.flags,
                                                ss, as_, soa8, samples.data_ptr(),
                                                stream.cuda_stream)
        call_s.append(time.perf_counter() - t0)
        return info

    def frame_ss():
        lib.render_frame_ss_device(bh, dk, cfg, cam, W, H, None, c.method, c.flags, ss, None,
                                   soa8, stream.cuda_stream)

    def frame_single():
        lib.render_frame_device(bh, dk, cfg, cam, W, H, None, c.method, c.flags, soa8,
                                stream.cuda_stream)

    if profile:
        for _ in range(warmup + 4):
            info = frame_adaptive()
            stream.synchronize()
        return {"scene": name, "width": W, "height": H, "max_samples": M, "threshold": threshold,
                "profiled_frames": warmup + 4, "edge_pixels": info["edge_pixels"]}

    # the two images once, and the adaptive frame's extra rays as a ray array
    frame_ss()
    stream.synchronize()
    img_ss = out8.clone()
    info = frame_adaptive()
    stream.synchronize()
    differ = int((img_ss != out8).any(dim=1).sum().item())
    step = (img_ss.int() - out8.int()).abs().max(dim=1).values   # per pixel, in bytes
    pixels = torch.nonzero(samples == M).flatten()
    E = int(pixels.numel())
    off_edge = samples != M
    differ_off = int((step[off_edge] > 0).sum().item())
    step_off = int(step[off_edge].max().item()) if differ_off else 0
    step_all = int(step.max().item())
    assert E == info["edge_pixels"], (E, info)
    rays = extra_rays(torch, cam, W, H, pixels, lib.sample_offsets(ss, as_)[B:M])
    out_x = torch.zeros((max(len(rays), 1), 4), dtype=torch.uint8, device="cuda")
    soa_x = abi.FrameSoA(rgba8=out_x.data_ptr())
    torch.cuda.synchronize()

    def frame_extra():
        if len(rays):
            lib._check(lib.load().bhrt_trace_rays_device(rays.data_ptr(), len(rays), lib._ptr(bh),
                                                         lib._ptr(dk), lib._ptr(cfg), c.method,
                                                         c.flags, lib._ptr(soa_x),
                                                         stream.cuda_stream),
                       "bhrt_trace_rays_device")

    def run_window(frame, seconds):
        """Frames one at a time, each followed by a stream synchronise, until `seconds` have
        passed; returns (s per frame, frames)."""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k = 0
        while k == 0 or time.perf_counter() - t0 < seconds:
            frame()
            stream.synchronize()
            k += 1
        return (time.perf_counter() - t0) / k, k

    ways = {"adaptive": frame_adaptive, "ss": frame_ss, "single": frame_single,
            "extra": frame_extra}
    for frame in ways.values():
        for _ in range(warmup):
            frame()
            stream.synchronize()
    lib.stats_discard()
    times = {w: [] for w in ways}
    frames = {w: 0 for w in ways}
    calls = []
    for _ in range(reps):
        for w, frame in ways.items():
            del call_s[:]
            t, k = run_window(frame, window)
            times[w].append(t)
            frames[w] += k
            if w == "adaptive":
                calls.append(statistics.mean(call_s))
        lib.stats_discard()
    out = {"scene": name, "width": W, "height": H, "camera": "B", "pattern": "regular grid",
           "min_samples": B, "max_samples": M, "threshold": threshold, "window_s": window,
           "reps": reps, "one_frame_at_a_time": True,
           "edge_pixels": E, "edge_fraction": round(E / n, 6),
           "sample_rays": info["sample_rays"], "rays_over_single": round(info["sample_rays"] / n, 4),
           "extra_rays": len(rays),
           "rgba8_pixels_differing_from_ss": differ,
           "rgba8_pixels_differing_off_edge": differ_off,
           "rgba8_largest_byte_step_off_edge": step_off, "rgba8_largest_byte_step": step_all}
    for w in ways:
        med = statistics.median(times[w])
        out[w] = {"frame_ms": round(med * 1e3, 4),
                  "frame_ms_min_max": [round(min(times[w]) * 1e3, 4), round(max(times[w]) * 1e3, 4)],
                  "frames_timed": frames[w]}
    ad, one = out["adaptive"]["frame_ms"], out["single"]["frame_ms"]
    out["adaptive"]["call_ms"] = round(statistics.median(calls) * 1e3, 4)
    out["adaptive"]["host_blocked_share"] = round(statistics.median(calls) * 1e3 / ad, 4)
    out["ss_over_adaptive"] = round(out["ss"]["frame_ms"] / ad, 3)
    out["adaptive_minus_single_ms"] = round(ad - one, 4)
    out["adaptive_minus_single_minus_extra_ms"] = round(ad - one - out["extra"]["frame_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="C2:1920x1080,C4:3840x2160")
    ap.add_argument("--samples", type=int, default=4, help="max_samples (min_samples is 1)")
    ap.add_argument("--thresholds", default="0.1,0.02")
    ap.add_argument("--window", type=float, default=0.6, help="seconds per timed window (>= 0.5)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=4, help="untimed frames of every way")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_adaptive.py needs a HIP device (no CPU path)")
    lib.load()
    for spec in args.scenes.split(","):
        name, size = spec.split(":")
        W, H = (int(v) for v in size.split("x"))
        for thr in (float(t) for t in args.thresholds.split(",")):
            print(json.dumps(bench_scene(torch, name, W, H, args.samples, thr, args.window,
                                         args.reps, args.warmup, args.profile)), flush=True)


if __name__ == "__main__":
    main()
