"""Temporal accumulation frames (bhrt_accum_frame_device) against what a caller could do without
them: one JSON line per scene.

Per scene (camera B, Halton 8, rgba8 out), four ways to produce one display frame, timed in one
process in alternating windows after a warm-up:
  accum        bhrt_accum_frame_device, edges off (a NaN threshold: no edge launch);
  accum_edges  the same with the edge factors (threshold 0.1), edge_factor out as well;
  torch        the plain one-offset frame with rgba32f (bhrt_render_frame_device), then the same
               blend, edge and gamma steps as torch ops on the same stream;
  plain        the plain rgba8 frame alone.
Each way is timed twice: ONE FRAME AT A TIME (a stream synchronise after every frame) and IN
FLIGHT (frames issued back to back from one thread, the host waiting only for the frame --depth
frames back). A window is a host clock around frames, at least --window seconds long; the figure
of a way is the median over --reps windows with the smallest and largest beside it (the spread).
call_ms is the host time inside the accumulator's call and host_blocked_share its share of the
frame: the call returns without waiting for the GPU.

--profile runs a few accum_edges frames, one at a time, and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for the times of k_ta_blend and k_ta_edges.
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


def bench_scene(torch, name, W, H, spp, window, reps, warmup, depth, profile):
    c = configs.CONFIGS[name]
    bh, dk, cfg = c.scene()
    n = W * H
    ss = abi.SupersamplingParams(spp, abi.JITTER_HALTON, 1.0)
    offsets = lib.sample_offsets(ss)
    cam = configs.camera("B")
    stream = torch.cuda.Stream()
    out8 = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    edge_out = torch.zeros(n, dtype=torch.float32, device="cuda")
    buf32 = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
    t_acc = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    t_edge = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    soa8 = abi.FrameSoA(rgba8=out8.data_ptr())
    soa32 = abi.FrameSoA(rgba32f=buf32.data_ptr())
    acc_off = lib.accum_create(W, H, None, abi.AccumParams(edge_threshold=float("nan")))
    acc_on = lib.accum_create(W, H, None, None)
    o_off = abi.AccumOut(rgba8=out8.data_ptr())
    o_on = abi.AccumOut(rgba8=out8.data_ptr(), edge_factor=edge_out.data_ptr())
    torch.cuda.synchronize()
    call_s = []
    counter = [0]

    def frame_accum(acc=acc_off, out=o_off):
        t0 = time.perf_counter()
        lib.accum_frame_device(acc, bh, dk, cfg, cam, c.method, c.flags, ss, out,
                               stream.cuda_stream)
        call_s.append(time.perf_counter() - t0)

    def frame_accum_edges():
        frame_accum(acc_on, o_on)

    def frame_plain():
        lib.render_frame_device(bh, dk, cfg, cam, W, H, None, c.method, c.flags, soa8,
                                stream.cuda_stream)

    def frame_torch():
        k = counter[0]
        counter[0] += 1
        at = configs.camera("B")
        at.use_offset, at.offset_x, at.offset_y = 1, float(offsets[k % spp][0]), float(offsets[k % spp][1])
        lib.render_frame_device(bh, dk, cfg, at, W, H, None, c.method, c.flags, soa32,
                                stream.cuda_stream)
        alpha = float(lib.accum_alpha(None, min(k, 32)))
        with torch.cuda.stream(stream):
            t_acc.mul_(1.0 - alpha).add_(buf32[:, :3], alpha=alpha)
            A = t_acc.view(H, W, 3)
            ctr = A[1:-1, 1:-1]
            g = torch.zeros((H - 2, W - 2), dtype=torch.float32, device="cuda")
            for nb in (A[:-2, 1:-1], A[2:, 1:-1], A[1:-1, :-2], A[1:-1, 2:]):
                g = torch.maximum(g, (ctr - nb).abs().sum(dim=-1) / 3.0)
            E = t_edge[1:-1, 1:-1]
            E.copy_(torch.where(g > 0.1, torch.ones_like(g), (E - 0.2).clamp_min(0.0)))
            out8[:, :3] = (t_acc.clamp(0.0, 1.0).pow(1.0 / 2.2) * 255.0).to(torch.uint8)
            out8[:, 3] = 255

    try:
        if profile:
            for _ in range(warmup + 8):
                frame_accum_edges()
                stream.synchronize()
            return {"scene": name, "width": W, "height": H, "profiled_frames": warmup + 8}

        def run_window(frame, seconds, in_flight):
            """Frames until `seconds` have passed: (s per frame, frames)."""
            torch.cuda.synchronize()
            pending = collections.deque()
            t0 = time.perf_counter()
            k = 0
            while k == 0 or time.perf_counter() - t0 < seconds:
                frame()
                if in_flight:
                    ev = torch.cuda.Event()
                    ev.record(stream)
                    pending.append(ev)
                    if len(pending) > depth:
                        pending.popleft().synchronize()
                else:
                    stream.synchronize()
                k += 1
            stream.synchronize()
            return (time.perf_counter() - t0) / k, k

        ways = {"accum": frame_accum, "accum_edges": frame_accum_edges, "torch": frame_torch,
                "plain": frame_plain}
        for frame in ways.values():
            for _ in range(warmup):
                frame()
                stream.synchronize()
        lib.stats_discard()
        out = {"scene": name, "width": W, "height": H, "camera": "B", "pattern": "halton",
               "samples": spp, "window_s": window, "reps": reps, "depth": depth}
        for mode, in_flight in (("one_at_a_time", False), ("in_flight", True)):
            times = {w: [] for w in ways}
            frames = {w: 0 for w in ways}
            calls = {w: [] for w in ways}
            for _ in range(reps):
                for w, frame in ways.items():
                    del call_s[:]
                    t, k = run_window(frame, window, in_flight)
                    times[w].append(t)
                    frames[w] += k
                    if call_s:
                        calls[w].append(statistics.mean(call_s))
                lib.stats_discard()
            res = {}
            for w in ways:
                med = statistics.median(times[w])
                res[w] = {"frame_ms": round(med * 1e3, 4),
                          "frame_ms_min_max": [round(min(times[w]) * 1e3, 4),
                                               round(max(times[w]) * 1e3, 4)],
                          "frames_timed": frames[w]}
                if calls[w]:
                    call = statistics.median(calls[w])
                    res[w]["call_ms"] = round(call * 1e3, 4)
                    res[w]["host_blocked_share"] = round(call / med, 4)
            res["accum_minus_plain_ms"] = round(res["accum"]["frame_ms"] - res["plain"]["frame_ms"], 4)
            res["accum_edges_minus_plain_ms"] = round(res["accum_edges"]["frame_ms"] -
                                                      res["plain"]["frame_ms"], 4)
            res["torch_over_accum_edges"] = round(res["torch"]["frame_ms"] /
                                                  res["accum_edges"]["frame_ms"], 3)
            out[mode] = res
        return out
    finally:
        torch.cuda.synchronize()
        lib.accum_destroy(acc_off)
        lib.accum_destroy(acc_on)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="C2:1920x1080,C4:3840x2160")
    ap.add_argument("--samples", type=int, default=8, help="Halton samples of the jitter cycle")
    ap.add_argument("--window", type=float, default=0.6, help="seconds per timed window (>= 0.6)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=4, help="untimed frames of every way")
    ap.add_argument("--depth", type=int, default=3, help="frames in flight")
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_temporal.py needs a HIP device (no CPU path)")
    lib.load()
    for spec in args.scenes.split(","):
        name, size = spec.split(":")
        W, H = (int(v) for v in size.split("x"))
        print(json.dumps(bench_scene(torch, name, W, H, args.samples, args.window, args.reps,
                                     args.warmup, args.depth, args.profile)), flush=True)


if __name__ == "__main__":
    main()
