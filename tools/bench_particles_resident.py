"""The visualizer's physics tick (update, then the arrays a renderer draws) three ways: one JSON
line per system size on stdout, a table of the kernel times on stderr.

Per size (3 000 particles, the visualizer's; 65 536; 4 194 304 -- bench_particles.py's system: disk
particles plus 1/64 test particles), one process, --rounds interleaved rounds of three ways:
  a_host      bh_update_particles + bh_get_particle_data into host arrays: the whole Particle array
              crosses PCIe both ways per tick, and a serial host loop extracts;
  b_resident  bhrt_particles_update_device + bhrt_particles_extract into host arrays: the kernels,
              and the D2H of the bytes extracted;
  c_device    bhrt_particles_update_device + bhrt_particles_extract_device on one stream, no host
              copy, --depth ticks in flight.
A window is a host clock around ticks that end in a synchronise, at least --window seconds long; a
way's figure is the median over the rounds with the smallest and largest beside it (the spread).

The kernel times are HIP events around each kernel (bhrt_particles_kernel_ms): the update with the
plain kernel and with the counting kernel on the same resident array (each the second of two
launches, so that both follow an update pass), the scan, the scatter, and the count pass that create
and upload run; --kernel-reps repetitions after one warm-up. Beside each: the bytes that must move, and the fraction
of the 8 TB/s HBM roofline that bytes / time is.
"""
import argparse
import collections
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing-engine-in-c_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bhrt import abi, lib  # noqa: E402
from bench_particles import HBM_PEAK_GBS, make_system  # noqa: E402

P = C.POINTER
DT = 0.01


def spread(v, scale=1e3, digits=4):
    return {"median": round(statistics.median(v) * scale, digits),
            "min_max": [round(min(v) * scale, digits), round(max(v) * scale, digits)]}


def bench_size(torch, L, n, window, rounds, depth, kernel_reps):
    bh_ctx = L.bh_initialize()
    assert L.bh_configure_black_hole(bh_ctx, 1.0, 0.0, 0.0) == 0
    assert L.bh_configure_simulation(bh_ctx, DT, 100.0, 1000, 1e-6) == 0
    ps_host, bh = make_system(L, n)              # way a steps this one
    cfg = abi.sim_config(DT, 100.0, 1000, 1e-6)
    objs = [lib.particles_create(ps_host) for _ in range(3)]   # ways b and c, the kernel times
    pos, vel = np.zeros((n, 3)), np.zeros((n, 3))
    typ = np.zeros(n, dtype=np.int32)
    stream = torch.cuda.Stream()
    shapes = {"positions": ((n, 3), torch.float64), "velocities": ((n, 3), torch.float64),
              "types": ((n,), torch.int32), "xyz32": ((n, 3), torch.float32), "count": ((1,), torch.int32)}
    dev = {f: torch.zeros(s, dtype=d, device="cuda") for f, (s, d) in shapes.items()}
    out_c = lib.particle_data(dev)
    # way b's host arrays: what bh_get_particle_data gives
    pos_b, vel_b, typ_b, cnt_b = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=np.int32), \
        np.zeros(1, dtype=np.int32)
    out_b = abi.ParticleData(positions=pos_b.ctypes.data, velocities=vel_b.ctypes.data,
                             types=typ_b.ctypes.data, count=cnt_b.ctypes.data)
    torch.cuda.synchronize()
    active = [0, 0, 0]

    def tick_a():
        assert L.bh_update_particles(bh_ctx, C.byref(ps_host)) == 0, lib.last_error()
        cnt = C.c_int(n)
        assert L.bh_get_particle_data(bh_ctx, C.byref(ps_host), pos.ctypes.data, vel.ctypes.data,
                                      typ.ctypes.data, C.byref(cnt)) == 0
        active[0] = cnt.value

    def tick_b():
        lib.particles_update_device(objs[0], bh, cfg, 1, None)
        assert L.bhrt_particles_extract(objs[0], n, C.byref(out_b)) == 0, lib.last_error()
        active[1] = int(cnt_b[0])

    def tick_c():
        lib.particles_update_device(objs[1], bh, cfg, 1, stream.cuda_stream)
        lib.particles_extract_device(objs[1], n, out_c, stream.cuda_stream)

    def run_window(tick, in_flight):
        torch.cuda.synchronize()
        pending = collections.deque()
        t0 = time.perf_counter()
        k = 0
        while k == 0 or time.perf_counter() - t0 < window:
            tick()
            if in_flight:
                ev = torch.cuda.Event()
                ev.record(stream)
                pending.append(ev)
                if len(pending) > depth:
                    pending.popleft().synchronize()
            k += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k, k

    ways = {"a_host": (tick_a, False), "b_resident": (tick_b, False), "c_device": (tick_c, True)}
    try:
        for tick, _ in ways.values():            # warm-up
            for _ in range(3):
                tick()
            torch.cuda.synchronize()
        times = {w: [] for w in ways}
        ticks = {w: 0 for w in ways}
        for _ in range(rounds):
            for w, (tick, in_flight) in ways.items():
                t, k = run_window(tick, in_flight)
                times[w].append(t)
                ticks[w] += k
        active[2] = int(dev["count"].cpu()[0])
        res = {w: dict(tick_ms=spread(times[w]), ticks_timed=ticks[w]) for w in ways}
        a = res["a_host"]["tick_ms"]
        res["a_host"]["spread_of_a"] = round((a["min_max"][1] - a["min_max"][0]) / a["median"], 4)
        for w in ("b_resident", "c_device"):
            res[w]["a_over_this"] = round(a["median"] / res[w]["tick_ms"]["median"], 2)
        # kernel times: HIP events, the plain and the counting update on the same resident array
        k_ms = collections.defaultdict(list)
        for r in range(kernel_reps + 1):
            ms = lib.particles_kernel_ms(objs[2], bh, cfg, n, out_c)
            if r:
                for name, v in ms.items():
                    k_ms[name].append(v * 1e-3)
        written = int(dev["count"].cpu()[0])
        nblocks = (n + 255) // 256
        extracted = 24 + 24 + 4 + 12      # positions, velocities, types, xyz32 per particle written
        need = {"update_plain": 304 * n, "update_counted": 304 * n + 4 * nblocks,
                "scan": 4 * nblocks + 4 * (nblocks + 1),
                "scatter": 4 * (nblocks + 1) + 4 * n + written * (24 + 24 + 4 + extracted) + 4,
                "count_pass": 4 * n + 4 * nblocks}
        kern = {}
        for name, v in k_ms.items():
            med = statistics.median(v)
            gbs = need[name] / med / 1e9
            kern[name] = {"ms": spread(v), "bytes": need[name], "GB_per_s": round(gbs, 1),
                          "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)}
        plain, counted = kern["update_plain"]["ms"], kern["update_counted"]["ms"]
        kern["counted_minus_plain_ms"] = round(counted["median"] - plain["median"], 4)
        kern["plain_spread_ms"] = round(plain["min_max"][1] - plain["min_max"][0], 4)
        tick_kernels = counted["median"] + kern["scan"]["ms"]["median"] + kern["scatter"]["ms"]["median"]
        res["c_device"]["kernels_ms"] = round(tick_kernels, 4)
        return {"workload": f"physics tick, {n} particles (1/64 geodesic test particles)",
                "particles": n, "active": {"a": active[0], "b": active[1], "c": active[2]},
                "window_s": window, "rounds": rounds, "depth": depth, "ticks": res,
                "kernels": kern, "kernel_reps": kernel_reps}
    finally:
        torch.cuda.synchronize()
        for o in objs:
            lib.particles_destroy(o)
        L.bh_shutdown(bh_ctx)


def table(lines):
    rows = ["kernel times, HIP events (ms: median [min, max]); bytes that must move; GB/s; "
            f"fraction of the {HBM_PEAK_GBS:.0f} GB/s HBM roofline"]
    for r in lines:
        rows.append(f"{r['particles']} particles ({r['kernel_reps']} repetitions)")
        for name in ("update_plain", "update_counted", "scan", "scatter", "count_pass"):
            k = r["kernels"][name]
            rows.append(f"  {name:15s} {k['ms']['median']:9.4f} [{k['ms']['min_max'][0]:.4f}, "
                        f"{k['ms']['min_max'][1]:.4f}]  {k['bytes']:>11d} B  {k['GB_per_s']:8.1f} GB/s  "
                        f"{k['hbm_frac']:.4f}")
        rows.append(f"  counted - plain {r['kernels']['counted_minus_plain_ms']:+.4f} ms; the plain "
                    f"kernel's own spread {r['kernels']['plain_spread_ms']:.4f} ms")
        t = r["ticks"]
        rows.append(f"  tick ms: a {t['a_host']['tick_ms']['median']} (spread "
                    f"{t['a_host']['spread_of_a']}), b {t['b_resident']['tick_ms']['median']} "
                    f"(a/b {t['b_resident']['a_over_this']}), c {t['c_device']['tick_ms']['median']} "
                    f"(a/c {t['c_device']['a_over_this']}; its kernels {t['c_device']['kernels_ms']})")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="3000,65536,4194304")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--depth", type=int, default=3, help="ticks in flight (way c)")
    ap.add_argument("--kernel-reps", type=int, default=9)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_particles_resident.py needs a HIP device (no CPU path)")
    L = lib.load()
    L.bh_initialize.restype = C.c_void_p
    L.bh_shutdown.argtypes = [C.c_void_p]
    L.bh_configure_black_hole.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double]
    L.bh_configure_simulation.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double]
    L.bh_update_particles.argtypes = [C.c_void_p, C.c_void_p]
    L.bh_get_particle_data.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       P(C.c_int)]
    lines = []
    for n in (int(v) for v in args.sizes.split(",")):
        lines.append(bench_size(torch, L, n, args.window, args.rounds, args.depth, args.kernel_reps))
        print(json.dumps(lines[-1]), flush=True)
    print(table(lines), file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
