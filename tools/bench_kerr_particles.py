"""The physical particle tick (bhrt_particles_kerr_update_device) timed beside the parity tick on
the same system and beside k_kerr's frame, in one process: one JSON line per system size.

Per size (4 194 304 and 3 000 particles, bench_particles_resident.py's sizes): a disk of prograde
circular orbits from the ISCO to 20 M with a plunging fraction (1/64 of the particles at rest
between 2.2 M and 5 M), spin 0.9, time_step 0.5, substeps 1. A round uploads the system afresh --
so that every round times the same particles, plungers included -- and issues --ticks ticks of one
step back to back on one stream with --depth in flight (the host waits only for the tick that many
back); a host clock around them, the median over --rounds rounds with the smallest and largest
beside it. The RK4 substeps of those ticks are counted by one more pass of the same ticks with the
`substeps` diagnostic, summed. The parity tick (bhrt_particles_update_device) runs the same way on
the same upload.

The yardstick: k_kerr's RK4 steps/s on bench_kerr.py's 1920x1080 spin-0.9 frame (the same `geom`
and `deriv`, four of each per step as a particle substep has), --depth frames in flight.

usage: python tools/bench_kerr_particles.py [--out FILE]   (FILE gets the JSON lines appended)"""
import argparse
import collections
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing-engine-in-c_amd"))
from bhrt import abi, lib  # noqa: E402

SPIN, MASS, DT, SUBSTEPS = 0.9, 1.0, 0.5, 1
PLUNGE_EVERY = 64


def make_particles(n, seed=1):
    """The benchmark's system as a numpy array of abi.PARTICLE_DTYPE."""
    rng = np.random.default_rng(seed)
    a = SPIN * MASS
    isco = abi.black_hole(MASS, SPIN).isco_radius
    r = rng.uniform(isco, 20.0, n)
    phi = rng.uniform(0.0, 2.0 * math.pi, n)
    plunge = np.arange(n) % PLUNGE_EVERY == PLUNGE_EVERY - 1
    r[plunge] = rng.uniform(2.2, 5.0, int(plunge.sum()))
    rho = np.sqrt(r * r + a * a)
    x, y = rho * np.cos(phi), rho * np.sin(phi)
    om = math.sqrt(MASS) / (r * np.sqrt(r) + a * math.sqrt(MASS))   # bhrt_kerr_orbit_velocity
    om[plunge] = 0.0
    p = np.zeros(n, dtype=abi.PARTICLE_DTYPE)
    p["position"] = np.stack([x, y, np.where(plunge, rng.uniform(-0.5, 0.5, n), 0.0)], axis=1)
    p["velocity"] = np.stack([om * -y, om * x, 0.0 * om], axis=1)
    p["mass"] = 1.0
    p["type"] = np.where(plunge, abi.PARTICLE_TEST, abi.PARTICLE_DISK)
    p["active"] = 1
    p["id"] = np.arange(1, n + 1)
    return p


def spread(v, scale=1e3, digits=4):
    return {"median": round(statistics.median(v) * scale, digits),
            "min_max": [round(min(v) * scale, digits), round(max(v) * scale, digits)]}


def bench_size(torch, n, ticks, rounds, depth):
    bh, cfg = abi.black_hole(MASS, SPIN), abi.sim_config(DT, 100.0, 1000, 1e-6)
    par = abi.KerrParticlesParams(SUBSTEPS)
    p = make_particles(n)
    system = abi.ParticleSystem(C.cast(p.ctypes.data, C.POINTER(abi.Particle)), n, n, n + 1, None)
    ps = lib.particles_create(system)
    stream = torch.cuda.Stream()
    sub = torch.zeros(n, dtype=torch.int32, device="cuda")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    diag = abi.KerrParticlesDiag(substeps=sub.data_ptr(), status=status.data_ptr())
    torch.cuda.synchronize()

    def physical(dg=None):
        lib.particles_kerr_update_device(ps, bh, cfg, 1, par, dg, stream.cuda_stream)

    def parity(dg=None):
        lib.particles_update_device(ps, bh, cfg, 1, stream.cuda_stream)

    def run_round(tick):
        lib.particles_upload(ps, system)
        torch.cuda.synchronize()
        pending = collections.deque()
        t0 = time.perf_counter()
        for _ in range(ticks):
            tick()
            ev = torch.cuda.Event()
            ev.record(stream)
            pending.append(ev)
            if len(pending) > depth:
                pending.popleft().synchronize()
        stream.synchronize()
        return (time.perf_counter() - t0) / ticks

    try:
        # the substeps of a round's ticks, and what became of the particles
        lib.particles_upload(ps, system)
        total, per_tick = 0, []
        for _ in range(ticks):
            physical(diag)
            stream.synchronize()
            per_tick.append(int(sub.sum().item()))
            total += per_tick[-1]
        statuses = np.bincount(status.cpu().numpy(), minlength=5).tolist()
        for tick in (physical, parity):     # warm-up
            run_round(tick)
        times = {"physical": [], "parity": []}
        for _ in range(rounds):
            times["physical"].append(run_round(physical))
            times["parity"].append(run_round(parity))
        med = statistics.median(times["physical"])
        return {"workload": f"physical particle tick, {n} particles, spin {SPIN}, dt {DT}, "
                            f"substeps {SUBSTEPS}, 1/{PLUNGE_EVERY} plungers",
                "particles": n, "ticks": ticks, "rounds": rounds, "depth": depth,
                "physical_tick_ms": spread(times["physical"]),
                "parity_tick_ms": spread(times["parity"]),
                "physical_over_parity": round(med / statistics.median(times["parity"]), 2),
                "substeps_per_round": total,
                "substeps_first_and_last_tick": [per_tick[0], per_tick[-1]],
                "gsubsteps_per_s": round(total / ticks / med / 1e9, 4),
                "status_after_last_tick": dict(zip(("moved", "captured", "not_timelike", "error",
                                                    "inactive"), statuses))}
    finally:
        torch.cuda.synchronize()
        lib.particles_destroy(ps)


def bench_k_kerr(torch, W, H, window, reps, depth):
    """k_kerr's RK4 steps/s on bench_kerr.py's frame, `depth` frames in flight."""
    n = W * H
    stream = torch.cuda.Stream()
    out8 = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    soa8 = abi.FrameSoA(rgba8=out8.data_ptr())
    bh, dk = abi.black_hole(1.0, SPIN), abi.disk(2.4, 12.0)
    cfg = abi.sim_config(0.25, 60.0, 2000)
    cam = abi.Camera(abi.v3(0.0, -18.0, 4.0), abi.v3(0.0, 18.0, -4.0), abi.v3(0.0, 0.0, 1.0), 40.0)

    def frame():
        lib.kerr_frame_device(bh, dk, cfg, cam, W, H, None, abi.BHRT_FLAG_DOPPLER, soa8, None,
                              stream.cuda_stream)

    torch.cuda.synchronize()
    lib.stats(reset=True)
    frame()
    stream.synchronize()
    steps = int(lib.stats(reset=True)["iterations"])
    for _ in range(2):
        frame()
    stream.synchronize()
    times = []
    for _ in range(reps):
        pending = collections.deque()
        t0 = time.perf_counter()
        k = 0
        while k == 0 or time.perf_counter() - t0 < window:
            frame()
            ev = torch.cuda.Event()
            ev.record(stream)
            pending.append(ev)
            if len(pending) >= depth:
                pending.popleft().synchronize()
            k += 1
        stream.synchronize()
        times.append((time.perf_counter() - t0) / k)
        lib.stats_discard()
    med = statistics.median(times)
    return {"workload": f"k_kerr frame {W}x{H}, spin {SPIN}, disk, doppler (bench_kerr.py's)",
            "steps_per_frame": steps, "frame_ms": spread(times), "depth": depth,
            "gsteps_per_s": round(steps / med / 1e9, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4194304,3000")
    ap.add_argument("--ticks", type=int, default=24, help="ticks per round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--depth", type=int, default=3, help="ticks (frames) in flight")
    ap.add_argument("--window", type=float, default=0.5, help="seconds per k_kerr window")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_kerr_particles.py needs a HIP device (no CPU path)")
    lib.load()
    lines = [bench_size(torch, int(v), args.ticks, args.rounds, args.depth)
             for v in args.sizes.split(",")]
    yard = bench_k_kerr(torch, 1920, 1080, args.window, args.rounds, args.depth)
    for l in lines:
        l["substeps_over_k_kerr_steps_rate"] = round(l["gsubsteps_per_s"] / yard["gsteps_per_s"], 3)
    for l in lines + [yard]:
        print(json.dumps(l), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
