#!/usr/bin/env python3
"""How large are the angle shifts of the C2 trace loop (bhrt_trace_core.h shift_or_eval, shift_chain)?

The a = 0 RK4 iteration takes six sin/cos by angle addition from a nearby known angle: stage 2,
3, 4 of ray_derivatives' theta (= state[1]) from stage 1 (delta = h/2 k1, h/2 k2, h k3 of
component 1), and the advance of state[1], [2], [3] by one step. The polynomials of a shift are
fitted to |delta| <= T (the fast path); a lane beyond T takes the wide shift, and a wave runs that
branch whenever ANY of its lanes needs it. This replays the C2 scene's RK4 in numpy (literal
ray_derivatives, raytracer.c:44-154; every ray run to its oracle step count) on a camera frame
and reports, per site and threshold T, the fraction of lane evaluations beyond T and the fraction
of 8x8-tile "waves" (a wave's 64 lanes = one claim tile) with any lane beyond T.

Two more sites are the chained anchors (shift_chain): stage 3 shifted from stage 2's angle
(theta3 - theta2 = h/2 (k2 - k1)[1]) and the advance of state[1] shifted from stage 4's angle
(theta' - theta4); both differences are second order in h. Per site the largest |delta| of the
frame is printed, and beside the tile count the mixed-wave model: a refilled wave holds rays of
every regime, so its 64 lanes are taken as independent draws and a wave evaluation leaves the
fast path with probability 1 - (1 - p)^64, p the lane fraction beyond T. Where that is at most
1e-4 (marked "ok") a narrower polynomial on T costs no wave its branch; where it is not, measure
(profiles/shiftchain/ab_parent_vs_new.txt: the views down the polar axis).

The replay also counts what the high-word filter of the plain-value test (all_below_2)
holds back: lane-stages whose raw accelerations hold a |d| >= 2 or a non-finite
value -- they take the exact |d| <= 10 test in the rare block -- and, of those, the ones the exact
test fails too (the literal form, as before), with the same tile and mixed-wave figures.

--ages adds the per-age table: for the four far-anchor sites (stage 2's and stage 4's theta, the
advances of state[2] and state[3]) the lanes beyond 1/64 by the ray's iteration index, and the
settled age K after which none is (profiles/nursery/shift_ages.txt).

  python tools/shift_deltas.py [W H] [--cam B | --cam x,y,z,fov] [--ages]
                                                        (default 480x270, B; CPU only)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing-engine-in-c_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from bhrt import abi, configs  # noqa: E402
import oracle as orc  # noqa: E402

SITES = ("stage2", "stage3", "stage4", "adv_y1", "adv_y2", "adv_y3", "stage3_from2",
         "adv_y1_from4")
TS = (1 / 16, 1 / 32, 1 / 64, 1 / 128, 1 / 1024)
# the far-anchor sites (shifts from the iteration's start) and the narrow-first bound, for the
# per-age table (--ages)
AGE_SITES = ("stage2", "stage4", "adv_y2", "adv_y3")
AGE_BOUND = 1 / 64
MODEL_MAX = 1e-4  # mixed-wave model: at most this share of wave evaluations beyond the bound


def parse_camera(spec):
    """"B" (a configs.CAMERAS name) or "x,y,z,fov": at (x, y, z) looking at the origin, up +z."""
    if spec in configs.CAMERAS:
        return configs.camera(spec)
    x, y, z, fov = (float(v) for v in spec.split(","))
    return abi.Camera(abi.v3(x, y, z), abi.v3(-x, -y, -z), abi.v3(0.0, 0.0, 1.0), fov)


def replay(cam, W, H, oracle=None):
    """The C2 scene's frame of `cam` replayed step by step. Returns a dict: lane_evals,
    wave_evals, and per site lane_over / wave_over (one count per threshold of TS) and max."""
    c = configs.CONFIGS["C2"]
    bh, dk, cfg = c.scene()
    rays = configs.camera_rays(cam, W, H)
    ref = (oracle or orc.oracle()).trace_rays(rays, bh, dk, cfg, c.method, c.flags)
    # iterations each ray executes: steps (+1 for HORIZON / MAX_DISTANCE exits; DISK: steps)
    iters = ref["steps"].astype(np.int64) + np.isin(ref["result"], (abi.RAY_HORIZON,
                                                                    abi.RAY_MAX_DISTANCE))
    M, rs, dt = bh.mass, bh.schwarzschild_radius, cfg.time_step
    o = rays["origin"][0]
    r0 = float(np.sqrt(o @ o))
    th0, ph0 = np.arccos(o[2] / r0), np.arctan2(o[1], o[0]) % (2 * np.pi)
    d = rays["direction"] / np.linalg.norm(rays["direction"], axis=1)[:, None]
    st, ct, sp, cp = np.sin(th0), np.cos(th0), np.sin(ph0), np.cos(ph0)
    vr = st * cp * d[:, 0] + st * sp * d[:, 1] + ct * d[:, 2]
    vth = (ct * cp * d[:, 0] + ct * sp * d[:, 1] - st * d[:, 2]) / r0
    vph = (-sp * d[:, 0] + cp * d[:, 1]) / (r0 * st)
    rm = max(r0, rs + 1e-10)
    g_tt, g_rr, g_hh = -(1 - rs / rm), 1 / (1 - rs / rm), rm * rm
    vt = np.sqrt(np.maximum(-(g_rr * vr * vr + g_hh * vth * vth + g_hh * vph * vph) / g_tt, 0.0))
    n = len(rays)
    y = np.stack([np.zeros(n), np.full(n, r0), np.full(n, th0), np.full(n, ph0), vt, vr])

    def derivs(s):
        r, th, v_r, v_th, v_ph = s[0].copy(), s[1], s[3], s[4], s[5]
        out = np.empty_like(s)
        out[0], out[1], out[2] = v_r, v_th, v_ph
        sn = np.sin(th)
        r = np.where(r <= rs * 1.5, rs * 1.5, r)
        sn = np.where(np.abs(sn) < 0.01, np.where(sn >= 0, 0.01, -0.01), sn)
        with np.errstate(all="ignore"):
            f = 1.0 - rs / r
            out[3] = -M / (r * r * f) * f + r * v_th * v_th + r * sn * sn * v_ph * v_ph
            out[4] = -2.0 * v_r * v_th / r + sn * np.cos(th) * v_ph * v_ph
            out[5] = -2.0 * v_r * v_ph / r - 2.0 * v_th * v_ph * np.cos(th) / sn
        with np.errstate(invalid="ignore"):
            mag = np.abs(out[3:])
            flags.append((~(mag < 2.0).all(axis=0), ~(mag <= 10.0).all(axis=0)))
        out[3:] = np.clip(np.nan_to_num(out[3:], nan=0.0, posinf=0.0, neginf=0.0), -10, 10)
        return out

    flags = []  # per stage of the current iteration: (some |d| >= 2 or non-finite, exact test fails)
    accel = dict(stage_evals=0, wave_stage_evals=0, lane_over2=0, wave_over2=0, lane_over10=0,
                 wave_over10=0)

    out = {s: dict(lane_over=np.zeros(len(TS)), wave_over=np.zeros(len(TS)), max=0.0)
           for s in SITES}
    # per age (1-based iteration index of a ray: every ray of the replay starts together, so the
    # loop index is the age): lanes alive, and lanes beyond 1/64 at each far-anchor site
    kmax = int(iters.max()) if n else 0
    ages = {s: np.zeros(kmax, dtype=np.int64) for s in AGE_SITES}
    ages["alive"] = np.zeros(kmax, dtype=np.int64)
    lane_evals = wave_evals = 0
    # tiles of 8x8 pixels as waves
    px, py = np.arange(n) % W, np.arange(n) // W
    tile = (py // 8) * ((W + 7) // 8) + px // 8
    ntile = tile.max() + 1
    for k in range(int(iters.max())):
        alive = iters > k
        if not alive.any():
            break
        r = y[1]
        h = np.where(r < rs * 2.5, min(dt * 0.001, 0.1),
                     np.where(r < rs * 5, min(dt * 0.01, 0.1),
                              np.where(r < rs * 15, min(dt * 0.1, 0.1), min(dt, 0.1))))
        flags.clear()
        k1 = derivs(y)
        k2 = derivs(y + 0.5 * h * k1)
        k3 = derivs(y + 0.5 * h * k2)
        k4 = derivs(y + h * k3)
        ynew = y + h * (k1 + 2 * k2 + 2 * k3 + k4) / 6.0
        deltas = {"stage2": 0.5 * h * k1[1], "stage3": 0.5 * h * k2[1], "stage4": h * k3[1],
                  "adv_y1": ynew[1] - y[1], "adv_y2": ynew[2] - y[2], "adv_y3": ynew[3] - y[3],
                  "stage3_from2": 0.5 * h * (k2[1] - k1[1]),
                  "adv_y1_from4": ynew[1] - (y[1] + h * k3[1])}
        lane_evals += int(alive.sum())
        tiles_alive = np.bincount(tile[alive], minlength=ntile) > 0
        wave_evals += int(tiles_alive.sum())
        ages["alive"][k] = int(alive.sum())
        for s in AGE_SITES:
            ages[s][k] = int((alive & (np.abs(deltas[s]) > AGE_BOUND)).sum())
        for s, dl in deltas.items():
            a = np.abs(dl)
            out[s]["max"] = max(out[s]["max"], float(a[alive].max()))
            for j, T in enumerate(TS):
                over = alive & (a > T)
                out[s]["lane_over"][j] += over.sum()
                out[s]["wave_over"][j] += (np.bincount(tile[over], minlength=ntile) > 0).sum()
        for over2, over10 in flags:
            accel["stage_evals"] += int(alive.sum())
            accel["wave_stage_evals"] += int(tiles_alive.sum())
            for name, f in (("over2", over2), ("over10", over10)):
                accel["lane_" + name] += int((alive & f).sum())
                accel["wave_" + name] += int((np.bincount(tile[alive & f], minlength=ntile) > 0).sum())
        y = np.where(alive, ynew, y)
    out["lane_evals"], out["wave_evals"] = lane_evals, wave_evals
    out["accel"] = accel
    out["ages"] = ages
    return out


def settled_age(ages):
    """The smallest K such that no lane of age > K is beyond AGE_BOUND at any far-anchor site
    (0: no lane ever is): the iterations a ray needs before it is "settled"."""
    any_over = np.zeros(len(ages["alive"]), dtype=bool)
    for s in AGE_SITES:
        any_over |= ages[s] > 0
    idx = np.nonzero(any_over)[0]
    return int(idx[-1]) + 1 if len(idx) else 0


def print_ages(res, rows=12):
    ages = res["ages"]
    K = settled_age(ages)
    print(f"per age (iteration index of a ray, 1-based): lanes alive, lanes beyond 1/{round(1 / AGE_BOUND)} "
          f"at the far-anchor sites {', '.join(AGE_SITES)}")
    print(f"{'age':>5s} {'alive':>9s} " + " ".join(f"{s:>9s}" for s in AGE_SITES))
    for k in range(min(max(rows, K + 2), len(ages["alive"]))):
        print(f"{k + 1:5d} {ages['alive'][k]:9d} " + " ".join(f"{ages[s][k]:9d}" for s in AGE_SITES))
    tail = {s: int(ages[s][rows:].sum()) for s in AGE_SITES}
    print(f"ages {rows + 1}..{len(ages['alive'])}: " + ", ".join(f"{s} {v}" for s, v in tail.items()))
    total = sum(int(ages[s].sum()) for s in AGE_SITES)
    print(f"settled age K = {K}: no lane older than K iterations is beyond the bound at any of the "
          f"four sites ({total} lane-site cases beyond it in all)")


def mixed_wave(p):
    """Probability that any of 64 independent lanes is beyond the bound."""
    return 1.0 - (1.0 - p) ** 64


def main(argv):
    cam_spec = "B"
    if "--cam" in argv:
        i = argv.index("--cam")
        cam_spec = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    with_ages = "--ages" in argv
    argv = [a for a in argv if a != "--ages"]
    W, H = (int(argv[0]), int(argv[1])) if len(argv) > 1 else (480, 270)
    res = replay(parse_camera(cam_spec), W, H)
    le, we = res["lane_evals"], res["wave_evals"]
    print(f"C2 camera {cam_spec} {W}x{H}: {le} lane-iterations, {we} tile-iterations")
    print("per threshold T: lane fraction beyond T, 8x8-tile fraction, mixed-wave model "
          "1-(1-p)^64 (ok: <= 1e-4)")
    print(f"{'site':13s} {'max|delta|':>10s}  " + "  ".join(f"{'T=1/%d' % round(1 / T):>32s}"
                                                              for T in TS))
    for s in SITES:
        cells = []
        for j in range(len(TS)):
            p = res[s]["lane_over"][j] / le
            m = mixed_wave(p)
            cells.append(f"{p:9.2e} {res[s]['wave_over'][j] / we:9.2e} {m:9.2e}"
                         f"{' ok' if m <= MODEL_MAX else '   '}")
        print(f"{s:13s} {res[s]['max']:10.3e}  " + "  ".join(cells))
    a = res["accel"]
    print(f"plain-value test, {a['stage_evals']} lane-stages, {a['wave_stage_evals']} tile-stages: "
          "lane fraction, 8x8-tile fraction, mixed-wave model")
    for name, what in (("over2", "held back by the high-word filter (some |d| >= 2 or non-finite)"),
                       ("over10", "failing the exact test too (literal form)")):
        p = a["lane_" + name] / a["stage_evals"]
        print(f"  {what:66s} {p:9.2e} {a['wave_' + name] / a['wave_stage_evals']:9.2e} "
              f"{mixed_wave(p):9.2e}")
    if with_ages:
        print_ages(res)


if __name__ == "__main__":
    main(sys.argv[1:])
