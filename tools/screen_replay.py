#!/usr/bin/env python3
"""What does the disk screen of the C2 trace loop (bhrt_trace_core.h disk_cand) decide, and how early?

Replays the C2 scene's RK4 iteration in numpy as tools/shift_deltas.py does (literal
ray_derivatives, raytracer.c:44-154), and with it the Cartesian point of every iteration, the
screen's terms on the segment (p_k, p_{k-1}) and this tree's exits (disk by the literal decision,
horizon, distance, step budget), so it needs no GPU and no oracle library. Per camera it prints the
frame's classes and mean iterations per ray, and the fraction of lane-evaluations, and of 8x8-tile
evaluations (a tile is the kernel's claim unit, hence a wave: counted when EVERY live lane of the
tile agrees), that

  sign      the sign test rejects (den (num + 2^-1000 den) < 0),
  far x     the far test on x rejects (sx^2 > out_sq den^2, |den| < 2^100),
  far y     the far test on y rejects,
  x then y  either far test rejects (per lane: a tile counts when each live lane is rejected by
            one of the two),
  full      the full screen rejects,

and the median |q_xy| of the candidate point. The arithmetic is numpy's, unfused: the figures are
statistics, not bit-exact decisions (tests/far_screen_rule.py has the exact rule).

Not valid for a camera on the polar axis (sin theta0 = 0 takes another set-up branch in
init_velocity): camera A is judged on the GPU.

  python tools/screen_replay.py [W H] [--cam B | --cam x,y,z,fov]...   (default 240x135, B)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytracing-engine-in-c_amd"))
from bhrt import abi, configs  # noqa: E402

TESTS = ("sign", "far x", "far y", "x then y", "full")
CLASSES = {"disk": abi.RAY_DISK, "horizon": abi.RAY_HORIZON, "max_distance": abi.RAY_MAX_DISTANCE,
           "max_steps": abi.RAY_MAX_STEPS}


def parse_camera(spec):
    """"B" (a configs.CAMERAS name) or "x,y,z,fov": at (x, y, z) looking at the origin, up +z."""
    if spec in configs.CAMERAS:
        return configs.camera(spec)
    x, y, z, fov = (float(v) for v in spec.split(","))
    return abi.Camera(abi.v3(x, y, z), abi.v3(-x, -y, -z), abi.v3(0.0, 0.0, 1.0), fov)


def replay(cam, W, H):
    c = configs.CONFIGS["C2"]
    bh, dk, cfg = c.scene()
    rays = configs.camera_rays(cam, W, H)
    M, rs, dt = bh.mass, bh.schwarzschild_radius, cfg.time_step
    max_steps, max_dist = cfg.max_integration_steps, cfg.max_ray_distance
    in_sq, out_sq = dk.inner_radius ** 2, dk.outer_radius ** 2
    o = rays["origin"][0]
    r0 = float(np.sqrt(o @ o))
    th0, ph0 = np.arccos(o[2] / r0), np.arctan2(o[1], o[0]) % (2 * np.pi)
    if abs(np.sin(th0)) < 1e-10:
        raise SystemExit("camera on the polar axis: not covered by this replay")
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
        out[3:] = np.clip(np.nan_to_num(out[3:], nan=0.0, posinf=0.0, neginf=0.0), -10, 10)
        return out

    px, py = np.arange(n) % W, np.arange(n) // W
    tile = (py // 8) * ((W + 7) // 8) + px // 8
    ntile = tile.max() + 1
    p = np.tile(o, (n, 1)).astype(np.float64)
    dist = np.zeros(n)
    result = np.full(n, -1)
    steps = np.zeros(n, dtype=np.int64)
    iters = np.zeros(n, dtype=np.int64)
    alive = np.ones(n, dtype=bool)
    lane = dict.fromkeys(TESTS, 0)
    wave = dict.fromkeys(TESTS, 0)
    lane_evals = wave_evals = 0
    rq = []
    for k in range(1, max_steps + 1):
        if not alive.any():
            break
        r = y[1]
        h = np.where(r < rs * 2.5, min(dt * 0.001, 0.1),
                     np.where(r < rs * 5, min(dt * 0.01, 0.1),
                              np.where(r < rs * 15, min(dt * 0.1, 0.1), min(dt, 0.1))))
        k1 = derivs(y)
        k2 = derivs(y + 0.5 * h * k1)
        k3 = derivs(y + 0.5 * h * k2)
        k4 = derivs(y + h * k3)
        y = np.where(alive, y + h * (k1 + 2 * k2 + 2 * k3 + k4) / 6.0, y)
        q = np.stack([y[1] * np.sin(y[2]) * np.cos(y[3]), y[1] * np.sin(y[2]) * np.sin(y[3]),
                      y[1] * np.cos(y[2])], axis=1)
        prev, p = p, np.where(alive[:, None], q, p)
        dist = dist + np.where(alive, np.sqrt(((p - prev) ** 2).sum(axis=1)), 0.0)
        iters += alive
        # the screen on segment k: plane "normal" = the previous point, straight line along d
        with np.errstate(all="ignore"):
            den = (d * prev).sum(axis=1)
            num = -(p * prev).sum(axis=1)
            d2 = den * den
            sx = d[:, 0] * num + p[:, 0] * den
            sy = d[:, 1] * num + p[:, 1] * den
            S = sx * sx + sy * sy
            small = np.abs(den) < 2.0 ** 100
            rej = {"sign": den * (2.0 ** -1000 * den + num) < 0.0,
                   "far x": (sx * sx > out_sq * d2) & small,
                   "far y": (sy * sy > out_sq * d2) & small}
            rej["x then y"] = rej["far x"] | rej["far y"]
            cand = ~rej["sign"] & (S >= in_sq * d2) & (S <= out_sq * d2) | ~small
            rej["full"] = ~cand
            t = num / den
            qx, qy = p[:, 0] + d[:, 0] * t, p[:, 1] + d[:, 1] * t
            s = qx * qx + qy * qy
            hit = cand & ~(np.abs(den) < 1e-10) & ~(t < 0.0) & (s >= in_sq) & (s <= out_sq) & \
                (k < max_steps)
        lane_evals += int(alive.sum())
        tiles_alive = np.bincount(tile[alive], minlength=ntile) > 0
        wave_evals += int(tiles_alive.sum())
        for name in TESTS:
            lane[name] += int((alive & rej[name]).sum())
            kept = np.bincount(tile[alive & ~rej[name]], minlength=ntile) > 0
            wave[name] += int((tiles_alive & ~kept).sum())
        rq.append(np.sqrt(s[alive & np.isfinite(s)]))
        # exits, the disk first
        end = np.where(hit, abi.RAY_DISK,
                       np.where(y[1] <= rs * 1.05, abi.RAY_HORIZON,
                                np.where(dist >= max_dist, abi.RAY_MAX_DISTANCE,
                                         np.where(k >= max_steps, abi.RAY_MAX_STEPS, -1))))
        done = alive & (end >= 0)
        result[done] = end[done]
        steps[done] = k
        alive &= ~done
    return dict(result=result, steps=steps, iters=iters, lane=lane, wave=wave,
                lane_evals=lane_evals, wave_evals=wave_evals,
                median_q=float(np.median(np.concatenate(rq))))


def main(argv):
    cams = []
    while "--cam" in argv:
        i = argv.index("--cam")
        cams.append(argv[i + 1])
        argv = argv[:i] + argv[i + 2:]
    W, H = (int(argv[0]), int(argv[1])) if len(argv) > 1 else (240, 135)
    for spec in cams or ["B"]:
        res = replay(parse_camera(spec), W, H)
        n = len(res["result"])
        le, we = res["lane_evals"], res["wave_evals"]
        print(f"C2 camera {spec} {W}x{H}: {n} rays, {res['iters'].mean():.1f} mean iterations per "
              f"ray, {le} lane-evaluations, {we} tile-evaluations, median |q_xy| {res['median_q']:.1f}")
        for name, code in CLASSES.items():
            m = res["result"] == code
            if m.any():
                print(f"  {name:13s} {m.mean():7.2%} of rays, mean steps {res['steps'][m].mean():7.1f}, "
                      f"{res['iters'][m].sum() / le:7.2%} of lane-evaluations")
        print(f"  {'rejected by':13s} {'lanes':>8s} {'8x8 tiles':>10s}")
        for name in TESTS:
            print(f"  {name:13s} {res['lane'][name] / le:8.2%} {res['wave'][name] / we:10.2%}")


if __name__ == "__main__":
    main(sys.argv[1:])
