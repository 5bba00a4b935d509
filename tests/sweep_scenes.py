"""Scenes off the five baseline configurations (the scene sweep).

A plain table shared by tests/golden/gen_golden.py (group `sweep`), the CPU tests and the GPU
tests of tests/test_scene_sweep.py. The baseline configurations (bhrt.configs) fix mass 1,
spin 0 / 0.9 / 0.99, dt 0.1, distance 100, disk (ISCO, 20) and tol 1e-6 / 1e-8; the host derives
step-size intervals, the far-field switch, the no-evict and bounded-state proofs, the rotation
bound, the RKF45 accept-all switch and the disk radius bounds from exactly those parameters.
Every scene here moves at least one of them.

    scene(name) -> (bh, dk, cfg, method, flags, cams)

The black hole is abi.black_hole(mass, spin): spin is dimensionless (a = spin * mass). All
frames of the sweep are W x H = 48 x 27 (1296 rays: several 256-lane blocks and a ragged tail).

Choices that avoid threshold coincidences:
  * M = 2.4, not 2.5: at 2.5, 15 rs = 75 = |W| puts every ray of camera W exactly on the
    far-field threshold (margin 0 for the whole frame);
  * no camera exactly on the polar axis beyond 15 rs (cameras A and V at M = 0.5, V at M = 2.4):
    the oracle's margin is 0 for every ray there, so the knife-edge rule would excuse the whole
    frame (the frame_C2_V fixture covers that path with a strict compare);
  * no M = 0 (abi.black_hole(0, spin != 0) divides by zero).
"""
import math

import numpy as np

from bhrt import abi, configs

W, H = 48, 27

# position, up, fov; direction = -position (looking at the origin). B is the baseline camera.
CAMERAS = {
    "B": None,                                        # configs.camera("B"); r0 = 30
    "N": ((9.0, -4.0, 1.5), (0.0, 0.0, 1.0), 60.0),   # near: r0 < 5 rs at M = 1
    "P": ((0.3, -0.2, 30.0), (0.0, 1.0, 0.0), 60.0),  # next to the polar axis, not st_tiny
    "W": ((1.0, 0.5, 75.0), (0.0, 1.0, 0.0), 40.0),   # far: r0 > 15 rs up to M = 2.4
    "E": ((0.0, -40.0, 0.25), (0.0, 0.0, 1.0), 60.0),  # disk nearly edge-on
    "S": ((3.0, 2.0, -26.0), (0.0, 1.0, 0.0), 75.0),  # southern hemisphere
    "I": ((2.9, 0.3, 0.4), (0.0, 0.0, 1.0), 90.0),    # inside 1.5 rs at M = 1
}

RK4, RKF45, LEAPFROG = abi.INTEGRATOR_RK4, abi.INTEGRATOR_RKF45, abi.INTEGRATOR_LEAPFROG
D = abi.BHRT_FLAG_DOPPLER
ISCO = "isco"
INF, NAN = math.inf, math.nan

# name: (mass, spin, method, dt, max_dist, max_steps, tol, disk (inner, outer) or None, flags,
#        cameras)
SCENES = {
    "m05_rk4":        (0.5, 0.0, RK4, 0.1, 100.0, 1000, 1e-6, (ISCO, 20.0), 0, "PBWN"),
    "m24_rk4":        (2.4, 0.0, RK4, 0.1, 100.0, 1000, 1e-6, (ISCO, 40.0), 0, "PBWN"),
    "m24_rkf":        (2.4, 0.0, RKF45, 0.1, 200.0, 600, 1e-6, (ISCO, 40.0), 0, "BW"),
    "m05_kerr_rkf":   (0.5, 0.45, RKF45, 0.1, 100.0, 2000, 1e-8, None, 0, "BN"),
    "m24_kerr_rk4":   (2.4, 0.9, RK4, 0.1, 150.0, 1000, 1e-6, (ISCO, 40.0), D, "BWS"),
    "retro_rk4":      (1.0, -0.9, RK4, 0.1, 100.0, 1000, 1e-6, (ISCO, 20.0), D, "BPE"),
    "a05_rkf_disk":   (1.0, 0.5, RKF45, 0.1, 100.0, 1000, 1e-6, (ISCO, 20.0), D, "BN"),
    "a0998_rkf":      (1.0, 0.998, RKF45, 0.1, 100.0, 2000, 1e-8, None, 0, "BS"),
    "extremal_rk4":   (1.0, 1.0, RK4, 0.1, 100.0, 500, 1e-6, (1.0, 20.0), D, "B"),
    "dt003_rk4":      (1.0, 0.0, RK4, 0.03, 100.0, 1500, 1e-6, (ISCO, 20.0), 0, "BN"),
    "dt05_rk4":       (1.0, 0.0, RK4, 0.5, 100.0, 1000, 1e-6, (ISCO, 20.0), 0, "BW"),
    "dt7_rk4":        (1.0, 0.0, RK4, 7.0, 100.0, 1000, 1e-6, (ISCO, 20.0), 0, "BW"),
    "dt7_kerr_rkf":   (1.0, 0.9, RKF45, 7.0, 100.0, 1000, 1e-6, (ISCO, 20.0), D, "BW"),
    "dtneg_rk4":      (1.0, 0.0, RK4, -0.1, 100.0, 400, 1e-6, (ISCO, 20.0), 0, "BN"),
    "dtneg_kerr_rkf": (1.0, 0.9, RKF45, -0.1, 100.0, 400, 1e-6, (ISCO, 20.0), D, "B"),
    "dt0_rk4":        (1.0, 0.0, RK4, 0.0, 100.0, 60, 1e-6, (ISCO, 20.0), 0, "B"),
    "tol_hi_s":       (1.0, 0.0, RKF45, 0.1, 100.0, 1000, 1.0, (ISCO, 20.0), 0, "BN"),
    "tol_lo_s":       (1.0, 0.0, RKF45, 0.1, 100.0, 600, 1e-12, (ISCO, 20.0), 0, "BN"),
    "tol_2m30":       (1.0, 0.9, RKF45, 0.1, 100.0, 1000, 2.0**-30, (ISCO, 20.0), D, "B"),
    "tol_below":      (1.0, 0.9, RKF45, 0.1, 100.0, 1000, float(np.nextafter(2.0**-30, 0.0)),
                       (ISCO, 20.0), D, "B"),
    "tol_1e12_kerr":  (1.0, 0.9, RKF45, 0.1, 100.0, 1000, 1e-12, (ISCO, 20.0), D, "BN"),
    "tol_0_kerr":     (1.0, 0.9, RKF45, 0.1, 100.0, 300, 0.0, None, 0, "B"),
    "tol_nan_kerr":   (1.0, 0.9, RKF45, 0.1, 100.0, 300, NAN, None, 0, "B"),
    "tol_1e301":      (1.0, 0.9, RKF45, 0.1, 100.0, 1000, 1e301, None, 0, "B"),
    "dist_inf":       (1.0, 0.0, RK4, 0.1, INF, 800, 1e-6, None, 0, "B"),
    "dist_nan":       (1.0, 0.9, RK4, 0.1, NAN, 800, 1e-6, (ISCO, 20.0), D, "B"),
    "dist_35":        (1.0, 0.0, RK4, 0.1, 35.0, 1000, 1e-6, (ISCO, 20.0), 0, "BW"),
    "dist_0":         (1.0, 0.0, RKF45, 0.1, 0.0, 1000, 1e-6, (ISCO, 20.0), 0, "B"),
    "disk_swapped":   (1.0, 0.0, RK4, 0.1, 100.0, 1000, 1e-6, (20.0, 6.0), 0, "B"),
    "disk_all":       (1.0, 0.0, RK4, 0.1, 100.0, 1000, 1e-6, (0.0, INF), 0, "BE"),
    "disk_nan":       (1.0, 0.0, RKF45, 0.1, 100.0, 1000, 1e-6, (NAN, 20.0), 0, "B"),
    "disk_neg":       (1.0, 0.9, RK4, 0.1, 100.0, 1000, 1e-6, (-1.0, 3.0), D, "BN"),
    "disk_wide":      (1.0, 0.9, RK4, 0.1, 300.0, 1000, 1e-6, (0.0, 1e3), D, "BW"),
    "disk_thin_ring": (1.0, 0.0, RKF45, 0.1, 100.0, 1000, 1e-6, (9.0, 9.5), 0, "BP"),
    "inside_rk4":     (1.0, 0.0, RK4, 0.1, 100.0, 1000, 1e-6, (ISCO, 20.0), 0, "I"),
    "inside_kerr":    (1.0, 0.9, RKF45, 0.1, 100.0, 1000, 1e-6, (ISCO, 20.0), D, "I"),
    "steps_3":        (1.0, 0.9, RKF45, 0.1, 100.0, 3, 1e-6, (ISCO, 20.0), D, "BN"),
    "steps_17":       (1.0, 0.0, RK4, 0.1, 100.0, 17, 1e-6, (ISCO, 20.0), 0, "N"),
    "leapfrog":       (2.4, 0.5, LEAPFROG, 0.1, 100.0, 50, 1e-6, (ISCO, 40.0), D, "B"),
    "m1e3":           (1e-3, 0.0, RK4, 0.1, 100.0, 1000, 1e-6, (0.006, 20.0), 0, "BN"),
    "m40":            (40.0, 0.0, RKF45, 1.0, 2000.0, 500, 1e-6, (ISCO, 800.0), 0, "W"),
}

RAY_GROUP = 7  # scenes per tests/golden/sweep_rays_<k>.npz (each file below 230 KB)

FRAMES = [(name, cam) for name, row in SCENES.items() for cam in row[9]]

# scenes whose one frame (camera B; I for inside_kerr) is also stored from the compiled reference
FRAME_FIXTURES = ("m24_rk4", "m05_kerr_rkf", "retro_rk4", "dt7_kerr_rkf", "dtneg_rk4",
                  "tol_below", "disk_neg", "inside_kerr")


def fixture_camera(name):
    return "I" if name == "inside_kerr" else "B"


def camera(key):
    if key == "B":
        return configs.camera("B")
    pos, up, fov = CAMERAS[key]
    return abi.Camera(abi.v3(*pos), abi.v3(-pos[0], -pos[1], -pos[2]), abi.v3(*up), fov)


def scene(name):
    mass, spin, method, dt, max_dist, max_steps, tol, disk, flags, cams = SCENES[name]
    bh = abi.black_hole(mass, spin)
    dk = None
    if disk is not None:
        inner, outer = disk
        dk = abi.disk(bh.isco_radius if inner == ISCO else inner, outer, 1.0, 1.0)
    cfg = abi.sim_config(dt, max_dist, max_steps, tol)
    return bh, dk, cfg, method, flags, tuple(cams)
