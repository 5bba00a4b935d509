"""The path kernels on the scene sweep: what is shared by tests/golden/gen_sweep_paths.py, the
CPU tests (tests/test_paths_sweep_cpu.py) and the GPU tests (tests/test_gpu_paths_sweep.py).

The full paths of the 181 edge rays in the 41 sweep scenes are 3.87 M points (93 MB), so the
fixtures tests/golden/sweep_paths_<k>.npz hold a digest of every path of the compiled
reference's integrate_photon_path(origin with t = 0, direction, ..., max_positions =
max_steps + 1), keyed "<scene>.<field>":

    res [181, 4] int32    return value, count m, hit.result, hit.steps
    sum [181, 4] float64  the plain left-to-right double sums over the m points of x, of y, of z
                          and of (|x| + |y|) + |z|
    pts [46, 3, 3]        for the rays with index % 4 == 0 the points min(1, m - 1), m // 2, m - 1
"""
import ctypes as C
import functools
import glob
import os

import numpy as np

import sweep_scenes as sw
from conftest import GOLDEN, golden, rays_from
from bhrt import abi

PATH_GROUP = 14  # scenes per tests/golden/sweep_paths_<k>.npz (each file below 230 KB)
PTS_EVERY = 4    # the rays whose three points are stored

_ARGS = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
         C.c_void_p, C.c_void_p]


@functools.lru_cache(maxsize=None)
def edge_rays():
    rays = rays_from(golden("rays_rk4_disk"))
    assert len(rays) == 181
    return rays


def integrate(fn, ray, bh, cfg, method, cap, fill=0.0, room=0):
    """One call of an integrate_photon_path (the reference's, the oracle's or libbhrt's) with the
    origin at t = 0, max_positions = cap and a path buffer of cap + room points filled with
    `fill`: (the whole buffer [cap + room, 3], count, return value, hit)."""
    if fn.argtypes is None:  # (libbhrt's prototype is declared by bhrt.lib)
        fn.argtypes = _ARGS
        fn.restype = C.c_int
    buf = np.full((cap + room, 3), fill)
    num = C.c_int(0)
    hit = abi.RayTraceHit()
    o, d = ray["origin"], ray["direction"]
    res = fn(C.byref(abi.Vector4D(0.0, *[float(x) for x in o])),
             C.byref(abi.v3(*[float(x) for x in d])), C.byref(bh), C.byref(cfg), method,
             buf.ctypes.data, cap, C.byref(num), C.byref(hit))
    return buf, num.value, res, hit


def pts_indices(m):
    return [min(1, m - 1), m // 2, m - 1]


def digest(points):
    """(sum [4], pts [3, 3]) of one path [m, 3]. np.cumsum adds strictly left to right (np.sum
    adds pairwise, Python's sum compensates)."""
    p = np.ascontiguousarray(points, dtype=np.float64)
    a = np.abs(p)
    cols = np.column_stack([p, (a[:, 0] + a[:, 1]) + a[:, 2]])
    return np.cumsum(cols, axis=0)[-1], p[pts_indices(len(p))]


def scene_digest(fn, name):
    """The fixture's three arrays of one scene from the integrate_photon_path `fn`."""
    bh, _, cfg, method, _, _ = sw.scene(name)
    rays = edge_rays()
    cap = cfg.max_integration_steps + 1
    res = np.zeros((len(rays), 4), dtype=np.int32)
    sums = np.zeros((len(rays), 4))
    pts = np.zeros(((len(rays) + PTS_EVERY - 1) // PTS_EVERY, 3, 3))
    for i, ray in enumerate(rays):
        buf, m, r, hit = integrate(fn, ray, bh, cfg, method, cap)
        assert 1 <= m <= cap, (name, i, m)
        res[i] = (r, m, hit.result, hit.steps)
        sums[i], p = digest(buf[:m])
        if i % PTS_EVERY == 0:
            pts[i // PTS_EVERY] = p
    return {"res": res, "sum": sums, "pts": pts}


def fixture_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "sweep_paths_*.npz")))


@functools.lru_cache(maxsize=None)
def fixtures():
    out = {}
    for p in fixture_files():
        with np.load(p, allow_pickle=False) as z:
            for k in z.files:
                name, f = k.split(".")
                out.setdefault(name, {})[f] = z[k]
    return out


# ---- rays whose duplicate segment hits at segment 2 (k_paths' R.k - k_before == 2) ----
# In the sweep a stuck ray's duplicate segment is segment 1 (q_1 == q_0 bit for bit, 72 hits),
# which the kernel decides like any segment; a hit on the duplicate segment BEHIND the first
# stuck point needs q_1 != q_0 with an unchanged state, and between finite points only rounding
# gives that (a knife-edge ray). A non-finite origin does it robustly: q_0 is not finite, the
# first iteration repairs the state (raytracer.c:543-548: r, theta, phi = 1) and leaves it
# there (LEAPFROG is a no-op, RKF45 at a tolerance it cannot meet rejects for ever), segment 1
# has a non-finite "normal" and cannot hit, and segment 2 = (q_1, q_1) hits a disk that holds
# the point below q_1 along the direction. The mass is small so that r = 1 is outside the
# horizon. tests/golden/paths_repaired_origin.npz holds the compiled reference's outputs.
REPAIRED_SCENES = {  # name: (mass, spin, method, tol); dt 0.1, distance 100, 40 steps
    "leapfrog": (0.01, 0.0, sw.LEAPFROG, 1e-6),
    "rkf_tol_lo": (0.01, 0.0, sw.RKF45, 1e-12),
    "kerr_tol_0": (0.01, 0.5, sw.RKF45, 0.0),
}
REPAIRED_FIELDS = ("result", "steps", "hit_x", "hit_y", "hit_z", "distance", "time_dilation")


def repaired_scene(name):
    mass, spin, method, tol = REPAIRED_SCENES[name]
    return (abi.black_hole(mass, spin), abi.disk(0.0, 20.0, 1.0, 1.0),
            abi.sim_config(0.1, 100.0, 40, tol), method)


@functools.lru_cache(maxsize=None)
def repaired_rays():
    nan, inf = np.nan, np.inf
    origins = [(nan, 0, 30), (0, nan, 30), (0, 0, nan), (nan, nan, nan), (inf, 0, 0), (0, inf, 5),
               (1, 2, inf), (-inf, 3, 1)]
    dirs = [(-0.6, -0.6, -0.5), (0.3, -0.2, -1.0), (-1, 0.2, 0.3), (0.1, 0.05, -1), (-0.45, -0.7, -0.55),
            (0.5, 0.5, 0.5)]
    rays = np.zeros(len(origins) * len(dirs), dtype=abi.RAY_DTYPE)
    rays["origin"] = [o for o in origins for _ in dirs]
    rays["direction"] = [d for _ in origins for d in dirs]
    return rays


def full_paths(fn, rays, bh, cfg, method):
    """(path [n, max_steps + 1, 3] with NaN beyond the count, res [n, 4] int32) of `fn`."""
    cap = cfg.max_integration_steps + 1
    path = np.full((len(rays), cap, 3), np.nan)
    res = np.zeros((len(rays), 4), dtype=np.int32)
    for i, ray in enumerate(rays):
        buf, m, r, hit = integrate(fn, ray, bh, cfg, method, cap)
        path[i, :m] = buf[:m]
        res[i] = (r, m, hit.result, hit.steps)
    return path, res
