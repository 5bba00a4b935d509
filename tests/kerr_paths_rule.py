"""The rule of include/bhrt_api.h "Physical photon paths" in numpy: the full path of every ray --
kerr_rule.py's trace (geometry, initial data, right-hand side, the five tests after a step, one
operation per rounding) with the kept position of every step recorded -- and which of its points
are stored for a given `every` and `max_positions`."""
import numpy as np

import kerr_rule as kr

_cache = {}


def full_paths(origins, dirs, spin, mass, disk, time_step, max_dist, max_steps):
    """The rule for N rays: result, steps, hit [N, 3], distance as kerr_rule.trace forms them, b =
    L_z / E, and `paths`, a list of N arrays [steps + 1, 3]: q_0 the origin as given, q_k the
    position the rule keeps after step k (the hit point for the step that hits the disk)."""
    o = np.array(origins, dtype=np.float64).reshape(-1, 3)
    n = kr.normalise(np.array(dirs, dtype=np.float64).reshape(-1, 3))
    N = len(o)
    M = float(mass)
    a = kr.spin_a(float(spin), M)
    rp = kr.r_plus(a, M)
    if disk is not None:
        d_lo, d_hi = disk[0] * disk[0] + a * a, disk[1] * disk[1] + a * a
    p0, E, ok = kr.initial_data(o, n, a, M)
    X = o.copy()
    P = p0.copy()
    result = np.full(N, -1, dtype=np.int32)
    steps = np.zeros(N, dtype=np.int32)
    dist = np.zeros(N)
    hit = o.copy()
    result[~ok] = kr.ERROR
    if max_steps <= 0:
        result[ok] = kr.MAX_STEPS
    lz0 = X[:, 0] * P[:, 1] - X[:, 1] * P[:, 0]
    record = []   # per step: (the rays that took it, their kept positions)
    live = np.nonzero(result < 0)[0]
    while live.size:
        x, y, z = X[live, 0], X[live, 1], X[live, 2]
        px, py, pz = P[live, 0], P[live, 1], P[live, 2]
        e = E[live]
        with np.errstate(all="ignore"):
            g = kr.geometry(x, y, z, a, M)
            h = time_step * np.minimum(1.0, np.maximum(g["r"] / (8.0 * M), 1.0 / 16.0))
            k1x, k1p = kr.rhs(x, y, z, px, py, pz, e, a, M, g)
            hh = 0.5 * h
            k2x, k2p = kr.rhs(x + hh * k1x[0], y + hh * k1x[1], z + hh * k1x[2],
                              px + hh * k1p[0], py + hh * k1p[1], pz + hh * k1p[2], e, a, M)
            k3x, k3p = kr.rhs(x + hh * k2x[0], y + hh * k2x[1], z + hh * k2x[2],
                              px + hh * k2p[0], py + hh * k2p[1], pz + hh * k2p[2], e, a, M)
            k4x, k4p = kr.rhs(x + h * k3x[0], y + h * k3x[1], z + h * k3x[2],
                              px + h * k3p[0], py + h * k3p[1], pz + h * k3p[2], e, a, M)
            h6 = h / 6.0
            nx, ny, nz = (c + h6 * ((k1x[i] + 2.0 * k2x[i]) + (2.0 * k3x[i] + k4x[i]))
                          for i, c in enumerate((x, y, z)))
            npx, npy, npz = (c + h6 * ((k1p[i] + 2.0 * k2p[i]) + (2.0 * k3p[i] + k4p[i]))
                             for i, c in enumerate((px, py, pz)))
            steps[live] += 1
            cx, cy, cz = nx - x, ny - y, nz - z
            seg = np.sqrt((cx * cx + cy * cy) + cz * cz)
            res = np.full(live.size, -1, dtype=np.int32)
            fin = np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz) & np.isfinite(npx) & \
                np.isfinite(npy) & np.isfinite(npz)
            res[~fin] = kr.ERROR                                   # 1. a non-finite state
            hx, hy, hz = nx.copy(), ny.copy(), nz.copy()
            dadd = seg.copy()
            gn = kr.geometry(nx, ny, nz, a, M)
            if disk is not None:                                   # 2. the disk
                cross = ((z > 0.0) & (nz <= 0.0)) | ((z < 0.0) & (nz >= 0.0))
                t = z / (z - nz)
                qx, qy = x + t * cx, y + t * cy
                s = qx * qx + qy * qy
                hitd = (res < 0) & cross & (d_lo <= s) & (s <= d_hi)
                res[hitd] = kr.DISK
                hx[hitd], hy[hitd], hz[hitd] = qx[hitd], qy[hitd], 0.0
                dadd[hitd] = (t * seg)[hitd]
            hor = (res < 0) & (gn["r"] <= rp)                      # 3. the horizon
            res[hor] = kr.HORIZON
            dadd[hor] = 0.0
            dadd[~fin] = 0.0
            nd = dist[live] + dadd                                 # 4. the distance
            res[(res < 0) & (nd > max_dist)] = kr.MAX_DISTANCE
            res[(res < 0) & (steps[live] >= max_steps)] = kr.MAX_STEPS   # 5. the steps
        dist[live] = nd
        X[live] = np.stack([nx, ny, nz], axis=1)
        P[live] = np.stack([npx, npy, npz], axis=1)
        kept = np.stack([hx, hy, hz], axis=1)
        hit[live] = kept
        record.append((live, kept))
        result[live] = res
        live = live[res < 0]
    buf = np.empty((N, len(record) + 1, 3))
    buf[:, 0] = o
    for k, (rays, kept) in enumerate(record):
        buf[rays, k + 1] = kept
    return dict(result=result, steps=steps, hit=hit, distance=dist, b=lz0 / E,
                paths=[buf[i, :steps[i] + 1] for i in range(N)])


def stored_points(path, every, max_positions):
    """The stored points of a full path [m, 3]: q_0, q_e, q_2e, ..., then q_{m-1} where
    (m - 1) % e != 0; of that list the first max_positions."""
    m = len(path)
    idx = list(range(0, m, every))
    if (m - 1) % every != 0:
        idx.append(m - 1)
    return path[idx[:max_positions]]


def stored_count(m, every, max_positions):
    """count[i] of a path of m points, in closed form."""
    kept = (m - 1) // every + 1 + (1 if (m - 1) % every else 0)
    return min(kept, max_positions)


# ---- the two ray sets of the tests (tests/test_kerr_paths_cpu.py, tests/test_gpu_kerr_paths.py) ----
SET_A_SIZE = (49, 27)


def set_a_rays(width=SET_A_SIZE[0], height=SET_A_SIZE[1], eps=0.0):
    """(origins, dirs) of the camera frame of kerr_rule's scenes; eps as kerr_rule.frame_rule."""
    cam = kr.camera()
    d = kr.camera_dirs(cam, width, height)
    if eps:
        d = d + eps * kr.normalise(np.random.default_rng(7).normal(size=d.shape))
    o = np.tile([cam.position.x, cam.position.y, cam.position.z], (len(d), 1))
    return o, d


def set_b_rays(eps=0.0):
    """(origins, dirs) of the two equatorial fans from kerr_rule.FAN_ORIGIN: 128 rays."""
    d = np.concatenate([kr.fan(+1), kr.fan(-1)])
    if eps:
        d = d + eps * kr.normalise(np.random.default_rng(7).normal(size=d.shape))
    return np.tile(kr.FAN_ORIGIN, (len(d), 1)), d


def rule(which, spin, disk, max_steps=kr.SCENE_STEPS, eps=0.0, size=SET_A_SIZE):
    """full_paths of set "A" (with the scene's disk) or "B" (disk None), traced once per session
    and left unchanged by its readers."""
    key = (which, spin, disk, max_steps, eps, size)
    if key not in _cache:
        o, d = set_a_rays(*size, eps=eps) if which == "A" else set_b_rays(eps)
        tr = full_paths(o, d, spin, kr.MASS, disk, kr.SCENE_DT, kr.SCENE_DIST, max_steps)
        tr["origins"], tr["dirs"] = o, d
        _cache[key] = tr
    return _cache[key]


def knife_edge(which, spin, disk, max_steps=kr.SCENE_STEPS, eps=1e-9, size=SET_A_SIZE):
    """Rays whose class or step count changes under a +-eps direction perturbation."""
    base = rule(which, spin, disk, max_steps, size=size)
    bad = np.zeros(len(base["result"]), dtype=bool)
    for s in (eps, -eps):
        p = rule(which, spin, disk, max_steps, eps=s, size=size)
        bad |= (p["result"] != base["result"]) | (p["steps"] != base["steps"])
    return bad
