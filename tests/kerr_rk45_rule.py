"""The adaptive Kerr-Schild null-ray rule of include/bhrt_api.h ("Physical geodesics, adaptive
steps") in numpy: Dormand-Prince 5(4) attempts with FSAL on kerr_rule's geometry, right-hand side
and initial data, the trial step, the error norm, the controller, the order of the tests after an
attempt, the Hermite disk point and the exit tangent. Float64 throughout, in the header's order;
rays are traced side by side in arrays, each with its own step."""
import numpy as np

import kerr_rule as kr
from kerr_rule import HORIZON, DISK, MAX_DISTANCE, MAX_STEPS, ERROR  # noqa: F401

# the standard Dormand-Prince tableau: rows of a (stage 7's row is the 5th-order weights), and
# e_j = b5_j - b4_j
A2 = (1.0 / 5.0,)
A3 = (3.0 / 40.0, 9.0 / 40.0)
A4 = (44.0 / 45.0, -56.0 / 15.0, 32.0 / 9.0)
A5 = (19372.0 / 6561.0, -25360.0 / 2187.0, 64448.0 / 6561.0, -212.0 / 729.0)
A6 = (9017.0 / 3168.0, -355.0 / 33.0, 46732.0 / 5247.0, 49.0 / 176.0, -5103.0 / 18656.0)
B5 = (35.0 / 384.0, 0.0, 500.0 / 1113.0, 125.0 / 192.0, -2187.0 / 6784.0, 11.0 / 84.0)
EC = (71.0 / 57600.0, 0.0, -71.0 / 16695.0, 71.0 / 1920.0, -17253.0 / 339200.0, 22.0 / 525.0,
      -1.0 / 40.0)
TOL_MIN, TOL_MAX = 1e-12, 1e-2
NEWTON = 4


def _rhs6(Y, E, a, M, g=None):
    """kerr_rule.rhs on a state [6, n]: the derivative [6, n]."""
    xd, pd = kr.rhs(Y[0], Y[1], Y[2], Y[3], Y[4], Y[5], E, a, M, g)
    return np.stack([xd[0], xd[1], xd[2], pd[0], pd[1], pd[2]])


def _stage(Y, h, row, ks):
    """y + h (a_1 k_1 + a_2 k_2 + ...), summed left to right over the non-zero weights."""
    s = None
    for w, k in zip(row, ks):
        if w == 0.0:
            continue
        s = w * k if s is None else s + w * k
    return Y + h * s


def hermite(q0, q1, m0, m1):
    """The cubic through q0, q1 with end derivatives m0, m1 (per unit theta):
    q0 + theta (m0 + theta (c2 + theta c3)); returns (c2, c3)."""
    d = q1 - q0
    return (3.0 * d - 2.0 * m0) - m1, (m0 + m1) - 2.0 * d


def trace(origins, dirs, spin, mass, disk, time_step, max_dist, max_steps, tol, diag=False):
    """The rule for N rays (arguments as kerr_rule.trace, and the tolerance). Returns result,
    steps (attempts), rejected, hit [N, 3], distance, chord [N, 3] (the rule's TANGENT: the exit
    tangent where result is MAX_DISTANCE, the Hermite derivative at the crossing where it is
    DISK -- under kerr_rule's key, so that kerr_rule.colour and sky_rule read it), n, b, and with
    diag h_residual and lz_drift."""
    o = np.array(origins, dtype=np.float64).reshape(-1, 3)
    n = kr.normalise(np.array(dirs, dtype=np.float64).reshape(-1, 3))
    N = len(o)
    M = float(mass)
    a = kr.spin_a(float(spin), M)
    rp = kr.r_plus(a, M)
    if disk is not None:
        d_lo, d_hi = disk[0] * disk[0] + a * a, disk[1] * disk[1] + a * a
    p0, E, ok = kr.initial_data(o, n, a, M)
    Y = np.concatenate([o.T, p0.T])          # [6, N]
    result = np.full(N, -1, dtype=np.int32)
    steps = np.zeros(N, dtype=np.int32)
    rejected = np.zeros(N, dtype=np.int32)
    dist = np.zeros(N)
    hit = o.copy()
    tang = np.zeros((N, 3))
    H = np.full(N, float(time_step))
    result[~ok] = ERROR
    if max_steps <= 0:
        result[ok] = MAX_STEPS
    lz0 = Y[0] * Y[4] - Y[1] * Y[3]
    lzd = np.zeros(N)
    with np.errstate(all="ignore"):
        num, den = kr.hamiltonian_parts(*Y, E, a, M)
        hres = np.where(ok, np.abs(num / den), 0.0)
        K1 = _rhs6(Y, E, a, M)
        R = kr.geometry(Y[0], Y[1], Y[2], a, M)["r"]
    live = np.nonzero(result < 0)[0]
    while live.size:
        y, e, k1 = Y[:, live], E[live], K1[:, live]
        with np.errstate(all="ignore"):
            h = np.minimum(H[live], R[live] / 2.0)
            k2 = _rhs6(_stage(y, h, A2, (k1,)), e, a, M)
            k3 = _rhs6(_stage(y, h, A3, (k1, k2)), e, a, M)
            k4 = _rhs6(_stage(y, h, A4, (k1, k2, k3)), e, a, M)
            k5 = _rhs6(_stage(y, h, A5, (k1, k2, k3, k4)), e, a, M)
            k6 = _rhs6(_stage(y, h, A6, (k1, k2, k3, k4, k5)), e, a, M)
            yn = _stage(y, h, B5, (k1, k2, k3, k4, k5, k6))
            gn = kr.geometry(yn[0], yn[1], yn[2], a, M)
            k7 = _rhs6(yn, e, a, M, gn)
            ev = h * (((((EC[0] * k1 + EC[2] * k3) + EC[3] * k4) + EC[4] * k5) + EC[5] * k6)
                      + EC[6] * k7)
            sc = tol * (1.0 + np.maximum(np.abs(y), np.abs(yn)))
            err = np.max(np.abs(ev) / sc, axis=0)
            fac = np.minimum(5.0, np.maximum(0.2, 0.9 * err ** -0.2))
            fac = np.where(np.isfinite(fac), fac, 0.2)
            steps[live] += 1
            res = np.full(live.size, -1, dtype=np.int32)
            # 1. a non-finite point or error
            fin = np.isfinite(yn).all(axis=0) & np.isfinite(err)
            res[~fin] = ERROR
            acc = fin & (err <= 1.0)
            rej = fin & ~acc
            rejected[live[rej]] += 1
            H[live] = h * fac
            cx, cy, cz = yn[0] - y[0], yn[1] - y[1], yn[2] - y[2]
            seg = np.sqrt((cx * cx + cy * cy) + cz * cz)
            hx, hy, hz = yn[0].copy(), yn[1].copy(), yn[2].copy()
            tx, ty, tz = k7[0].copy(), k7[1].copy(), k7[2].copy()
            dadd = seg.copy()
            # 3. the disk, on the Hermite polynomial of the accepted step
            if disk is not None:
                z0, z1 = y[2], yn[2]
                cross = ((z0 > 0.0) & (z1 <= 0.0)) | ((z0 < 0.0) & (z1 >= 0.0))
                m0, m1 = h[None, :] * k1[:3], h[None, :] * k7[:3]
                c2, c3 = hermite(y[:3], yn[:3], m0, m1)
                th = z0 / (z0 - z1)
                for _ in range(NEWTON):
                    pz = z0 + th * (m0[2] + th * (c2[2] + th * c3[2]))
                    dz = m0[2] + th * (2.0 * c2[2] + th * (3.0 * c3[2]))
                    tn = th - pz / dz
                    th = np.where(np.isfinite(tn), np.minimum(1.0, np.maximum(0.0, tn)), th)
                qx = y[0] + th * (m0[0] + th * (c2[0] + th * c3[0]))
                qy = y[1] + th * (m0[1] + th * (c2[1] + th * c3[1]))
                s = qx * qx + qy * qy
                hitd = acc & cross & (d_lo <= s) & (s <= d_hi)
                res[hitd] = DISK
                hx[hitd], hy[hitd], hz[hitd] = qx[hitd], qy[hitd], 0.0
                dadd[hitd] = (th * seg)[hitd]
                for c, t in enumerate((tx, ty, tz)):
                    t[hitd] = (m0[c] + th * (2.0 * c2[c] + th * (3.0 * c3[c])))[hitd]
            # 4. the horizon
            hor = acc & (res < 0) & (gn["r"] <= rp)
            res[hor] = HORIZON
            dadd[hor] = 0.0
            dadd[~acc] = 0.0
            # 5. the distance
            nd = dist[live] + dadd
            res[acc & (res < 0) & (nd > max_dist)] = MAX_DISTANCE
            # 6. the attempts (after a rejection too)
            res[(res < 0) & (steps[live] >= max_steps)] = MAX_STEPS
            if diag:
                num, den = kr.hamiltonian_parts(*yn, e, a, M, gn)
                hres[live] = np.where(acc, np.maximum(hres[live], np.abs(num / den)), hres[live])
                lzd[live] = np.where(acc, np.abs((yn[0] * yn[4] - yn[1] * yn[3]) - lz0[live]),
                                     lzd[live])
        dist[live] = nd
        move = acc | ~fin                 # a rejected attempt leaves the ray where it was
        Y[:, live[move]] = yn[:, move]
        K1[:, live[acc]] = k7[:, acc]
        R[live[acc]] = gn["r"][acc]
        hit[live[move]] = np.stack([hx, hy, hz], axis=1)[move]
        tang[live[acc]] = np.stack([tx, ty, tz], axis=1)[acc]
        result[live] = res
        live = live[res < 0]
    out = dict(result=result, steps=steps, rejected=rejected, hit=hit, distance=dist, chord=tang,
               n=n, b=lz0 / E)
    if diag:
        out["h_residual"] = hres
        out["lz_drift"] = lzd
    return out


# ---- the scenes of the tests: kerr_rule's, at the tolerances below ----
TOLS = (1e-6, 1e-8)
REF_TOL, REF_STEPS = 1e-13, 40000
KNIFE_EPS = 1e-7
_cache = {}


def scene(spin, disk, tol):
    """(bh, disk, cfg) of a test scene: kerr_rule.scene with the tolerance set."""
    bh, dk, cfg = kr.scene(spin, disk)
    cfg.tolerance = tol
    return bh, dk, cfg


def frame_rule(spin, disk, width, height, tol, eps=0.0, max_steps=kr.SCENE_STEPS):
    """The adaptive rule's frame (traced once per session); eps as kerr_rule.frame_rule's."""
    key = (spin, disk, width, height, tol, eps, max_steps)
    if key not in _cache:
        cam = kr.camera()
        d = kr.camera_dirs(cam, width, height)
        if eps:
            e = kr.normalise(np.random.default_rng(7).normal(size=d.shape))
            d = d + eps * e
        o = np.tile([cam.position.x, cam.position.y, cam.position.z], (len(d), 1))
        tr = trace(o, d, spin, kr.MASS, disk, kr.SCENE_DT, kr.SCENE_DIST, max_steps, tol, diag=True)
        tr["dirs"] = d
        _cache[key] = tr
    return _cache[key]


def knife_edge(spin, disk, width, height, tol, eps=KNIFE_EPS):
    """Rays whose class, attempts or rejected count changes under a +-eps direction perturbation."""
    base = frame_rule(spin, disk, width, height, tol)
    bad = np.zeros(len(base["result"]), dtype=bool)
    for s in (eps, -eps):
        p = frame_rule(spin, disk, width, height, tol, s)
        bad |= ((p["result"] != base["result"]) | (p["steps"] != base["steps"]) |
                (p["rejected"] != base["rejected"]))
    return bad


def fan_trace(spin, side, tol):
    """kerr_rule.fan from FAN_ORIGIN through the adaptive rule, without a disk."""
    d = kr.fan(side)
    o = np.tile(kr.FAN_ORIGIN, (len(d), 1))
    return trace(o, d, spin, kr.MASS, None, kr.SCENE_DT, kr.SCENE_DIST, kr.SCENE_STEPS, tol)
