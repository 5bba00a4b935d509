"""The emission rule of include/bhrt_api.h ("Kerr disk emission") in numpy: kerr_rk45_rule's
attempts, controller, tests and Hermite crossing point, with up to K disk crossings recorded per
ray instead of the first ending it; the redshift factor of a crossing from the constants of the
motion, the emissivity, the intensity and the colour. Float64 throughout, in the header's order."""
import numpy as np

import kerr_rule as kr
import kerr_rk45_rule as k5
from kerr_rule import HORIZON, DISK, MAX_DISTANCE, MAX_STEPS, ERROR  # noqa: F401
from kerr_rk45_rule import A2, A3, A4, A5, A6, B5, EC, NEWTON, _rhs6, _stage, hermite

MAX_CROSSINGS = 4


def orbit(r, spin, mass):
    """(Omega, N) of the equatorial circular orbit at Boyer-Lindquist radius r: a = spin * mass is
    the physical spin, the disk turning about +z in +phi."""
    M = float(mass)
    a = float(spin) * M
    sm = np.sqrt(M)
    om = sm / (r * np.sqrt(r) + a * sm)
    t = 1.0 - a * om
    N = (1.0 - (2.0 * M / r) * (t * t)) - (om * om) * (r * r + a * a)
    return om, N


def redshift(r, E, lz, spin, mass):
    """g = sqrt(N) / (E + Omega L_z); 0 where N > 0 or E + Omega L_z > 0 fails or g is not
    finite."""
    with np.errstate(all="ignore"):
        om, N = orbit(np.asarray(r, dtype=np.float64), spin, mass)
        den = E + om * lz
        g = np.sqrt(N) / den
    return np.where((N > 0.0) & (den > 0.0) & np.isfinite(g), g, 0.0)


def emissivity(r, inner, q):
    return np.power(inner / r, q)


def trace(origins, dirs, spin, mass, disk, time_step, max_dist, max_steps, tol, K, q=0.0):
    """The rule for N rays (arguments as kerr_rk45_rule.trace, K = max_crossings, q the
    emissivity's index; disk = (inner, outer), not None). Returns kerr_rk45_rule.trace's fields
    and count [N], radius, redshift [K, N] (NaN beyond a ray's count), cross_xy [K, N, 2],
    intensity [N], E and lz [N]."""
    assert 1 <= K <= MAX_CROSSINGS and disk is not None
    o = np.array(origins, dtype=np.float64).reshape(-1, 3)
    n = kr.normalise(np.array(dirs, dtype=np.float64).reshape(-1, 3))
    N = len(o)
    M = float(mass)
    a = kr.spin_a(float(spin), M)
    rp = kr.r_plus(a, M)
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
    count = np.zeros(N, dtype=np.int32)
    radius = np.full((K, N), np.nan)
    red = np.full((K, N), np.nan)
    cross_xy = np.full((K, N, 2), np.nan)
    inten = np.zeros(N)
    with np.errstate(all="ignore"):
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
            k5_ = _rhs6(_stage(y, h, A5, (k1, k2, k3, k4)), e, a, M)
            k6 = _rhs6(_stage(y, h, A6, (k1, k2, k3, k4, k5_)), e, a, M)
            yn = _stage(y, h, B5, (k1, k2, k3, k4, k5_, k6))
            gn = kr.geometry(yn[0], yn[1], yn[2], a, M)
            k7 = _rhs6(yn, e, a, M, gn)
            ev = h * (((((EC[0] * k1 + EC[2] * k3) + EC[3] * k4) + EC[4] * k5_) + EC[5] * k6)
                      + EC[6] * k7)
            sc = tol * (1.0 + np.maximum(np.abs(y), np.abs(yn)))
            err = np.max(np.abs(ev) / sc, axis=0)
            fac = np.minimum(5.0, np.maximum(0.2, 0.9 * err ** -0.2))
            fac = np.where(np.isfinite(fac), fac, 0.2)
            steps[live] += 1
            res = np.full(live.size, -1, dtype=np.int32)
            fin = np.isfinite(yn).all(axis=0) & np.isfinite(err)     # 1.
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
            # 3. the disk: a crossing is recorded; the K-th ends the ray
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
            crossed = acc & cross & (d_lo <= s) & (s <= d_hi)
            ci = np.nonzero(crossed)[0]
            if ci.size:
                rays = live[ci]
                k = count[rays]
                r = np.sqrt(s[ci] - a * a)
                g = redshift(r, e[ci], lz0[rays], spin, M)
                radius[k, rays] = r
                red[k, rays] = g
                cross_xy[k, rays, 0], cross_xy[k, rays, 1] = qx[ci], qy[ci]
                g2 = g * g
                inten[rays] = inten[rays] + (g2 * g2) * emissivity(r, disk[0], q)
                count[rays] = k + 1
            hitd = crossed & (count[live] == K)
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
        dist[live] = nd
        move = acc | ~fin
        Y[:, live[move]] = yn[:, move]
        K1[:, live[acc]] = k7[:, acc]
        R[live[acc]] = gn["r"][acc]
        hit[live[move]] = np.stack([hx, hy, hz], axis=1)[move]
        tang[live[acc]] = np.stack([tx, ty, tz], axis=1)[acc]
        result[live] = res
        live = live[res < 0]
    return dict(result=result, steps=steps, rejected=rejected, hit=hit, distance=dist, chord=tang,
                n=n, b=lz0 / E, count=count, radius=radius, redshift=red, cross_xy=cross_xy,
                intensity=inten, E=E, lz=lz0)


def disk_base(rxy, disk):
    """The frame colour contract's disk colour without the Doppler block at cylindrical radius
    rxy (kerr_rule.colour's disk branch): [.., 3]."""
    nr = np.clip((rxy - disk.inner_radius) / (disk.outer_radius - disk.inner_radius), 0, 1)
    su = np.sqrt(1.0 - nr)
    T = np.clip(disk.temperature_scale * (2000.0 + 18000.0 * (su * np.sqrt(su))), 1000.0, 40000.0)
    tt = (T - 1000.0) / (40000.0 - 1000.0)
    r = np.where(tt < 0.5, tt * 2.0, 1.0)
    g = np.where(tt < 0.25, 0.0, np.where(tt < 0.75, (tt - 0.25) * 2.0, 1.0))
    b = np.where(tt < 0.5, 0.0, (tt - 0.5) * 2.0)
    br = 0.2 + 0.8 * (tt * tt)
    return np.stack([r * br, g * br, b * br], axis=-1)


def emission_colour(count, radius, redshift_, a2, disk, q, gain):
    """clamp(gain sum_k w_k base_k, 0, 1) from recorded crossings (radius, redshift [K, N]; base_k
    at rxy = sqrt(radius^2 + a^2)): [N, 3]; rows of rays without crossings are 0."""
    K, N = radius.shape
    rgb = np.zeros((N, 3))
    with np.errstate(all="ignore"):
        for k in range(K):
            m = count > k
            r, g = radius[k, m], redshift_[k, m]
            g2 = g * g
            w = (g2 * g2) * emissivity(r, disk.inner_radius, q)
            rgb[m] = rgb[m] + w[:, None] * disk_base(np.sqrt(r * r + a2), disk)
    return np.clip(gain * rgb, 0.0, 1.0)


def colour(tr, bh, disk, q, gain):
    """The rule's colour of a traced set (no sky map): the adaptive rule's for count 0, the
    emission's otherwise."""
    rgb = kr.colour(tr, bh, disk, 0)
    a = bh.spin * bh.mass
    em = emission_colour(tr["count"], tr["radius"], tr["redshift"], a * a, disk, q, gain)
    has = tr["count"] > 0
    rgb[has] = em[has]
    return rgb


# ---- the scenes of the tests ----
TOL = 1e-8
KNIFE_EPS = k5.KNIFE_EPS
Q, GAIN = 3.0, 1.0
_cache = {}


def frame_rule(spin, disk, width, height, K, eps=0.0, tol=TOL, q=Q):
    """The emission rule's frame (traced once per session); eps as kerr_rule.frame_rule's."""
    key = (spin, disk, width, height, K, eps, tol, q)
    if key not in _cache:
        cam = kr.camera()
        d = kr.camera_dirs(cam, width, height)
        if eps:
            e = kr.normalise(np.random.default_rng(7).normal(size=d.shape))
            d = d + eps * e
        o = np.tile([cam.position.x, cam.position.y, cam.position.z], (len(d), 1))
        tr = trace(o, d, spin, kr.MASS, disk, kr.SCENE_DT, kr.SCENE_DIST, kr.SCENE_STEPS, tol, K, q)
        tr["dirs"] = d
        _cache[key] = tr
    return _cache[key]


def _differs(p, base):
    return ((p["result"] != base["result"]) | (p["steps"] != base["steps"]) |
            (p["rejected"] != base["rejected"]) | (p["count"] != base["count"]))


def knife_edge(spin, disk, width, height, K, eps=KNIFE_EPS):
    """kerr_rk45_rule.knife_edge extended with count: rays whose class, attempts, rejected or
    count changes under a +-eps direction perturbation."""
    base = frame_rule(spin, disk, width, height, K)
    bad = np.zeros(len(base["result"]), dtype=bool)
    for s in (eps, -eps):
        bad |= _differs(frame_rule(spin, disk, width, height, K, s), base)
    return bad


# the fan of the higher-order test: 64 rays from (0, -30, 3) that graze the photon orbit of a
# spin-0.9 hole, spread in impact parameter across the band where 1 to 4 crossings occur
FAN_ORIGIN = (0.0, -30.0, 3.0)
FAN_SPIN, FAN_DISK = 0.9, (2.4, 12.0)
FAN_DT, FAN_DIST, FAN_STEPS = 0.25, 100.0, 4000
FAN_B = (4.721176, 4.761176)
FAN_RAYS = 64
FAN_EPS = 1e-9


def fan_dirs(eps=0.0):
    o = np.array(FAN_ORIGIN)
    axis = kr.normalise(np.array([0.0, 30.0, -3.0]))
    side = kr.normalise(np.array([0.0, 3.0, 30.0]))
    b = np.linspace(FAN_B[0], FAN_B[1], FAN_RAYS)
    d = axis[None, :] + (b / np.sqrt((o * o).sum()))[:, None] * side[None, :]
    if eps:
        d = d + eps * kr.normalise(np.random.default_rng(7).normal(size=d.shape))
    return d


def fan_scene():
    bh, dk, cfg = k5.scene(FAN_SPIN, FAN_DISK, TOL)
    cfg.time_step, cfg.max_ray_distance, cfg.max_integration_steps = FAN_DT, FAN_DIST, FAN_STEPS
    return bh, dk, cfg


def fan_trace(K=MAX_CROSSINGS, eps=0.0, q=Q):
    key = ("fan", K, eps, q)
    if key not in _cache:
        d = fan_dirs(eps)
        o = np.tile(FAN_ORIGIN, (len(d), 1))
        tr = trace(o, d, FAN_SPIN, kr.MASS, FAN_DISK, FAN_DT, FAN_DIST, FAN_STEPS, TOL, K, q)
        tr["dirs"] = d
        _cache[key] = tr
    return _cache[key]


def fan_knife_edge(K=MAX_CROSSINGS, eps=FAN_EPS):
    base = fan_trace(K)
    bad = np.zeros(len(base["result"]), dtype=bool)
    for s in (eps, -eps):
        bad |= _differs(fan_trace(K, s), base)
    return bad
