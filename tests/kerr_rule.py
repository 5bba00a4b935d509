"""The Kerr-Schild null-ray rule of include/bhrt_api.h ("Physical geodesics") in numpy: geometry,
initial data, the right-hand side, the step size, the RK4 step, the order of the tests after a
step, the diagnostics, the camera's rays and the colour. Float64 throughout, one operation per
rounding, in the header's order; rays are traced side by side in arrays."""
import math

import numpy as np

from bhrt import abi

HORIZON, DISK, MAX_DISTANCE, MAX_STEPS, ERROR = (abi.RAY_HORIZON, abi.RAY_DISK,
                                                 abi.RAY_MAX_DISTANCE, abi.RAY_MAX_STEPS,
                                                 abi.RAY_ERROR)


def spin_a(spin, mass):
    """The integration's spin parameter: a~ = -(spin * mass) (time reversal)."""
    return -(spin * mass)


def r_plus(a, M):
    return M + math.sqrt(M * M - a * a)


def geometry(x, y, z, a, M):
    """r, f, l, and the sums the gradients reuse, at points (x, y, z)."""
    a2 = a * a
    rho2 = (x * x + y * y) + z * z
    w = rho2 - a2
    D = np.sqrt(w * w + 4.0 * a2 * (z * z))
    r2 = (w + D) / 2.0
    r = np.sqrt(r2)
    G = r2 * r2 + a2 * (z * z)
    S = r2 + a2
    f = 2.0 * M * (r * r2) / G
    lx = (r * x + a * y) / S
    ly = (r * y - a * x) / S
    lz = z / r
    return dict(r=r, r2=r2, D=D, G=G, S=S, f=f, lx=lx, ly=ly, lz=lz)


def rhs(x, y, z, px, py, pz, E, a, M, g=None):
    """(xdot, pdot) of H = 1/2 [-E^2 + p.p - f u^2], u = E + l.p, with the analytic gradients."""
    if g is None:
        g = geometry(x, y, z, a, M)
    r, r2, D, G, S, f = g["r"], g["r2"], g["D"], g["G"], g["S"], g["f"]
    lx, ly, lz = g["lx"], g["ly"], g["lz"]
    a2 = a * a
    u = E + ((lx * px + ly * py) + lz * pz)
    fu = f * u
    xd = (px - fu * lx, py - fu * ly, pz - fu * lz)
    drx, dry, drz = x * r / D, y * r / D, z * S / (r * D)
    r3 = r * r2
    dfx = f * (3.0 * drx / r - (4.0 * r3 * drx) / G)
    dfy = f * (3.0 * dry / r - (4.0 * r3 * dry) / G)
    dfz = f * (3.0 * drz / r - (4.0 * r3 * drz + 2.0 * a2 * z) / G)
    two_r = 2.0 * r
    # d_i l_x, d_i l_y, d_i l_z for i = x, y, z
    dlx = ((x * drx + r) / S - lx * two_r * drx / S,
           (x * dry + a) / S - lx * two_r * dry / S,
           (x * drz) / S - lx * two_r * drz / S)
    dly = ((y * drx - a) / S - ly * two_r * drx / S,
           (y * dry + r) / S - ly * two_r * dry / S,
           (y * drz) / S - ly * two_r * drz / S)
    dlz = (-z * drx / r2, -z * dry / r2, 1.0 / r - z * drz / r2)
    hu2 = 0.5 * (u * u)
    pd = tuple(df * hu2 + fu * ((dlx[i] * px + dly[i] * py) + dlz[i] * pz)
               for i, df in enumerate((dfx, dfy, dfz)))
    return xd, pd


def initial_data(origin, n, a, M):
    """The static observer's photon of local energy 1 along unit n at `origin`: (p [.., 3], E,
    ok). ok is False where no static observer exists (f >= 1 or r <= r+)."""
    o = np.asarray(origin, dtype=np.float64)
    n = np.asarray(n, dtype=np.float64)
    with np.errstate(all="ignore"):
        g = geometry(o[..., 0], o[..., 1], o[..., 2], a, M)
        f = g["f"]
        ok = (f < 1.0) & (g["r"] > r_plus(a, M))
        kappa = np.sqrt(1.0 - f)
        l = np.stack([g["lx"], g["ly"], g["lz"]], axis=-1)
        ln = (l[..., 0] * n[..., 0] + l[..., 1] * n[..., 1]) + l[..., 2] * n[..., 2]
        v = n + ((kappa - 1.0) * ln)[..., None] * l
        lv = (l[..., 0] * v[..., 0] + l[..., 1] * v[..., 1]) + l[..., 2] * v[..., 2]
        kt = 1.0 / kappa + f * lv / (1.0 - f)
        p = v + (f * (kt + lv))[..., None] * l
    return p, kappa, ok


def hamiltonian_parts(x, y, z, px, py, pz, E, a, M, g=None):
    """(-E^2 + p.p - f u^2, E^2 + p.p + f u^2): H's numerator and the diag's denominator."""
    if g is None:
        g = geometry(x, y, z, a, M)
    u = E + ((g["lx"] * px + g["ly"] * py) + g["lz"] * pz)
    pp = (px * px + py * py) + pz * pz
    fu2 = g["f"] * (u * u)
    return (pp - E * E) - fu2, (E * E + pp) + fu2


def normalise(d):
    d = np.asarray(d, dtype=np.float64)
    L = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return d / L[..., None]


def camera_dirs(cam, width, height, rows=None):
    """The directions of (a shard of) a camera frame, row 0 = top, as the kernel forms them: the
    basis of calculate_ray_direction, then per pixel one operation per rounding."""
    def vnorm(v):
        l = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        return [c * (1.0 / l) for c in v]

    def cross(p, q):
        return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]

    fwd = vnorm([cam.direction.x, cam.direction.y, cam.direction.z])
    right = vnorm(cross(fwd, [cam.up.x, cam.up.y, cam.up.z]))
    up = cross(right, fwd)
    plane_h = 2.0 * math.tan(cam.fov_deg * math.pi / 180.0 / 2.0)
    plane_w = plane_h * (float(width) / float(height))
    ox, oy = (cam.offset_x, cam.offset_y) if cam.use_offset else (0.5, 0.5)
    ys = np.arange(height)
    if rows is not None and rows.num_shards > 1:
        ys = ys[(ys // rows.row_block) % rows.num_shards == rows.shard]
    ndcx = (2.0 * ((np.arange(width) + ox) / width) - 1.0) * plane_w
    ndcy = (1.0 - 2.0 * ((ys + oy) / height)) * plane_h
    v = np.empty((len(ys), width, 3))
    for k in range(3):
        v[:, :, k] = (fwd[k] + right[k] * ndcx[None, :]) + up[k] * ndcy[:, None]
    return normalise(v.reshape(-1, 3))


def trace(origins, dirs, spin, mass, disk, time_step, max_dist, max_steps, diag=False):
    """The rule for N rays. origins, dirs [N, 3] (dirs need not be unit: the rule normalises);
    disk None or (inner, outer). Returns result, steps, hit [N, 3], distance, chord [N, 3] (the
    last segment; the exit chord where result is MAX_DISTANCE), n [N, 3], b = L_z / E, and with
    diag h_residual and lz_drift."""
    o = np.array(origins, dtype=np.float64).reshape(-1, 3)
    n = normalise(np.array(dirs, dtype=np.float64).reshape(-1, 3))
    N = len(o)
    M = float(mass)
    a = spin_a(float(spin), M)
    rp = r_plus(a, M)
    if disk is not None:
        d_lo, d_hi = disk[0] * disk[0] + a * a, disk[1] * disk[1] + a * a
    p0, E, ok = initial_data(o, n, a, M)
    X = o.copy()
    P = p0.copy()
    result = np.full(N, -1, dtype=np.int32)
    steps = np.zeros(N, dtype=np.int32)
    dist = np.zeros(N)
    hit = o.copy()
    chord = np.zeros((N, 3))
    result[~ok] = ERROR
    if max_steps <= 0:
        result[ok] = MAX_STEPS
    lz0 = X[:, 0] * P[:, 1] - X[:, 1] * P[:, 0]
    hres = np.zeros(N)
    lzd = np.zeros(N)
    with np.errstate(all="ignore"):
        num, den = hamiltonian_parts(X[:, 0], X[:, 1], X[:, 2], P[:, 0], P[:, 1], P[:, 2], E, a, M)
        hres = np.where(ok, np.abs(num / den), 0.0)
    live = np.nonzero(result < 0)[0]
    while live.size:
        x, y, z = X[live, 0], X[live, 1], X[live, 2]
        px, py, pz = P[live, 0], P[live, 1], P[live, 2]
        e = E[live]
        with np.errstate(all="ignore"):
            g = geometry(x, y, z, a, M)
            h = time_step * np.minimum(1.0, np.maximum(g["r"] / (8.0 * M), 1.0 / 16.0))
            k1x, k1p = rhs(x, y, z, px, py, pz, e, a, M, g)
            hh = 0.5 * h
            k2x, k2p = rhs(x + hh * k1x[0], y + hh * k1x[1], z + hh * k1x[2],
                           px + hh * k1p[0], py + hh * k1p[1], pz + hh * k1p[2], e, a, M)
            k3x, k3p = rhs(x + hh * k2x[0], y + hh * k2x[1], z + hh * k2x[2],
                           px + hh * k2p[0], py + hh * k2p[1], pz + hh * k2p[2], e, a, M)
            k4x, k4p = rhs(x + h * k3x[0], y + h * k3x[1], z + h * k3x[2],
                           px + h * k3p[0], py + h * k3p[1], pz + h * k3p[2], e, a, M)
            h6 = h / 6.0
            new = [c + h6 * ((k1[i] + 2.0 * k2[i]) + (2.0 * k3[i] + k4[i]))
                   for c, k1, k2, k3, k4, i in
                   ((x, k1x, k2x, k3x, k4x, 0), (y, k1x, k2x, k3x, k4x, 1), (z, k1x, k2x, k3x, k4x, 2),
                    (px, k1p, k2p, k3p, k4p, 0), (py, k1p, k2p, k3p, k4p, 1),
                    (pz, k1p, k2p, k3p, k4p, 2))]
            nx, ny, nz, npx, npy, npz = new
            steps[live] += 1
            cx, cy, cz = nx - x, ny - y, nz - z
            seg = np.sqrt((cx * cx + cy * cy) + cz * cz)
            res = np.full(live.size, -1, dtype=np.int32)
            # 1. non-finite state
            fin = np.isfinite(nx) & np.isfinite(ny) & np.isfinite(nz) & np.isfinite(npx) & \
                np.isfinite(npy) & np.isfinite(npz)
            res[~fin] = ERROR
            hx, hy, hz = nx.copy(), ny.copy(), nz.copy()
            dadd = seg.copy()
            gn = geometry(nx, ny, nz, a, M)
            # 2. disk
            if disk is not None:
                cross = ((z > 0.0) & (nz <= 0.0)) | ((z < 0.0) & (nz >= 0.0))
                t = z / (z - nz)
                qx, qy = x + t * cx, y + t * cy
                s = qx * qx + qy * qy
                hitd = (res < 0) & cross & (d_lo <= s) & (s <= d_hi)
                res[hitd] = DISK
                hx[hitd], hy[hitd], hz[hitd] = qx[hitd], qy[hitd], 0.0
                dadd[hitd] = (t * seg)[hitd]
            # 3. horizon
            hor = (res < 0) & (gn["r"] <= rp)
            res[hor] = HORIZON
            dadd[hor] = 0.0
            dadd[~fin] = 0.0
            # 4. distance
            nd = dist[live] + dadd
            far = (res < 0) & (nd > max_dist)
            res[far] = MAX_DISTANCE
            # 5. steps
            res[(res < 0) & (steps[live] >= max_steps)] = MAX_STEPS
            if diag:
                num, den = hamiltonian_parts(nx, ny, nz, npx, npy, npz, e, a, M, gn)
                acc = fin
                hres[live] = np.where(acc, np.maximum(hres[live], np.abs(num / den)), hres[live])
                lzd[live] = np.where(acc, np.abs((nx * npy - ny * npx) - lz0[live]), lzd[live])
        dist[live] = nd
        X[live] = np.stack([nx, ny, nz], axis=1)
        P[live] = np.stack([npx, npy, npz], axis=1)
        hit[live] = np.stack([hx, hy, hz], axis=1)
        chord[live] = np.stack([cx, cy, cz], axis=1)
        result[live] = res
        live = live[res < 0]
    out = dict(result=result, steps=steps, hit=hit, distance=dist, chord=chord, n=n,
               b=lz0 / E)
    if diag:
        out["h_residual"] = hres
        out["lz_drift"] = lzd
    return out


def sky_fields(tr):
    """sky_x/y/z: the exit chord of a MAX_DISTANCE ray, else not written."""
    return tr["result"] == MAX_DISTANCE, tr["chord"]


def colour(tr, bh, disk, flags):
    """The frame colour contract for a traced set (no sky map): [N, 3]."""
    res, hit, n, c = tr["result"], tr["hit"], tr["n"], tr["chord"]
    N = len(res)
    with np.errstate(all="ignore"):
        cl = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        unit = c / cl[:, None]
        dy = np.where(res == MAX_DISTANCE, unit[:, 1], n[:, 1])
        t = 0.5 * (dy + 1.0)
        rgb = np.stack([(1.0 - t) * 1.0 + t * 0.5, (1.0 - t) * 1.0 + t * 0.7,
                        (1.0 - t) * 1.0 + t * 1.0], axis=1)
        rgb[res == HORIZON] = 0.0
        dk = res == DISK
        if disk is not None and dk.any():
            hx, hy = hit[dk, 0], hit[dk, 1]
            rxy = np.sqrt(hx * hx + hy * hy)
            nr = np.clip((rxy - disk.inner_radius) / (disk.outer_radius - disk.inner_radius), 0, 1)
            su = np.sqrt(1.0 - nr)
            T = np.clip(disk.temperature_scale * (2000.0 + 18000.0 * (su * np.sqrt(su))),
                        1000.0, 40000.0)
            tt = (T - 1000.0) / (40000.0 - 1000.0)
            r = np.where(tt < 0.5, tt * 2.0, 1.0)
            g = np.where(tt < 0.25, 0.0, np.where(tt < 0.75, (tt - 0.25) * 2.0, 1.0))
            b = np.where(tt < 0.5, 0.0, (tt - 0.5) * 2.0)
            br = 0.2 + 0.8 * (tt * tt)
            r, g, b = r * br, g * br, b * br
            if flags & abi.BHRT_FLAG_DOPPLER:
                d = unit[dk]
                sp, cp = hy / rxy, hx / rxy
                dop = 1.0 + ((d[:, 0] * -sp + d[:, 1] * cp) + d[:, 2] * 0.0) * 0.5
                zf = dop * np.sqrt(1.0 - bh.schwarzschild_radius / rxy)
                lo = zf < 1.0
                r, b = (np.where(lo, np.minimum(1.0, r * (2.0 - zf)), r * (2.0 - zf)),
                        np.where(lo, b * zf, np.minimum(1.0, b * zf)))
                beam = (dop * dop) * (dop * dop)
                r, g, b = (np.clip(v * beam, 0.0, 1.0) for v in (r, g, b))
            rgb[dk] = np.stack([r, g, b], axis=1)
    assert rgb.shape == (N, 3)
    return rgb


def critical_b(a, M, prograde):
    """The analytic critical impact parameter of Kerr spin a (signed; a != 0) on one side."""
    s = -1.0 if prograde else 1.0
    r = 2.0 * M * (1.0 + math.cos(2.0 / 3.0 * math.acos(s * a / M)))
    return -(r ** 3 - 3.0 * M * r * r + a * a * r + a * a * M) / (a * (r - M))


# ---- the scenes of the tests (tests/test_kerr_cpu.py, tests/test_gpu_kerr.py) ----
MASS = 1.0
SCENE_DT, SCENE_DIST, SCENE_STEPS = 0.25, 60.0, 2000
FRAME_SIZES = ((48, 27), (49, 27))      # the odd width puts an L_z = 0 column over the pole
SCENES = ((0.0, (6.0, 12.0)), (0.5, (4.3, 12.0)), (0.9, (2.4, 12.0)))   # (spin, disk radii)
FAN_ORIGIN, FAN_RAYS = (20.0, 0.0, 0.0), 64
_cache = {}


def camera():
    return abi.Camera(abi.v3(0.0, -18.0, 4.0), abi.v3(0.0, 18.0, -4.0), abi.v3(0.0, 0.0, 1.0), 40.0)


def scene(spin, disk):
    """(bh, disk, cfg) of a test scene as the library takes them."""
    return (abi.black_hole(MASS, spin), abi.disk(*disk) if disk else None,
            abi.sim_config(SCENE_DT, SCENE_DIST, SCENE_STEPS))


def frame_rule(spin, disk, width, height, eps=0.0):
    """The rule's frame (traced once per session): eps != 0 adds eps times a fixed unit vector per
    ray to its direction -- the perturbation of the knife-edge test."""
    key = (spin, disk, width, height, eps)
    if key not in _cache:
        cam = camera()
        d = camera_dirs(cam, width, height)
        if eps:
            e = normalise(np.random.default_rng(7).normal(size=d.shape))
            d = d + eps * e
        o = np.tile([cam.position.x, cam.position.y, cam.position.z], (len(d), 1))
        tr = trace(o, d, spin, MASS, disk, SCENE_DT, SCENE_DIST, SCENE_STEPS, diag=True)
        tr["dirs"] = d
        _cache[key] = tr
    return _cache[key]


def knife_edge(spin, disk, width, height, eps=1e-9):
    """Rays whose class or step count changes under a +-eps direction perturbation."""
    base = frame_rule(spin, disk, width, height)
    bad = np.zeros(len(base["result"]), dtype=bool)
    for s in (eps, -eps):
        p = frame_rule(spin, disk, width, height, s)
        bad |= (p["result"] != base["result"]) | (p["steps"] != base["steps"])
    return bad


def fan(side, count=FAN_RAYS, b_lo=0.5, b_hi=9.0):
    """Equatorial directions from FAN_ORIGIN on one side (side = +1: n_y > 0), spread evenly in
    the sine of the angle from the -x axis, i.e. roughly evenly in impact parameter."""
    s = np.linspace(b_lo, b_hi, count) / FAN_ORIGIN[0]
    return np.stack([-np.sqrt(1.0 - s * s), side * s, np.zeros(count)], axis=1)


def critical_angle_b(spin, side, rounds=7):
    """The rule's critical impact parameter on one side, by bracketing the capture / escape
    boundary of equatorial rays from FAN_ORIGIN: (b, the bracket's relative width)."""
    key = ("crit", spin, side)
    if key in _cache:
        return _cache[key]
    lo, hi = 0.0, 0.6
    o = np.tile(FAN_ORIGIN, (66, 1))
    for _ in range(rounds):
        al = np.linspace(lo, hi, 66)
        d = np.stack([-np.cos(al), side * np.sin(al), 0.0 * al], axis=1)
        tr = trace(o, d, spin, MASS, None, SCENE_DT, SCENE_DIST, SCENE_STEPS)
        cap = tr["result"] == HORIZON
        k = int(np.nonzero(cap)[0].max())
        assert cap[:k + 1].all() and not cap[k + 1:].any(), (spin, side)
        assert (tr["result"][k + 1:] == MAX_DISTANCE).all(), (spin, side)
        lo, hi = al[k], al[k + 1]
        b, width = 0.5 * (tr["b"][k] + tr["b"][k + 1]), abs(tr["b"][k + 1] - tr["b"][k])
    _cache[key] = (float(b), float(width / abs(b)))
    return _cache[key]


def analytic_b(spin, b_sign):
    """The analytic critical impact parameter with the sign of b_sign, in the integration's
    convention (spin a~ = -spin * MASS): 3 sqrt(3) M at spin 0."""
    a = spin_a(spin, MASS)
    if a == 0.0:
        return math.copysign(3.0 * math.sqrt(3.0) * MASS, b_sign)
    both = (critical_b(a, MASS, True), critical_b(a, MASS, False))
    return [w for w in both if w * b_sign > 0][0]
