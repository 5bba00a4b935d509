"""THE PARTICLE RULE of include/bhrt_api.h ("Physical particles: timelike geodesics for resident
systems") in numpy, on kerr_rule.py's own geometry and right-hand side: the step from a coordinate
velocity to a momentum, the tick's substep count, the RK4 substep on the seven components, the
tests after a substep, what is written, the diagnostics, the orbit helper and Bardeen's closed
forms. Float64 throughout, one operation per rounding, in the header's order; the particles of an
array (abi.PARTICLE_DTYPE) move side by side. Also the seeded populations of the tests and their
knife-edge sets."""
import math

import numpy as np

from bhrt import abi
import kerr_rule as kr

MOVED, CAPTURED, NOT_TIMELIKE, ERROR, INACTIVE = (abi.PSTAT_MOVED, abi.PSTAT_CAPTURED,
                                                  abi.PSTAT_NOT_TIMELIKE, abi.PSTAT_ERROR,
                                                  abi.PSTAT_INACTIVE)
WRITTEN = ("position", "velocity", "energy", "angular_momentum", "proper_time", "coordinate_time",
           "age", "time_dilation", "active")
KEPT = ("acceleration", "mass", "type", "id", "temperature")
MASS, DT = 1.0, 0.5


def spin_a(spin, mass):
    """The particle rule's spin parameter: a = +(spin * mass), forward in time."""
    return spin * mass


def momentum(pos, vel, a, M):
    """From velocity to momentum: (p [n, 3], E, u^t, N, r) at pos [n, 3] for velocities vel."""
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    with np.errstate(all="ignore"):
        g = kr.geometry(x, y, z, a, M)
        f, l = g["f"], (g["lx"], g["ly"], g["lz"])
        w = 1.0 + ((l[0] * vel[:, 0] + l[1] * vel[:, 1]) + l[2] * vel[:, 2])
        N = (1.0 - ((vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1]) + vel[:, 2] * vel[:, 2])) - \
            f * (w * w)
        ut = 1.0 / np.sqrt(N)
        c = f * w
        p = np.stack([ut * (vel[:, i] + c * l[i]) for i in range(3)], axis=1)
    return p, ut * (1.0 - c), ut, N, g["r"]


def stage(Y, E, a, M, g=None):
    """d(x, p, tau)/dt at Y [n, 7]: (xdot, pdot) / tdot and 1 / tdot, the reciprocal formed once;
    also tdot = E + f u."""
    x, y, z, px, py, pz = (Y[:, i] for i in range(6))
    if g is None:
        g = kr.geometry(x, y, z, a, M)
    xd, pd = kr.rhs(x, y, z, px, py, pz, E, a, M, g)
    u = E + ((g["lx"] * px + g["ly"] * py) + g["lz"] * pz)
    tdot = E + g["f"] * u
    it = 1.0 / tdot
    return np.stack([d * it for d in xd + pd] + [it], axis=1), tdot


def residual(Y, E, a, M, g=None):
    """|((p.p - E^2) - f u^2) + 1| / (((E^2 + p.p) + f u^2) + 1)."""
    num, den = kr.hamiltonian_parts(*(Y[:, i] for i in range(6)), E, a, M, g)
    return np.abs(num + 1.0) / (den + 1.0)


def substep_count(r, M, substeps):
    """m of a tick that starts at radius r."""
    q = np.minimum(1.0, np.maximum(r / (8.0 * M), 1.0 / 16.0))
    return substeps * np.ceil(1.0 / q).astype(np.int64)


def _near_integer(r, M, eps):
    """8 M / r within eps (relative) of an integer <= 16: where m jumps."""
    v = 8.0 * M / r
    k = np.rint(v)
    return (k >= 1.0) & (k <= 16.0) & (np.abs(v - k) <= eps * k)


def clone(particles):
    """A copy byte for byte, the padding of the 152-byte struct included."""
    flat = np.ascontiguousarray(particles)
    return np.frombuffer(bytearray(flat.tobytes()), dtype=flat.dtype).reshape(flat.shape)


def update(particles, spin, mass, dt, steps, substeps, eps=1e-9, record=None):
    """`steps` ticks of the array by the rule. Returns (the new array, diag): diag has h_residual,
    lz_drift, status, substeps by array index and `edge`, the knife-edge mask under eps; steps == 0
    returns (a copy, None). `record`, a list, gets per finished tick (Y [n, 7] with tau of this call
    in column 6, the mask of particles that completed that tick)."""
    out = clone(particles)
    if steps == 0:
        return out, None
    n = len(out)
    M = float(mass)
    a = spin_a(float(spin), M)
    rp = kr.r_plus(a, M)
    status = np.full(n, INACTIVE, dtype=np.int32)
    nsub = np.zeros(n, dtype=np.int32)
    hres, lzd = np.zeros(n), np.zeros(n)
    edge = np.zeros(n, dtype=bool)
    act = out["active"] != 0
    with np.errstate(all="ignore"):
        P, E, ut, N, r0 = momentum(out["position"], out["velocity"], a, M)
        inside = act & (r0 <= rp)
        timelike = np.isfinite(N) & (N > 0.0)
        edge |= act & (np.abs(r0 - rp) <= eps * rp)
        edge |= act & ~inside & (np.abs(N) <= eps)
    status[inside] = CAPTURED
    out["active"][inside] = 0
    status[act & ~inside & ~timelike] = NOT_TIMELIKE
    ran = act & ~inside & timelike
    status[ran] = MOVED
    Y = np.zeros((n, 7))
    Y[:, :3] = out["position"]
    Y[:, 3:6] = P
    lz0 = Y[:, 0] * Y[:, 4] - Y[:, 1] * Y[:, 3]
    live = np.nonzero(ran)[0]
    with np.errstate(all="ignore"):
        hres[live] = residual(Y[live], E[live], a, M)
        for _ in range(steps):
            if not live.size:
                break
            r = kr.geometry(Y[live, 0], Y[live, 1], Y[live, 2], a, M)["r"]
            m = substep_count(r, M, substeps)
            edge[live] |= _near_integer(r, M, eps)
            h = dt / m
            out["age"][live] += dt
            out["coordinate_time"][live] += dt
            done = np.zeros(live.size, dtype=bool)
            for j in range(int(m.max())):
                sel = ~done & (j < m)
                ii = live[sel]
                y, e, hs = Y[ii], E[ii], h[sel][:, None]
                hh = 0.5 * hs
                k1, _ = stage(y, e, a, M)
                k2, _ = stage(y + hh * k1, e, a, M)
                k3, _ = stage(y + hh * k2, e, a, M)
                k4, _ = stage(y + hs * k3, e, a, M)
                yn = y + (hs / 6.0) * ((k1 + 2.0 * k2) + (2.0 * k3 + k4))
                nsub[ii] += 1
                fin = np.isfinite(yn).all(axis=1)
                gn = kr.geometry(yn[:, 0], yn[:, 1], yn[:, 2], a, M)
                cap = fin & (gn["r"] <= rp)
                edge[ii] |= fin & (np.abs(gn["r"] - rp) <= eps * rp)
                Y[ii[fin]] = yn[fin]
                hres[ii[fin]] = np.maximum(hres[ii[fin]], residual(yn, e, a, M, gn)[fin])
                status[ii[~fin]] = ERROR
                status[ii[cap]] = CAPTURED
                out["active"][ii[~fin | cap]] = 0
                done[np.nonzero(sel)[0][~fin | cap]] = True
            if record is not None:
                mask = np.zeros(n, dtype=bool)
                mask[live[~done]] = True
                record.append((Y.copy(), mask))
            live = live[~done]
        idx = np.nonzero(ran)[0]
        d, tdot = stage(Y[idx], E[idx], a, M)
    lz = Y[idx, 0] * Y[idx, 4] - Y[idx, 1] * Y[idx, 3]
    lzd[idx] = np.abs(lz - lz0[idx])
    out["position"][idx] = Y[idx, :3]
    out["velocity"][idx] = d[:, :3]
    out["energy"][idx] = E[idx]
    out["angular_momentum"][idx] = lz
    out["proper_time"][idx] += Y[idx, 6]
    out["time_dilation"][idx] = tdot
    return out, dict(h_residual=hres, lz_drift=lzd, status=status, substeps=nsub, edge=edge)


def knife_edge(particles, spin, mass, dt, steps, substeps, eps=1e-9):
    """The particles that at some tick start have 8 M / r within eps (relative) of an integer
    <= 16, whose start point or a substep end has r within eps of r+, or whose N is within eps of
    0: where rounding decides an integer."""
    _, diag = update(particles, spin, mass, dt, steps, substeps, eps=eps)
    return diag["edge"] if diag else np.zeros(len(particles), dtype=bool)


# ---- the orbit helper and the closed forms ----
def orbit_velocity(x, y, a, M, prograde=True):
    """bhrt_kerr_orbit_velocity: (v [3], ok) of the circular equatorial geodesic through (x, y, 0)."""
    s = 1.0 if prograde else -1.0
    with np.errstate(all="ignore"):
        r = np.sqrt((x * x + y * y) - a * a)
        sm, sr = math.sqrt(M), np.sqrt(r)
        ok = (r > kr.r_plus(a, M)) & ((r * sr - 3.0 * M * sr) + s * (2.0 * a * sm) > 0.0)
        om = s * sm / (r * sr + s * (a * sm))
    return np.stack([om * -y, om * x, 0.0 * om], axis=-1), ok


def bardeen(r, a, M, prograde=True):
    """E and L_z of the circular equatorial geodesic at Boyer-Lindquist r (Bardeen 1972)."""
    s = 1.0 if prograde else -1.0
    sm = math.sqrt(M)
    den = r ** 0.75 * math.sqrt(r ** 1.5 - 3.0 * M * math.sqrt(r) + s * 2.0 * a * sm)
    E = (r ** 1.5 - 2.0 * M * math.sqrt(r) + s * a * sm) / den
    L = s * sm * (r * r - s * 2.0 * a * sm * math.sqrt(r) + a * a) / den
    return E, L


def isco(a, M, prograde=True):
    s = -1.0 if prograde else 1.0
    c = a / M
    z1 = 1.0 + (1.0 - c * c) ** (1.0 / 3.0) * ((1.0 + c) ** (1.0 / 3.0) + (1.0 - c) ** (1.0 / 3.0))
    z2 = math.sqrt(3.0 * c * c + z1 * z1)
    return M * (3.0 + z2 + s * math.sqrt((3.0 - z1) * (3.0 + z1 + 2.0 * z2)))


def carter_q(Y, E, a):
    """Carter's constant of states Y [n, 6+] with energies E."""
    x, y, z, px, py, pz = (Y[:, i] for i in range(6))
    r = kr.geometry(x, y, z, a, 1.0)["r"]
    ct = z / r
    st = np.sqrt(1.0 - ct * ct)
    lz = x * py - y * px
    pth = (x * px + y * py) * ct / st - r * st * pz
    return pth * pth + ct * ct * (a * a * (1.0 - E * E) + lz * lz / (st * st))


# ---- the populations of the tests (tests/test_kerr_particles_cpu.py, test_gpu_kerr_particles.py) ----
SPINS = (0.0, 0.5, 0.9)
COUNTS = (1, 63, 64, 65, 255, 256, 257, 1000)
SUBSTEPS = (1, 2)
STEPS = (0, 1, 7, 40)
_cache = {}


def blank(n):
    """n particles with every kept field filled with recognisable values."""
    p = np.zeros(n, dtype=abi.PARTICLE_DTYPE)
    i = np.arange(n)
    p["acceleration"] = np.stack([0.25 + i, -1.5 * i, 1e-3 * i], axis=1)
    p["mass"] = 1.0 + 0.125 * (i % 9)
    p["type"] = i % 4
    p["id"] = 100 + i
    p["temperature"] = 3000.0 + i
    p["active"] = 1
    p["age"] = 0.5 * (i % 5)
    p["coordinate_time"] = 2.0
    p["proper_time"] = 1.0
    return p


def circular(spin, radii, prograde=True, phase=0.0):
    """Circular equatorial orbits at Boyer-Lindquist radii (mass MASS), by the helper's formula."""
    a = spin_a(spin, MASS)
    radii = np.atleast_1d(np.asarray(radii, dtype=np.float64))
    p = blank(len(radii))
    rho = np.sqrt(radii * radii + a * a)
    x, y = rho * np.cos(phase), rho * np.sin(phase)
    v, ok = orbit_velocity(x, y, a, MASS, prograde)
    assert np.all(ok)
    p["position"] = np.stack([x, y, 0.0 * x], axis=1)
    p["velocity"] = v
    return p


def population(spin, n=1000, seed=2027):
    """The seeded GPU-test population of spin `spin`, first n particles: circular orbits both ways,
    inclined eccentric orbits with periapsis down to about 3 M, plungers that are captured within
    40 ticks (some within 7), every 7th particle inactive, two not-timelike particles, one inside
    r+, all four types. The special ones stand first, so that every count has some."""
    key = (spin, seed)
    if key not in _cache:
        N = max(COUNTS)
        rng = np.random.default_rng(seed + int(round(spin * 100)))
        a = spin_a(spin, MASS)
        rp = kr.r_plus(a, MASS)
        p = blank(N)
        kind = np.arange(N) % 5           # 0, 1 circular pro / retro; 2, 3 eccentric; 4 plunger
        phi = rng.uniform(0.0, 2.0 * math.pi, N)
        for i in range(N):
            k = kind[i]
            pro = k != 1
            lo = 1.05 * isco(a, MASS, pro)
            R = rng.uniform(lo, 20.0)
            rho = math.sqrt(R * R + a * a)
            x, y = rho * math.cos(phi[i]), rho * math.sin(phi[i])
            v, ok = orbit_velocity(np.float64(x), np.float64(y), a, MASS, pro)
            assert ok
            z = 0.0
            if k in (2, 3):               # slower than circular, out of the plane
                v = v * rng.uniform(0.62, 0.95)
                v[2] = rng.uniform(-0.12, 0.12)
                z = rng.uniform(-1.0, 1.0)
            if k == 4:                    # close in, falling
                R = rng.uniform(max(1.15 * rp, 2.15), 4.5)   # (outside the ergosphere)
                rho = math.sqrt(R * R + a * a)
                x, y = rho * math.cos(phi[i]), rho * math.sin(phi[i])
                vr = -rng.uniform(0.0, 0.3)
                v = np.array([vr * math.cos(phi[i]), vr * math.sin(phi[i]),
                              rng.uniform(-0.05, 0.05)])
                z = rng.uniform(-0.5, 0.5)
            p["position"][i] = (x, y, z)
            p["velocity"][i] = v
        p["active"][np.arange(N) % 7 == 1] = 0
        p["active"][8] = 7                # any non-zero flag is active
        for i, d in ((2, (0.0, 1.2, 0.0)), (6, (0.72, -0.72, 0.64))):   # |v| = 1.2
            p["position"][i] = (10.0, 0.0, 0.0) if i == 2 else (0.0, 6.0, 2.0)
            p["velocity"][i] = d
            p["active"][i] = 1
        p["position"][3] = (0.6 * rp, 0.3 * rp, 0.1)                    # inside r+, at rest
        p["velocity"][3] = 0.0
        p["active"][3] = 1
        _cache[key] = p
    return clone(_cache[key][:n])


def population_rule(spin, n, steps, substeps):
    """update() of population(spin, n), traced once per session."""
    key = ("rule", spin, n, steps, substeps)
    if key not in _cache:
        _cache[key] = update(population(spin, n), spin, MASS, DT, steps, substeps)
    return _cache[key]
