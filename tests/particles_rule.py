"""The extract rule of device-resident particle systems (include/bhrt_api.h, bhrt_particles_extract*)
restated in numpy, and the synthetic systems the tests of it share.

extract(particles, max_count) is bh_get_particle_data on the array with *count = max_count: the first
min(A, max_count) ACTIVE particles in array order, A the number of active ones. positions, velocities
and types are copied, ids is Particle.id, xyz32 and vel32 are (float) of the same doubles, count[0] is
the number written, and elements at or beyond it are not written: apply() writes the rule's result
into sentinel-filled arrays and leaves the rest alone, which is what a test compares with."""
import numpy as np

from bhrt import abi

FIELDS = abi.PARTICLE_DATA_FIELDS
SENTINEL = 0x5A   # every byte of an output array before the call


def extract(particles, max_count):
    """The rule on a numpy array of abi.PARTICLE_DTYPE: a dict of the six arrays, each of exactly
    count rows, and count."""
    assert max_count >= 1
    idx = np.nonzero(particles["active"] != 0)[0][:max_count]
    pos = np.ascontiguousarray(particles["position"][idx])
    vel = np.ascontiguousarray(particles["velocity"][idx])
    with np.errstate(over="ignore", invalid="ignore"):
        xyz32, vel32 = pos.astype(np.float32), vel.astype(np.float32)
    return {"positions": pos, "velocities": vel,
            "types": particles["type"][idx].astype(np.int32),
            "ids": particles["id"][idx].astype(np.int32),
            "xyz32": xyz32, "vel32": vel32, "count": int(len(idx))}


def sentinel_arrays(max_count, fields=FIELDS):
    """Host arrays of max_count elements (count: one), every byte SENTINEL."""
    out = {}
    for f in fields:
        if f == "count":
            out[f] = np.empty(1, dtype=np.int32)
        else:
            tail, dtype = abi.PARTICLE_DATA_SHAPES[f]
            out[f] = np.empty((max_count,) + tail, dtype=dtype)
        out[f].view(np.uint8)[...] = SENTINEL
    return out


def apply(particles, max_count, fields=FIELDS):
    """What the outputs must hold after the call, starting from sentinel_arrays: the rule's rows,
    the sentinel at and beyond the count."""
    want = extract(particles, max_count)
    out = sentinel_arrays(max_count, fields)
    for f in fields:
        if f == "count":
            out[f][0] = want["count"]
        else:
            out[f][:want["count"]] = want[f]
    return out


def bits(a):
    """The array as unsigned integers of its element size: NaN payloads and signed zeros count."""
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.nonzero(bits(got).ravel() != bits(want).ravel())[0]
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[:5]}"


def same_particles(got, want, what=""):
    """Two abi.PARTICLE_DTYPE arrays field for field, bit for bit (the struct has padding)."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in abi.PARTICLE_DTYPE.names:
        a = np.ascontiguousarray(got[f]).view(np.uint8)
        b = np.ascontiguousarray(want[f]).view(np.uint8)
        bad = np.nonzero((a != b).reshape(len(got), -1).any(axis=1))[0] if len(got) else []
        assert len(bad) == 0, f"{what}: field {f} differs at particles {bad[:5]}"


# ---- synthetic systems -------------------------------------------------------------------------
RS = 2.0   # the Schwarzschild radius of the tests' hole (mass 1)
DT = 0.05


def synthetic(n, seed=0):
    """n particles of mixed types around a mass-1 hole, as abi.PARTICLE_DTYPE, all active: orbiting
    disk and Hawking particles, test particles inside 20 rs (the geodesic branch) and outside it,
    and every 7th particle just outside rs moving inward at 0.9, so that updates with DT really
    deactivate particles (the radius falls by 0.045 a step from at most rs + 0.6)."""
    rng = np.random.default_rng(1000 + 17 * n + seed)
    a = np.zeros(n, dtype=abi.PARTICLE_DTYPE)
    r = rng.uniform(6.0, 60.0, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    z = rng.uniform(-0.05, 0.05, n) * r
    v = np.sqrt(1.0 / r)
    a["position"] = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    a["velocity"] = np.stack([-v * np.sin(phi), v * np.cos(phi), rng.normal(0, 0.01, n)], axis=1)
    a["type"] = rng.integers(0, 4, n)          # TEST, DISK, HAWKING, JET
    inward = np.arange(n) % 7 == 3
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rin = RS + rng.uniform(0.01, 0.6, n)
    a["position"][inward] = (d * rin[:, None])[inward]
    a["velocity"][inward] = (-0.9 * d)[inward]
    a["type"][inward] = np.where(np.arange(n) % 2 == 0, abi.PARTICLE_DISK, abi.PARTICLE_HAWKING)[inward]
    a["mass"] = rng.uniform(0.0, 1.0, n)
    a["temperature"] = rng.uniform(1e3, 1e4, n)
    a["age"] = rng.uniform(0.0, 3.0, n)
    a["time_dilation"] = 1.0
    a["active"] = 1
    a["id"] = np.arange(1, n + 1) * 3 + 1      # (not the index, so ids are told from ranks)
    return a


PATTERNS = ("all", "none", "alternating", "random_half", "first_only", "last_only")


def activity(n, pattern, seed=0):
    """The `active` flags of a pattern, int32 [n]."""
    f = np.zeros(n, dtype=np.int32)
    if pattern == "all":
        f[:] = 1
    elif pattern == "alternating":
        f[::2] = 1
    elif pattern == "random_half":
        f[:] = np.random.default_rng(77 + n + seed).integers(0, 2, n)
    elif pattern == "first_only":
        f[0] = 1
    elif pattern == "last_only":
        f[-1] = 1
    else:
        assert pattern == "none", pattern
    return f


def max_counts(n, active):
    """max_count in {1, A-1, A, A+1, n, n+5}, the valid ones, each once."""
    return sorted({m for m in (1, active - 1, active, active + 1, n, n + 5) if m >= 1})
