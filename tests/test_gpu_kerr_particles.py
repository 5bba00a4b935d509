"""Physical particles on the GPU: bhrt_particles_kerr_update_device (kerr.hip k_kerr_particles)
against the numpy rule (kerr_particles_rule.py; the rule: include/bhrt_api.h "Physical particles").

  * against the rule: every count of the wave and workgroup edges, three spins, substeps 1 and 2,
    0, 1, 7 and 40 ticks, on the seeded populations -- `active`, `status` and `substeps` equal
    outside the knife-edge set, the written floats and the diagnostics within the 1e-5 contract
    (conftest's compare: rtol 1e-5 with an absolute floor of 1e-9), the kept fields and the
    untouched particles byte-identical to the upload;
  * extract after a physical update, and the object's block counts against a fresh count pass;
  * purity: a permuted array, a repeated call, an explicit stream, two objects on two streams;
  * physics on the device: circular orbits stay circular and carry Bardeen's E and L_z;
  * the parity update of the same object before and after a physical call.
The worst observed ratios go to profiles/kerr_particles/test_figures.txt."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, golden
from bhrt import abi
import kerr_particles_rule as pr
import kerr_rule as kr
import particles_rule as ex

pytestmark = pytest.mark.gpu
FIGURES = os.path.join(ROOT, "profiles", "kerr_particles", "test_figures.txt")
EPS, FLOOR = 1e-5, 1e-9
FLOATS = ("position", "velocity", "energy", "angular_momentum", "proper_time", "coordinate_time",
          "age", "time_dilation")
DIAG_FLOATS = ("h_residual", "lz_drift")
M = pr.MASS
NMAX = max(pr.COUNTS)
ELEM = {f: int(np.prod(s, dtype=np.int64)) * np.dtype(d).itemsize
        for f, (s, d) in abi.PARTICLE_DATA_SHAPES.items()}
ELEM["count"] = 4


def _figure(key, text):
    """One line per key in profiles/kerr_particles/test_figures.txt, rewritten in place."""
    lines = {}
    if os.path.exists(FIGURES):
        for l in open(FIGURES).read().splitlines():
            if ": " in l:
                k, v = l.split(": ", 1)
                lines[k] = v
    lines[key] = text
    os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
    with open(FIGURES, "w") as f:
        f.write("".join(f"{k}: {v}\n" for k, v in sorted(lines.items())))


class HostSystem:
    """A ParticleSystem over a byte-for-byte copy of a numpy array of abi.PARTICLE_DTYPE."""

    def __init__(self, particles):
        self.a = pr.clone(particles)
        n = len(self.a)
        self.ps = abi.ParticleSystem(C.cast(self.a.ctypes.data, C.POINTER(abi.Particle)), n, n,
                                     int(self.a["id"].max()) + 1, None)


def _scene(spin, dt=pr.DT):
    return abi.black_hole(M, spin), abi.sim_config(dt, 100.0, 1000, 1e-6)


def _diag_tensors(n, fill=-7):
    import torch
    t = {f: torch.full((n,), fill, dtype=torch.float64 if abi.KERR_PARTICLES_DIAG_DTYPES[f] ==
                       np.float64 else torch.int32, device="cuda")
         for f in abi.KERR_PARTICLES_DIAG_FIELDS}
    return t, abi.KerrParticlesDiag(**{f: v.data_ptr() for f, v in t.items()})


def _device(lib, particles, spin, steps, substeps, stream=None, calls=1):
    """`calls` physical updates of `steps` ticks on a fresh object: (the downloaded array, the last
    call's diagnostics)."""
    import torch
    bh, cfg = _scene(spin)
    hs = HostSystem(particles)
    ps = lib.particles_create(hs.ps)
    try:
        t, dg = _diag_tensors(len(particles))
        torch.cuda.synchronize()      # (the fills are done, whatever stream the update takes)
        for _ in range(calls):
            lib.particles_kerr_update_device(ps, bh, cfg, steps, abi.KerrParticlesParams(substeps),
                                             dg, stream)
        lib.particles_download(ps, hs.ps)
        torch.cuda.synchronize()
        return hs.a, {f: v.cpu().numpy() for f, v in t.items()}
    finally:
        lib.particles_destroy(ps)


def _ratio(a, b):
    """The worst |a - b| against the contract's tolerance EPS max(|a|, |b|) + FLOOR; NaN == NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not a.size:
        return 0.0
    na, nb = np.isnan(a), np.isnan(b)
    assert (na == nb).all()
    ok = ~na
    tol = EPS * np.maximum(np.abs(a[ok]), np.abs(b[ok])) + FLOOR
    return float((np.abs(a[ok] - b[ok]) / tol).max()) if ok.any() else 0.0


def _check(start, got, gdiag, want, wdiag, what):
    """One device result against the rule's; returns the worst ratio to the tolerance."""
    keep = ~wdiag["edge"]
    for f, g, w in (("active", got["active"], want["active"]),
                    ("status", gdiag["status"], wdiag["status"]),
                    ("substeps", gdiag["substeps"], wdiag["substeps"])):
        bad = np.nonzero((g != w) & keep)[0]
        assert bad.size == 0, f"{what}: {f} differs at {bad[:10]}: got {g[bad[:10]]} want {w[bad[:10]]}"
    same = keep & (gdiag["status"] == wdiag["status"]) & (gdiag["substeps"] == wdiag["substeps"])
    worst = 0.0
    for f in FLOATS:
        r = _ratio(got[f][same], want[f][same])
        assert r <= 1.0, f"{what}: {f} at {r:.3g} of the tolerance"
        worst = max(worst, r)
    for f in DIAG_FLOATS:
        r = _ratio(gdiag[f][same], wdiag[f][same])
        assert r <= 1.0, f"{what}: {f} at {r:.3g} of the tolerance"
        worst = max(worst, r)
    for f in pr.KEPT:
        assert got[f].tobytes() == start[f].tobytes(), f"{what}: {f} changed"
    # untouched particles, in every byte; those captured at the start, in all but the flag
    st = gdiag["status"]
    raw_g = got.view(np.uint8).reshape(len(got), 152)
    raw_s = pr.clone(start)
    raw_s["active"][(st == pr.CAPTURED) & (gdiag["substeps"] == 0)] = 0
    raw_s = raw_s.view(np.uint8).reshape(len(got), 152)
    still = (st == pr.INACTIVE) | (st == pr.NOT_TIMELIKE) | \
        ((st == pr.CAPTURED) & (gdiag["substeps"] == 0))
    assert (raw_g[still] == raw_s[still]).all(), f"{what}: an untouched particle changed"
    assert (gdiag["h_residual"][still] == 0).all() and (gdiag["lz_drift"][still] == 0).all()
    assert (got["active"][st == pr.NOT_TIMELIKE] != 0).all()
    return worst


@pytest.mark.parametrize("steps", [s for s in pr.STEPS if s])
@pytest.mark.parametrize("substeps", pr.SUBSTEPS)
@pytest.mark.parametrize("spin", pr.SPINS)
def test_against_the_rule(bhrt_lib, spin, substeps, steps):
    """Every count; the rule is traced once on the whole population, of which a smaller count's
    particles are the first (a particle's result does not depend on the count:
    test_kerr_particles_cpu.py checks that of the rule, and this test of the kernel)."""
    want, wdiag = pr.population_rule(spin, NMAX, steps, substeps)
    worst, edge = 0.0, 0
    for n in pr.COUNTS:
        start = pr.population(spin, n)
        got, gdiag = _device(bhrt_lib, start, spin, steps, substeps)
        w = {f: v[:n] for f, v in wdiag.items()}
        worst = max(worst, _check(start, got, gdiag, want[:n], w, f"spin {spin} n {n}"))
        edge = int(w["edge"].sum())
    st = wdiag["status"]
    _figure(f"rule spin {spin} substeps {substeps} steps {steps}",
            f"worst |gpu - rule| / tolerance {worst:.3e} over counts {pr.COUNTS}; statuses "
            f"{np.bincount(st, minlength=5).tolist()}, substeps up to {int(wdiag['substeps'].max())}, "
            f"knife-edge particles {edge}")


@pytest.mark.parametrize("spin", pr.SPINS)
def test_zero_steps_is_a_no_op(bhrt_lib, spin):
    start = pr.population(spin, 257)
    got, gdiag = _device(bhrt_lib, start, spin, 0, 1)
    assert got.tobytes() == start.tobytes()
    for f, v in gdiag.items():          # nothing launched: the diagnostics keep their fill
        assert (v == -7).all(), f


@pytest.mark.parametrize("spin", pr.SPINS)
def test_extract_after_a_physical_update(bhrt_lib, spin):
    """bhrt_particles_extract_device gives the rule's active particles in array order, and the
    object's block counts equal a fresh count pass over the same array."""
    import torch
    lib = bhrt_lib
    bh, cfg = _scene(spin)
    n = NMAX
    start = pr.population(spin, n)
    want, wdiag = pr.population_rule(spin, n, 7, 1)
    assert not wdiag["edge"].any()
    hs = HostSystem(start)
    ps = lib.particles_create(hs.ps)
    fresh = None
    try:
        before = lib.particles_state(ps)["updates"]
        lib.particles_kerr_update_device(ps, bh, cfg, 7)
        assert lib.particles_state(ps)["updates"] == before + 1
        A = int((want["active"] != 0).sum())
        assert 0 < A < int((start["active"] != 0).sum())      # some were captured
        for mc in ex.max_counts(n, A):
            t = {f: torch.full(((1 if f == "count" else mc) * ELEM[f],), ex.SENTINEL,
                               dtype=torch.uint8, device="cuda") for f in ex.FIELDS}
            lib.particles_extract_device(ps, mc, abi.ParticleData(**{f: v.data_ptr()
                                                                     for f, v in t.items()}))
            torch.cuda.synchronize()
            c = int(t["count"].cpu().numpy().view(np.int32)[0])
            assert c == min(A, mc)
            ids = t["ids"].cpu().numpy().view(np.int32)
            assert ids[:c].tolist() == want["id"][want["active"] != 0][:c].tolist()
            assert (t["ids"].cpu().numpy()[4 * c:] == ex.SENTINEL).all()
            pos = t["positions"].cpu().numpy().view(np.float64).reshape(mc, 3)[:c]
            assert _ratio(pos, want["position"][want["active"] != 0][:c]) <= 1.0
        lib.particles_download(ps, hs.ps)
        again = HostSystem(hs.a)                              # a count pass over the same array
        fresh = lib.particles_create(again.ps)
        for mc in (n, max(1, A // 3)):
            got = [lib.particles_extract(p, mc, fill=3) for p in (ps, fresh)]
            for f in ex.FIELDS:
                ex.same_bits(got[0][f], got[1][f], f"spin {spin} max_count {mc}: {f}")
    finally:
        lib.particles_destroy(ps)
        if fresh is not None:
            lib.particles_destroy(fresh)


def test_a_permuted_array_gives_the_permuted_result(bhrt_lib):
    spin, n = 0.9, 777
    start = pr.population(spin, n)
    perm = np.random.default_rng(3).permutation(n)
    rows = lambda x: x.view(np.uint8).reshape(n, 152)        # (padding bytes included)
    moved = np.frombuffer(bytearray(rows(start)[perm].tobytes()), dtype=abi.PARTICLE_DTYPE)
    a, da = _device(bhrt_lib, start, spin, 7, 2)
    b, db = _device(bhrt_lib, moved, spin, 7, 2)
    assert (rows(a)[perm] == rows(b)).all()
    assert (da["status"] == pr.CAPTURED).any() and (da["status"] == pr.MOVED).any()
    for f in abi.KERR_PARTICLES_DIAG_FIELDS:
        ex.same_bits(da[f][perm], db[f], f)


def test_repeated_calls_and_streams_give_the_same_bits(bhrt_lib):
    import torch
    spin, n = 0.5, 1000
    start = pr.population(spin, n)
    a, da = _device(bhrt_lib, start, spin, 7, 1)
    b, db = _device(bhrt_lib, start, spin, 7, 1)
    s = torch.cuda.Stream()
    c, dc = _device(bhrt_lib, start, spin, 7, 1, stream=s.cuda_stream)
    for other, d in ((b, db), (c, dc)):
        assert other.tobytes() == a.tobytes()
        for f in abi.KERR_PARTICLES_DIAG_FIELDS:
            ex.same_bits(d[f], da[f], f)


def test_two_objects_interleaved_on_two_streams(bhrt_lib):
    """Calls on two objects issued alternately on two streams with no synchronise in between: each
    matches its own serial result bit for bit."""
    import torch
    lib = bhrt_lib
    spins, sizes, calls = (0.9, 0.0), (1000, 777), 3
    parts = [pr.population(s, n) for s, n in zip(spins, sizes)]
    want = [_device(lib, p, s, 2, 1, calls=calls)[0] for p, s in zip(parts, spins)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    systems = [HostSystem(p) for p in parts]
    objs = [lib.particles_create(s.ps) for s in systems]
    try:
        torch.cuda.synchronize()
        for _ in range(calls):
            for i in range(2):
                bh, cfg = _scene(spins[i])
                lib.particles_kerr_update_device(objs[i], bh, cfg, 2, None, None,
                                                 streams[i].cuda_stream)
        for i in range(2):
            lib.particles_download(objs[i], systems[i].ps)
            assert systems[i].a.tobytes() == want[i].tobytes(), i
            assert lib.particles_state(objs[i])["updates"] == calls
    finally:
        for o in objs:
            lib.particles_destroy(o)


def test_circular_orbits_on_the_device(bhrt_lib):
    """One population of circular orbits, both ways at three spins: E and L_z after one tick match
    Bardeen's closed forms to 1e-9 (the drift of L_z over one tick is far below that), and the
    radius stays within 1e-4 over 400 ticks, read every 40."""
    lib = bhrt_lib
    worst_r, worst_c = 0.0, 0.0
    for spin in pr.SPINS:
        a = pr.spin_a(spin, M)
        bh, cfg = _scene(spin)
        for pro in (True, False):
            lo = 1.05 * pr.isco(a, M, pro)
            radii = np.array([lo] + [r for r in (6.0, 10.0, 20.0) if r > lo])
            start = pr.circular(spin, radii, pro, phase=0.3)
            one, _ = _device(lib, start, spin, 1, 1)
            for i, r in enumerate(radii):
                E, L = pr.bardeen(r, a, M, pro)
                worst_c = max(worst_c, abs(one["energy"][i] - E) / abs(E),
                              abs(one["angular_momentum"][i] - L) / abs(L))
            hs = HostSystem(start)
            ps = lib.particles_create(hs.ps)
            try:
                for _ in range(10):
                    lib.particles_kerr_update_device(ps, bh, cfg, 40)
                    lib.particles_download(ps, hs.ps)
                    x = hs.a["position"]
                    r = kr.geometry(x[:, 0], x[:, 1], x[:, 2], a, M)["r"]
                    worst_r = max(worst_r, float((np.abs(r - radii) / radii).max()))
                assert (hs.a["active"] != 0).all()
                assert np.allclose(hs.a["coordinate_time"], start["coordinate_time"] + 200.0,
                                   rtol=0, atol=1e-9)
            finally:
                lib.particles_destroy(ps)
    _figure("circular orbits", f"worst |r - r0| / r0 over 400 ticks {worst_r:.3e} (bound 1e-4); "
            f"worst relative E, L_z error against Bardeen after one tick {worst_c:.3e} (bound 1e-9)")
    assert worst_r <= 1e-4 and worst_c <= 1e-9


def test_parity_update_before_and_after_a_physical_call(bhrt_lib, oracle):
    """bhrt_particles_update_device on the same object before and after a physical call still
    matches orc_update_particles (integers exact, floats to the 1e-5 contract) on a golden system."""
    lib = bhrt_lib
    O = oracle.lib
    O.orc_update_particles.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.BlackHoleParams),
                                       C.POINTER(abi.SimulationConfig), C.c_int]
    g = golden("particles")
    pre = "case0_"
    bh = abi.BlackHoleParams(*g[pre + "bh"])
    cfg = abi.sim_config(float(g[pre + "in"][4]), 100.0, 1000, 1e-6)
    a = np.zeros(int(g[pre + "in"][5]), dtype=abi.PARTICLE_DTYPE)
    for k, f in (("pos", "position"), ("vel", "velocity"), ("type", "type"), ("active", "active"),
                 ("id", "id"), ("age", "age"), ("temp", "temperature"), ("mass", "mass"),
                 ("tdil", "time_dilation")):
        a[f] = g[pre + "init_" + k]
    hs = HostSystem(a)
    ps = lib.particles_create(hs.ps)

    def parity(what):
        ref = pr.clone(hs.a)
        lib.particles_update_device(ps, bh, cfg, 3)
        lib.particles_download(ps, hs.ps)
        O.orc_update_particles(ref.ctypes.data, len(ref), C.byref(bh), C.byref(cfg), 3)
        for f in ("active", "type", "id"):
            assert np.array_equal(hs.a[f], ref[f]), (what, f)
        for f in ("position", "velocity", "age", "time_dilation", "energy", "proper_time"):
            assert _ratio(hs.a[f], ref[f]) <= 1.0, (what, f)

    try:
        parity("before")
        lib.particles_kerr_update_device(ps, bh, abi.sim_config(pr.DT), 2)
        lib.particles_download(ps, hs.ps)
        assert (hs.a["coordinate_time"][hs.a["energy"] != 0] > 0).all()
        parity("after")
    finally:
        lib.particles_destroy(ps)
