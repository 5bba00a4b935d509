"""Device-resident particle systems on the GPU (bhrt_particles_*; the rule: include/bhrt_api.h,
restated in particles_rule.py). Every comparison is bit-exact -- doubles and floats as unsigned
integer views, so NaN payloads count -- with no tolerance and no exempted case:

  * update parity: the resident array after bhrt_particles_update_device equals, field for field,
    the host array after bhrt_update_particles_steps, over the step sequence (1, 1, 3, 10), on the
    systems of tests/golden/particles.npz and synthetic ones of 1 to 65 795 particles (more than
    256 workgroups: the scan loops) whose updates really deactivate particles;
  * extract: after each of those steps, for six activity patterns and every max_count of
    {1, A-1, A, A+1, n, n+5}, every output equals the rule on the downloaded array and
    bh_get_particle_data, the count is right, sentinel-filled outputs are untouched at and beyond
    it, subsets of the outputs work and the host form equals the device form;
  * the block_active invariant, the stream rules, and upload after a host-side change.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from bhrt import abi
import particles_rule as pr

pytestmark = pytest.mark.gpu

P = C.POINTER
STEPS = (1, 1, 3, 10)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000, 65795)
ELEM = {f: int(np.prod(s, dtype=np.int64)) * np.dtype(d).itemsize
        for f, (s, d) in abi.PARTICLE_DATA_SHAPES.items()}
ELEM["count"] = 4


def _bind(L):
    PS = P(abi.ParticleSystem)
    L.add_particle.argtypes = [PS, P(abi.Vector3D), P(abi.Vector3D), C.c_double, C.c_int]
    L.remove_particle.argtypes = [PS, C.c_int]
    L.bhrt_update_particles_steps.argtypes = [PS, P(abi.BlackHoleParams), P(abi.SimulationConfig),
                                              C.c_int, P(C.c_double)]
    L.bh_initialize.restype = C.c_void_p
    L.bh_shutdown.argtypes = [C.c_void_p]
    L.bh_get_particle_data.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, P(C.c_int)]
    return L


class HostSystem:
    """A ParticleSystem over a numpy array of abi.PARTICLE_DTYPE (with spare capacity)."""

    def __init__(self, particles, spare=8):
        n = len(particles)
        self.store = np.zeros(n + spare, dtype=abi.PARTICLE_DTYPE)
        self.store[:n] = particles
        next_id = int(particles["id"].max()) + 1 if n else 1
        self.ps = abi.ParticleSystem(C.cast(self.store.ctypes.data, P(abi.Particle)), n + spare, n,
                                     next_id, None)

    @property
    def a(self):
        return self.store[:self.ps.count]


@pytest.fixture(scope="module")
def env(bhrt_lib):
    L = _bind(bhrt_lib.load())
    ctx = L.bh_initialize()
    yield bhrt_lib, L, ctx
    L.bh_shutdown(ctx)


def _scene():
    return abi.black_hole(1.0, 0.0), abi.sim_config(pr.DT, 100.0, 1000, 1e-6)


def _host_update(L, hs, bh, cfg, steps):
    assert L.bhrt_update_particles_steps(C.byref(hs.ps), C.byref(bh), C.byref(cfg), steps, None) == 0


def _device_outputs(max_count, fields=pr.FIELDS):
    """Sentinel-filled device byte arrays for the fields, and the abi.ParticleData over them."""
    import torch
    t = {f: torch.full(((1 if f == "count" else max_count) * ELEM[f],), pr.SENTINEL,
                       dtype=torch.uint8, device="cuda") for f in fields}
    return t, abi.ParticleData(**{f: v.data_ptr() for f, v in t.items()})


def _typed(raw, max_count):
    """The byte arrays read back, as the rule's dtypes and shapes."""
    out = {}
    for f, t in raw.items():
        b = t.cpu().numpy()
        if f == "count":
            out[f] = b.view(np.int32)
        else:
            tail, dtype = abi.PARTICLE_DATA_SHAPES[f]
            out[f] = b.view(dtype).reshape((max_count,) + tail)
    return out


def _same_outputs(got, want, what):
    assert sorted(got) == sorted(want), what
    for f in want:
        pr.same_bits(got[f], want[f], f"{what}: {f}")


def _get_particle_data(L, ctx, hs, max_count):
    """bh_get_particle_data on the host system: positions, velocities, types of `count` rows."""
    pos, vel = np.zeros((max_count, 3)), np.zeros((max_count, 3))
    typ = np.zeros(max_count, dtype=np.int32)
    cnt = C.c_int(max_count)
    assert L.bh_get_particle_data(ctx, C.byref(hs.ps), pos.ctypes.data, vel.ctypes.data,
                                  typ.ctypes.data, C.byref(cnt)) == 0
    return pos[:cnt.value], vel[:cnt.value], typ[:cnt.value], cnt.value


def _check_extracts(env, ps, hs, what, stream=None):
    """Every max_count of the rule, device and host form, and two subsets, against the rule on
    hs.a (the downloaded array) and bh_get_particle_data."""
    lib, L, ctx = env
    n = len(hs.a)
    A = int((hs.a["active"] != 0).sum())
    for mc in pr.max_counts(n, A):
        want = pr.apply(hs.a, mc)
        raw, out = _device_outputs(mc)
        lib.particles_extract_device(ps, mc, out, stream)
        got = _typed(raw, mc)
        _same_outputs(got, want, f"{what}, max_count {mc}")
        assert got["count"][0] == min(A, mc), (what, mc)
        pos, vel, typ, cnt = _get_particle_data(L, ctx, hs, mc)
        assert cnt == got["count"][0], (what, mc)
        pr.same_bits(got["positions"][:cnt], pos, f"{what}: positions vs bh_get_particle_data")
        pr.same_bits(got["velocities"][:cnt], vel, f"{what}: velocities vs bh_get_particle_data")
        assert np.array_equal(got["types"][:cnt], typ), (what, mc)
        host = lib.particles_extract(ps, mc, fill=0)
        for f in pr.FIELDS:   # the host form: the same rows, and what it held beyond the count
            rows = 1 if f == "count" else cnt
            pr.same_bits(host[f][:rows], got[f][:rows], f"{what}: host form {f}")
            assert not host[f][rows:].any(), (what, mc, f)
    for fields in (("ids", "xyz32", "count"), ("velocities",)):   # the rest NULL
        mc = max(1, A - 1)
        raw, out = _device_outputs(mc, fields)
        lib.particles_extract_device(ps, mc, out, stream)
        _same_outputs(_typed(raw, mc), pr.apply(hs.a, mc, fields), f"{what}, subset {fields}")
        host = lib.particles_extract(ps, mc, fields=fields, fill=0)
        w = pr.extract(hs.a, mc)
        for f in fields:
            if f != "count":
                pr.same_bits(host[f][:w["count"]], w[f], f"{what}: host subset {f}")


def _walk(env, particles, bh, cfg, what, patterns=("keep",)):
    """The step sequence on a resident object and on a host copy, for each activity pattern:
    download == host array after every step, and the extracts of _check_extracts."""
    lib, L, ctx = env
    res = HostSystem(particles)   # what the resident object is made of and downloaded into
    ps = lib.particles_create(res.ps)
    deactivated = 0
    try:
        for pat in patterns:
            start = particles.copy()
            if pat != "keep":
                start["active"] = pr.activity(len(start), pat)
            host = HostSystem(start)
            res.a[:] = start
            lib.particles_upload(ps, res.ps)
            assert lib.particles_state(ps)["count"] == len(start)
            _check_extracts(env, ps, host, f"{what} {pat} after upload")
            for k, s in enumerate(STEPS):
                before = lib.particles_state(ps)["updates"]
                lib.particles_update_device(ps, bh, cfg, s)
                assert lib.particles_state(ps)["updates"] == before + 1
                _host_update(L, host, bh, cfg, s)
                res.a["age"] = -1.0
                lib.particles_download(ps, res.ps)
                pr.same_particles(res.a, host.a, f"{what} {pat} step {k} (+{s})")
                _check_extracts(env, ps, host, f"{what} {pat} step {k} (+{s})")
            deactivated += int(((start["active"] != 0) & (host.a["active"] == 0)).sum())
        lib.particles_update_device(ps, bh, cfg, 0)   # a no-op
        lib.particles_download(ps, res.ps)
        pr.same_particles(res.a, host.a, f"{what}: steps 0")
    finally:
        lib.particles_destroy(ps)
    return deactivated


@pytest.mark.parametrize("n", SIZES)
def test_update_parity_and_extracts_on_synthetic_systems(env, n):
    bh, cfg = _scene()
    particles = pr.synthetic(n)
    geo = (particles["type"] == abi.PARTICLE_TEST) & \
        (np.linalg.norm(particles["position"], axis=1) < 20 * pr.RS)
    deactivated = _walk(env, particles, bh, cfg, f"n {n}", pr.PATTERNS)
    if n >= 63:   # the systems do what they are for
        assert deactivated > 0 and geo.any() and len(set(particles["type"])) == 4


def test_update_parity_and_extracts_on_the_golden_systems(env):
    g = golden("particles")
    fields = (("pos", "position"), ("vel", "velocity"), ("type", "type"), ("active", "active"),
              ("id", "id"), ("age", "age"), ("temp", "temperature"), ("mass", "mass"),
              ("tdil", "time_dilation"))
    for c in range(int(g["ncases"])):
        pre = f"case{c}_"
        bh = abi.BlackHoleParams(*g[pre + "bh"])
        cfg = abi.sim_config(float(g[pre + "in"][4]), 100.0, 1000, 1e-6)
        a = np.zeros(int(g[pre + "in"][5]), dtype=abi.PARTICLE_DTYPE)
        for k, f in fields:
            a[f] = g[pre + "init_" + k]
        _walk(env, a, bh, cfg, f"golden case {c}")


@pytest.mark.parametrize("n", (1000, 65795))
def test_block_counts_of_the_update_equal_a_fresh_count_pass(env, n):
    """An object updated by the counting kernel and an object made (count pass) from the host array
    after the same updates extract the same bits."""
    lib, L, ctx = env
    bh, cfg = _scene()
    a, b = HostSystem(pr.synthetic(n, seed=1)), HostSystem(pr.synthetic(n, seed=1))
    updated = lib.particles_create(a.ps)
    fresh = None
    try:
        for s in (15, 4):
            lib.particles_update_device(updated, bh, cfg, s)
            _host_update(L, b, bh, cfg, s)
            if fresh is None:
                fresh = lib.particles_create(b.ps)
            else:
                lib.particles_upload(fresh, b.ps)
            assert (b.a["active"] == 0).any()
            for mc in (n, max(1, n // 3)):
                got = [lib.particles_extract(p, mc, fill=3) for p in (updated, fresh)]
                for f in pr.FIELDS:
                    pr.same_bits(got[0][f], got[1][f], f"n {n} after {s} steps: {f}")
                assert got[0]["count"][0] == min(mc, int((b.a["active"] != 0).sum()))
    finally:
        lib.particles_destroy(updated)
        lib.particles_destroy(fresh)


def _busy():
    import torch
    sleep = getattr(torch.cuda, "_sleep", None)
    if sleep is not None:
        sleep(20_000_000)
    else:
        m = torch.ones(2048, 2048, device="cuda")
        for _ in range(8):
            m = m @ m * 1e-3


def _expected_ticks(env, particles, bh, cfg, ticks, mc):
    """The outputs of `ticks` ticks (one update step, one extract) of a serial run."""
    lib, L, ctx = env
    host = HostSystem(particles)
    want = []
    for _ in range(ticks):
        _host_update(L, host, bh, cfg, 1)
        want.append(pr.apply(host.a, mc))
    return want


@pytest.mark.parametrize("explicit", (False, True), ids=("null_stream", "torch_stream"))
def test_stream_orders_after_fills_behind_a_busy_kernel(env, explicit):
    """Outputs sentinel-filled on a stream behind a busy kernel, no host sync before update +
    extract on that stream (NULL: the default stream's order), read back on it: the extracts, not
    the fill."""
    import torch
    lib, L, ctx = env
    bh, cfg = _scene()
    n, mc, ticks = 1000, 1005, 3
    particles = pr.synthetic(n, seed=2)
    want = _expected_ticks(env, particles, bh, cfg, ticks, mc)
    res = HostSystem(particles)
    ps = lib.particles_create(res.ps)
    stream = torch.cuda.Stream() if explicit else torch.cuda.current_stream()
    if not explicit:
        assert stream.cuda_stream == 0
    try:
        outs = [_device_outputs(mc) for _ in range(ticks)]
        torch.cuda.synchronize()   # (allocation done; everything below stays queued)
        with torch.cuda.stream(stream):
            _busy()
            for raw, out in outs:
                for t in raw.values():
                    t.fill_(pr.SENTINEL)
                lib.particles_update_device(ps, bh, cfg, 1, stream.cuda_stream or None)
                lib.particles_extract_device(ps, mc, out, stream.cuda_stream or None)
            for k, (raw, out) in enumerate(outs):
                _same_outputs(_typed(raw, mc), want[k], f"tick {k}")
    finally:
        lib.particles_destroy(ps)


def test_two_objects_interleaved_on_two_streams(env):
    """Ticks of two objects issued alternately on two streams with no synchronise in between give
    the bits of the serial runs."""
    import torch
    lib, L, ctx = env
    bh, cfg = _scene()
    sizes, ticks = (1000, 777), 4
    parts = [pr.synthetic(n, seed=3 + i) for i, n in enumerate(sizes)]
    want = [_expected_ticks(env, p, bh, cfg, ticks, len(p)) for p in parts]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    systems = [HostSystem(p) for p in parts]
    objs = [lib.particles_create(s.ps) for s in systems]
    try:
        outs = [[_device_outputs(len(p)) for _ in range(ticks)] for p in parts]
        torch.cuda.synchronize()
        for k in range(ticks):
            for i in range(2):
                lib.particles_update_device(objs[i], bh, cfg, 1, streams[i].cuda_stream)
                lib.particles_extract_device(objs[i], len(parts[i]), outs[i][k][1],
                                             streams[i].cuda_stream)
        torch.cuda.synchronize()
        for i in range(2):
            for k in range(ticks):
                _same_outputs(_typed(outs[i][k][0], len(parts[i])), want[i][k],
                              f"object {i} tick {k}")
    finally:
        for o in objs:
            lib.particles_destroy(o)


def test_upload_after_a_host_side_change(env):
    """remove_particle and add_particle on the host system, then upload: the count changes and the
    next extract is of the new array; a download into a system of another count is refused."""
    lib, L, ctx = env
    bh, cfg = _scene()
    n = 300
    hs = HostSystem(pr.synthetic(n, seed=9))
    ps = lib.particles_create(hs.ps)
    try:
        lib.particles_update_device(ps, bh, cfg, 2)
        lib.particles_download(ps, hs.ps)
        for pid in hs.a["id"][[0, 17, 255, 256, 299]]:
            assert L.remove_particle(C.byref(hs.ps), int(pid)) == 0
        added = [L.add_particle(C.byref(hs.ps), C.byref(abi.v3(9.0 + i, 0.5, -0.25)),
                                C.byref(abi.v3(0.0, 0.3, 0.01)), 1.0, abi.PARTICLE_TEST)
                 for i in range(5)]
        assert min(added) > int(hs.store["id"][:n].max()) and hs.ps.count == n + 5
        with pytest.raises(lib.BhrtError, match="resident"):
            lib.particles_download(ps, hs.ps)
        lib.particles_upload(ps, hs.ps)
        assert lib.particles_state(ps) == {"count": n + 5, "device": 0, "updates": 1}
        _check_extracts(env, ps, hs, "after upload")
        got = lib.particles_extract(ps, n + 5)
        c = int(got["count"][0])   # the added particles are active and the last in array order
        assert c == int((hs.a["active"] != 0).sum()) and got["ids"][c - 5:c].tolist() == added
        lib.particles_update_device(ps, bh, cfg, 1)
        _host_update(L, hs, bh, cfg, 1)
        _check_extracts(env, ps, hs, "a step after upload")
        bigger = HostSystem(pr.synthetic(5000, seed=4))   # growth of the device buffer
        lib.particles_upload(ps, bigger.ps)
        _check_extracts(env, ps, bigger, "after an upload that grows the buffer")
        # the refusals of a live object write nothing and leave the state alone
        state = lib.particles_state(ps)
        raw, out = _device_outputs(8)
        for call, message in ((lambda: lib.particles_update_device(ps, bh, cfg, -1), "steps"),
                              (lambda: lib.particles_update_device(ps, None, cfg, 1), "NULL"),
                              (lambda: lib.particles_extract_device(ps, 0, out), "max_count"),
                              (lambda: lib.particles_extract_device(ps, 8, None), "NULL"),
                              (lambda: lib.particles_extract_device(ps, 8, abi.ParticleData()),
                               "every output pointer is NULL")):
            with pytest.raises(lib.BhrtError, match=message):
                call()
        assert lib.particles_state(ps) == state
        for t in raw.values():
            assert (t.cpu().numpy() == pr.SENTINEL).all()
    finally:
        lib.particles_destroy(ps)
