"""Physical photon paths on the GPU (bhrt_kerr_paths*; kerr.hip k_kerr_paths) against the numpy rule
(tests/kerr_paths_rule.py; stated in include/bhrt_api.h "Physical photon paths").

Inputs, from kerr_rule.py's scenes (M = 1, time_step 0.25, distance 60, 2000 steps, (spin, disk) in
{(0, [6, 12]), (0.5, [4.3, 12]), (0.9, [2.4, 12])}):
  set A  the 1323 rays of the 49x27 camera frame from (0, -18, 4), WITH the scene's disk: 20 full
         claims of 64 rays and one of 43, every wave a mix of disk, horizon and escaping rays, an
         L_z = 0 column over the pole; 33..309 steps, so 512 positions hold every path;
  set B  the 128 rays of the two equatorial fans from (20, 0, 0), WITHOUT a disk (they lie in z = 0
         exactly); 97..325 steps.
Counts and classes must equal the rule's on EVERY ray: the sets' knife-edge sets (rays whose class
or step count changes under a +-1e-9 direction perturbation) are empty (test_kerr_paths_cpu.py), so
nothing is exempt. Stored coordinates agree to the project's 1e-5 contract (conftest.compare: 1e-5
of the larger magnitude plus the 1e-9 floor): the kernel contracts products into FMAs and
multiplies by reciprocals where the rule divides, a few 1e-16 per operation, which the rule
amplifies by at most 1.2e4 into a point (test_kerr_cpu.py).

The worst observed ratios go to profiles/kerr_paths/test_figures.txt."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, compare
from bhrt import abi
import kerr_rule as kr
import kerr_paths_rule as kpr

pytestmark = pytest.mark.gpu
FIGURES = os.path.join(ROOT, "profiles", "kerr_paths", "test_figures.txt")
EPS = 1e-5
FILL = 7.0
P_FULL = 512
SHORT = 50
RGB = ("rgb_r", "rgb_g", "rgb_b")
HITS = ("result", "steps", "hit_x", "hit_y", "hit_z", "distance", "sky_x", "sky_y", "sky_z")
RECORDS = HITS + RGB + ("rgba8",)
SETS = [("A", spin, disk) for spin, disk in kr.SCENES] + [("B", spin, None) for spin, _ in kr.SCENES]
IDS = [f"set{w}-spin{s}" for w, s, _ in SETS]


def _figure(key, text):
    """One line per key in profiles/kerr_paths/test_figures.txt, rewritten in place."""
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


def _flags(spin):
    return abi.BHRT_FLAG_DOPPLER if spin else 0


def _rays(which, n=None):
    o, d = kpr.set_a_rays() if which == "A" else kpr.set_b_rays()
    rays = np.zeros(len(o), dtype=abi.RAY_DTYPE)
    rays["origin"] = o
    rays["direction"] = d
    return rays[:n] if n else rays


def _upload(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.float64).reshape(-1, 6)).cuda()


def _hit_tensors(n, fields, diag):
    import torch
    dt = {"result": torch.int32, "steps": torch.int32, "rgba32f": torch.float32,
          "rgba8": torch.uint8}
    t = {f: torch.full((n, 4) if f in abi.DISPLAY_FIELDS else (n,), 7,
                       dtype=dt.get(f, torch.float64), device="cuda") for f in fields}
    d = {f: torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
         for f in (("h_residual", "lz_drift") if diag else ())}
    return t, d


def _run(lib, rays, spin, disk, P=P_FULL, every=1, want=("xyz", "xyz32", "count"), hits=(),
         diag=False, stream=None, cfg=None):
    """One bhrt_kerr_paths_device call into fresh device arrays (fill 7), as numpy arrays."""
    import torch
    bh, dk, c = kr.scene(spin, disk)
    cfg = cfg or c
    n = len(rays)
    d_rays = _upload(rays)
    out = {}
    if "xyz" in want:
        out["xyz"] = torch.full((n, P, 3), FILL, dtype=torch.float64, device="cuda")
    if "xyz32" in want:
        out["xyz32"] = torch.full((n, P, 3), FILL, dtype=torch.float32, device="cuda")
    if "count" in want:
        out["count"] = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    paths = abi.Paths(*[out[k].data_ptr() if k in out else None for k in ("xyz", "xyz32", "count")])
    t, d = _hit_tensors(n, hits, diag)
    kd = abi.KerrDiag(d["h_residual"].data_ptr(), d["lz_drift"].data_ptr()) if diag else None
    torch.cuda.synchronize()
    lib.kerr_paths_device(d_rays.data_ptr(), n, bh, dk, cfg, P, every, _flags(spin), paths,
                          lib.soa_from_tensors(t) if hits else None, kd, stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in {**out, **t, **d}.items()}


_FULL = {}


def _full(lib, which, spin, disk):
    """The every-1, 512-position call of a whole set, run once for the module, left unchanged."""
    key = (which, spin)
    if key not in _FULL:
        got = _run(lib, _rays(which), spin, disk)
        for v in got.values():
            v.setflags(write=False)
        _FULL[key] = got
    return _FULL[key]


def _ratio(a, b):
    """The worst |diff| / tolerance of conftest.compare's float policy."""
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / (EPS * np.maximum(np.abs(a), np.abs(b)) + 1e-9)))


def _stored(xyz, count):
    """All stored points of a call, ray after ray: [sum(count), 3]."""
    return np.concatenate([xyz[i, :c] for i, c in enumerate(count)])


def _check_rows(got, want_rows, P, what):
    """Counts exact; every stored coordinate within tolerance; xyz32 the floats of xyz; every
    element at or beyond count[i] still the fill. Returns the worst |diff| / tol."""
    want_count = np.array([len(r) for r in want_rows], dtype=np.int32)
    bad = np.nonzero(got["count"] != want_count)[0]
    assert bad.size == 0, (what, bad[:10], got["count"][bad[:10]], want_count[bad[:10]])
    g, w = _stored(got["xyz"], want_count), np.concatenate(want_rows)
    worst = _ratio(g, w)
    print(f"{what}: {len(g)} stored points, worst |diff| / tol {worst:.3e}")
    compare({"xyz": g.reshape(-1)}, {"xyz": w.reshape(-1)}, EPS, check_sky=False, what=what,
            fields=("xyz",))
    beyond = np.arange(P)[None, :] >= want_count[:, None]
    assert (got["xyz"][beyond] == FILL).all(), what
    if "xyz32" in got:
        assert np.array_equal(_stored(got["xyz32"], want_count), g.astype(np.float32)), what
        assert (got["xyz32"][beyond] == np.float32(FILL)).all(), what
    return worst


# 1, 2. whole sets against the rule ----------------------------------------------------------------
@pytest.mark.parametrize("which,spin,disk", SETS, ids=IDS)
def test_paths_match_the_rule(bhrt_lib, which, spin, disk):
    rule = kpr.rule(which, spin, disk)
    got = _full(bhrt_lib, which, spin, disk)
    assert np.array_equal(got["count"], rule["steps"] + 1)    # every ray: nothing is exempt
    worst = _check_rows(got, rule["paths"], P_FULL, f"set {which} spin {spin}")
    counts = np.bincount(rule["result"], minlength=6).tolist()
    _figure(f"1-2 set {which} spin {spin}",
            f"{len(rule['steps'])} rays, classes {counts}, {int(got['count'].sum())} stored points, "
            f"longest {int(got['count'].max())}, worst |diff| / tol {worst:.3e}")


# 3. decimation and truncation ---------------------------------------------------------------------
@pytest.mark.parametrize("spin,disk", kr.SCENES, ids=[f"spin{s}" for s, _ in kr.SCENES])
def test_decimation_and_truncation(bhrt_lib, spin, disk):
    worst = 0.0
    for which, dk, n in (("B", None, None), ("A", disk, 130)):
        rays = _rays(which, n)
        rule = kpr.rule(which, spin, dk)["paths"][:len(rays)]
        every1 = _run(bhrt_lib, rays, spin, dk, want=("xyz", "count"))
        own = [every1["xyz"][i, :c] for i, c in enumerate(every1["count"])]
        assert every1["count"].max() < P_FULL
        for every in (3, 8, 100000):
            for P in (1, 2, 7, 64):
                got = _run(bhrt_lib, rays, spin, dk, P=P, every=every)
                what = f"set {which} spin {spin} every {every} P {P}"
                # a row is a pure function of its ray: the same kernel's every-1 points, decimated
                same = [kpr.stored_points(q, every, P) for q in own]
                assert np.array_equal(got["count"], [len(s) for s in same]), what
                assert np.array_equal(_stored(got["xyz"], got["count"]), np.concatenate(same)), what
                worst = max(worst, _check_rows(got, [kpr.stored_points(q, every, P) for q in rule],
                                               P, what))
    _figure(f"3 decimation spin {spin}", f"24 calls, worst |diff| / tol {worst:.3e}")


# 4. batch independence ----------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_batch_the_run_or_the_stream(bhrt_lib):
    import torch
    spin, disk = kr.SCENES[2]
    whole = _full(bhrt_lib, "A", spin, disk)
    for n in (1, 63, 64, 65, 130):
        part = _run(bhrt_lib, _rays("A", n), spin, disk)
        for k in ("xyz", "xyz32", "count"):
            assert np.array_equal(part[k], whole[k][:n]), (n, k)
    again = _run(bhrt_lib, _rays("A"), spin, disk)
    for k in ("xyz", "xyz32", "count"):
        assert np.array_equal(again[k], whole[k]), k
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        on = _run(bhrt_lib, _rays("A"), spin, disk, stream=s.cuda_stream)
        for k in ("xyz", "xyz32", "count"):
            assert np.array_equal(on[k], whole[k]), k


# 5. hit records -----------------------------------------------------------------------------------
@pytest.mark.parametrize("which,spin,disk", [SETS[0], SETS[2], SETS[5]], ids=[IDS[0], IDS[2], IDS[5]])
def test_hit_records_are_kerr_rays_devices(bhrt_lib, which, spin, disk):
    import torch
    rays = _rays(which)
    n = len(rays)
    got = _run(bhrt_lib, rays, spin, disk, hits=RECORDS, diag=True)
    bh, dk, cfg = kr.scene(spin, disk)
    t, d = _hit_tensors(n, RECORDS, True)
    d_rays = _upload(rays)
    torch.cuda.synchronize()
    bhrt_lib.kerr_rays_device(d_rays.data_ptr(), n, bh, dk, cfg, _flags(spin),
                              bhrt_lib.soa_from_tensors(t),
                              abi.KerrDiag(d["h_residual"].data_ptr(), d["lz_drift"].data_ptr()), None)
    torch.cuda.synchronize()
    for f, v in {**t, **d}.items():
        assert np.array_equal(got[f], v.cpu().numpy(), equal_nan=True), f
    # the points are unchanged by the hit launch, and the path's class is k_kerr's
    full = _full(bhrt_lib, which, spin, disk)
    assert np.array_equal(got["xyz"], full["xyz"]) and np.array_equal(got["count"], full["count"])
    assert np.array_equal(got["count"], got["steps"] + 1)
    last = got["xyz"][np.arange(n), got["count"] - 1]
    hit = np.stack([got["hit_x"], got["hit_y"], got["hit_z"]], 1)
    worst = _ratio(last, hit)
    differ = int((last.view(np.uint64) != hit.view(np.uint64)).any(axis=1).sum())
    print(f"set {which} spin {spin}: q_(m-1) vs hit_*: worst |diff| / tol {worst:.3e}, "
          f"{differ} of {n} rays differ in some bit")
    _figure(f"5 hits set {which} spin {spin}",
            f"q_(m-1) vs hit_* worst |diff| / tol {worst:.3e}; rays differing in any bit {differ} of {n}")
    compare({"q": last.reshape(-1)}, {"q": hit.reshape(-1)}, EPS, check_sky=False, what="q vs hit",
            fields=("q",))


# 6. edge classes ----------------------------------------------------------------------------------
def test_short_budget_zero_steps_and_an_origin_without_an_observer(bhrt_lib):
    spin, disk = kr.SCENES[2]
    bh, dk, _ = kr.scene(spin, disk)
    rays = _rays("A")
    n = len(rays)
    full = kpr.rule("A", spin, disk)
    short = kpr.rule("A", spin, disk, SHORT)
    cfg = abi.sim_config(kr.SCENE_DT, kr.SCENE_DIST, SHORT)
    got = _run(bhrt_lib, rays, spin, disk, P=64, hits=("result", "steps"), cfg=cfg)
    early = full["steps"] <= SHORT
    ended = early & (full["result"] != kr.MAX_STEPS)
    assert 50 < ended.sum() < n
    assert np.array_equal(got["count"][early], full["steps"][early] + 1)
    assert np.array_equal(got["result"][ended], full["result"][ended])
    assert (got["count"][~early] == SHORT + 1).all() and (got["result"][~early] == kr.MAX_STEPS).all()
    _check_rows(got, short["paths"], 64, "50 steps")
    # zero steps: the origin alone
    cfg0 = abi.sim_config(kr.SCENE_DT, kr.SCENE_DIST, 0)
    got = _run(bhrt_lib, rays[:130], spin, disk, P=4, hits=("result", "steps"), cfg=cfg0)
    assert (got["count"] == 1).all() and (got["result"] == kr.MAX_STEPS).all()
    assert np.array_equal(got["xyz"][:, 0], rays["origin"][:130]) and (got["xyz"][:, 1:] == FILL).all()
    assert np.array_equal(got["xyz32"][:, 0], rays["origin"][:130].astype(np.float32))
    # one device ray from inside the horizon: the origin alone, RAY_ERROR with steps 0
    bad = rays[:1].copy()
    bad["origin"][0] = (0.5, 0.0, 0.0)
    got = _run(bhrt_lib, bad, spin, disk, P=4, hits=("result", "steps", "hit_x"))
    assert got["count"].tolist() == [1] and got["xyz"][0, 0].tolist() == [0.5, 0.0, 0.0]
    assert (got["xyz"][0, 1:] == FILL).all()
    assert got["result"].tolist() == [kr.ERROR] and got["steps"].tolist() == [0]
    assert got["hit_x"].tolist() == [0.5]
    # the host form refuses that ray and leaves the arrays untouched
    L = bhrt_lib.load()
    xyz = np.full((1, 4, 3), FILL)
    count = np.full(1, 7, dtype=np.int32)
    paths = abi.Paths(xyz=xyz.ctypes.data, xyz32=None, count=count.ctypes.data)
    cfgf = kr.scene(spin, disk)[2]
    rc = L.bhrt_kerr_paths(bad.ctypes.data, 1, C.byref(bh), C.byref(dk), C.byref(cfgf), 4, 1, 0,
                           C.byref(paths), None, None)
    assert rc == -1 and "no static observer" in bhrt_lib.last_error()
    assert (xyz == FILL).all() and count.tolist() == [7]


# 7. output subsets --------------------------------------------------------------------------------
def test_count_alone_and_xyz32_alone_write_nothing_else(bhrt_lib):
    import torch
    spin, disk = kr.SCENES[1]
    bh, dk, cfg = kr.scene(spin, disk)
    rays = _rays("A")[::10]   # 133 rays of every class: rows shorter than P and truncated rows
    n, P, G = len(rays), 40, 256
    full = _run(bhrt_lib, rays, spin, disk, P=P)
    d_rays = _upload(rays)
    cnt = torch.full((n + 2 * G,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bhrt_lib.kerr_paths_device(d_rays.data_ptr(), n, bh, dk, cfg, P, 1, 0,
                               abi.Paths(None, None, cnt[G:].data_ptr()))
    torch.cuda.synchronize()
    c = cnt.cpu().numpy()
    assert np.array_equal(c[G:G + n], full["count"]) and (c[:G] == 7).all() and (c[G + n:] == 7).all()
    x32 = torch.full((n * P * 3 + 2 * G,), FILL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    bhrt_lib.kerr_paths_device(d_rays.data_ptr(), n, bh, dk, cfg, P, 1, 0,
                               abi.Paths(None, x32[G:].data_ptr(), None))
    torch.cuda.synchronize()
    x = x32.cpu().numpy()
    assert np.array_equal(x[G:G + n * P * 3].reshape(n, P, 3), full["xyz32"])
    assert (x[:G] == FILL).all() and (x[G + n * P * 3:] == FILL).all()
    assert (full["count"] == P).any() and (full["count"] < P).any()   # truncated and whole rows


# 8. statistics ------------------------------------------------------------------------------------
def test_statistics_count_the_path_launch_and_the_hit_launch(bhrt_lib):
    spin, disk = kr.SCENES[2]
    rays = _rays("A")
    n = len(rays)
    steps = int((_full(bhrt_lib, "A", spin, disk)["count"] - 1).sum())
    bhrt_lib.stats(reset=True)
    _run(bhrt_lib, rays, spin, disk, P=7, every=8, want=("count",))
    st = bhrt_lib.stats(reset=True)
    assert (st["launches"], st["rays"], st["iterations"]) == (1, n, steps)
    _run(bhrt_lib, rays, spin, disk, P=7, every=8, want=("count",), hits=("result",))
    st = bhrt_lib.stats(reset=True)
    assert (st["launches"], st["rays"], st["iterations"]) == (2, 2 * n, 2 * steps)


# 9. streams ---------------------------------------------------------------------------------------
def test_null_stream_orders_after_a_default_stream_fill(bhrt_lib):
    """A NULL hip_stream is ordered like the legacy default stream: fills of the outputs queued
    there before the call land before the paths, and a copy queued there after it sees them. A
    larger batch (8 x set A), so that a missing order would show; no synchronisation between."""
    import torch
    spin, disk = kr.SCENES[2]
    bh, dk, cfg = kr.scene(spin, disk)
    rays = np.tile(_rays("A"), 8)
    n, P = len(rays), 48
    ref = _run(bhrt_lib, rays, spin, disk, P=P, every=8, hits=("result", "hit_x"))
    d_rays = _upload(rays)
    torch.cuda.synchronize()
    for _ in range(3):
        xyz = torch.empty((n, P, 3), dtype=torch.float64, device="cuda")
        x32 = torch.empty((n, P, 3), dtype=torch.float32, device="cuda")
        cnt = torch.empty((n,), dtype=torch.int32, device="cuda")
        t, _d = _hit_tensors(n, ("result", "hit_x"), False)
        for v in (xyz, x32, cnt, *t.values()):   # default-stream fills, right before the call
            v.fill_(7)
        bhrt_lib.kerr_paths_device(d_rays.data_ptr(), n, bh, dk, cfg, P, 8, _flags(spin),
                                   abi.Paths(xyz.data_ptr(), x32.data_ptr(), cnt.data_ptr()),
                                   bhrt_lib.soa_from_tensors(t), None, None)
        got = {"xyz": xyz.cpu().numpy(), "xyz32": x32.cpu().numpy(), "count": cnt.cpu().numpy(),
               **{f: v.cpu().numpy() for f, v in t.items()}}   # default-stream copies after it
        for k in ref:
            assert np.array_equal(got[k], ref[k]), k


# 10. the host form --------------------------------------------------------------------------------
@pytest.mark.parametrize("which,spin,disk", [SETS[2], SETS[3]], ids=[IDS[2], IDS[3]])
def test_host_form_equals_the_device_form(bhrt_lib, which, spin, disk):
    bh, dk, cfg = kr.scene(spin, disk)
    rays = _rays(which)
    for P, every in ((P_FULL, 1), (16, 8), (3, 1)):   # ragged rows; short rows; every row full
        dev = _run(bhrt_lib, rays, spin, disk, P=P, every=every, hits=RECORDS, diag=True)
        host = bhrt_lib.kerr_paths(rays, bh, dk, cfg, max_positions=P, every=every,
                                   flags=_flags(spin), fill=FILL, fields=RECORDS, diag=True)
        assert np.array_equal(host["xyz"], dev["xyz"]) and np.array_equal(host["count"], dev["count"])
        h32 = bhrt_lib.kerr_paths(rays, bh, dk, cfg, max_positions=P, every=every, f32=True,
                                  fill=FILL, fields=())
        assert np.array_equal(h32["xyz"], dev["xyz32"]) and np.array_equal(h32["count"], dev["count"])
        # sky_* elements the kernel does not write keep what the host arrays held (0), the device
        # arrays their fill
        md = dev["result"] == kr.MAX_DISTANCE
        for f in RECORDS + ("h_residual", "lz_drift"):
            want = np.where(md, dev[f], 0.0) if f.startswith("sky_") else dev[f]
            assert np.array_equal(host[f], want, equal_nan=True), (P, every, f)
        if P == 3:
            assert (dev["count"] == 3).all()
