"""Batched photon paths on the GPU (bhrt_trace_paths_device / bhrt_trace_paths, paths.hip
k_paths) against the compiled reference's fixture (tests/golden/path_batch.npz) and, for shapes
beyond it, the oracle's orc_integrate_photon_path / orc_trace_ray_method, both through the rule
functions of tests/test_paths_cpu.py.

Tolerances are the project's own (test_gpu_parity.test_paths_vs_reference): count, result and
steps exact; points and hit floats rtol 1e-5 with atol 1e-9. No ray is exempt: the fixture holds
no knife-edge ray, and the camera crop's rays are checked against KNIFE_EDGE here."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import KNIFE_EDGE
from bhrt import abi, configs
from test_paths_cpu import (build_paths_demo, fixture_scenes, oracle_paths, scene_paths,
                            stored_points)

pytestmark = pytest.mark.gpu
RTOL, ATOL = 1e-5, 1e-9
SENT, SENT32, SENTI = 7.0e77, np.float32(7.0e37), -7
BIG = 100000  # an `every` larger than any path
ALL = ("xyz", "xyz32", "count")
NAMES = ["rk4_disk", "rkf45_disk_stuck", "rk4_kerr_disk", "rkf45_kerr099", "steps0", "leapfrog"]


@functools.lru_cache(maxsize=None)
def scenes():
    return {s["name"]: s for s in fixture_scenes()}


@functools.lru_cache(maxsize=None)
def fixture_paths(name):
    return scene_paths(scenes()[name])


@functools.lru_cache(maxsize=None)
def crop():
    """The camera-B rays of a 40 x 25 pixel crop of C2's frame, C2's scene, and the oracle's
    paths of those rays. The crop straddles column 1248, where trace_ray's disk test stops
    hitting on the first segments: the left half of every row ends after 1-2 iterations, the
    right half runs to the step budget, so every wave holds both."""
    import oracle as orc
    c = configs.CONFIGS["C2"]
    bh, dk, cfg = c.scene()
    rays = configs.camera_rays(configs.camera("B"), c.width, c.height).reshape(c.height, c.width)
    rays = np.ascontiguousarray(rays[500:525, 1228:1268]).reshape(-1)
    o = orc.oracle()
    _, margin = o.trace_rays_margin(rays, bh, dk, cfg, c.method)
    assert (margin >= KNIFE_EDGE).all(), np.nonzero(margin < KNIFE_EDGE)[0]
    return rays, bh, dk, cfg, c.method, oracle_paths(o, rays, bh, dk, cfg, c.method)


def run_device(lib, rays, bh, dk, cfg, method, P, every, outputs=ALL, hits=True, stream=None):
    """One bhrt_trace_paths_device call into sentinel-filled device arrays (filled on the default
    stream, no synchronisation before the call); returns the host copies."""
    import torch
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8)).cuda()
    t = {"xyz": torch.full((n, P, 3), SENT, dtype=torch.float64, device="cuda"),
         "xyz32": torch.full((n, P, 3), float(SENT32), dtype=torch.float32, device="cuda"),
         "count": torch.full((n,), SENTI, dtype=torch.int32, device="cuda")}
    h = {f: torch.full((n,), SENTI, dtype=torch.int32 if f in ("result", "steps")
                       else torch.float64, device="cuda") for f in abi.PATH_HIT_FIELDS}
    paths = abi.Paths(**{f: t[f].data_ptr() for f in outputs})
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    lib.trace_paths_device(d_rays.data_ptr(), n, bh, dk, cfg, method, P, every, paths,
                           lib.soa_from_tensors(h) if hits else None,
                           stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    got = {f: v.cpu().numpy() for f, v in t.items()}  # (default-stream copies: no sync before)
    got.update({f: v.cpu().numpy() for f, v in h.items()})
    return got


def check_paths(got, want_paths, every, P, outputs=ALL, what=""):
    """Counts exact, stored points within tolerance, xyz32 == float32(xyz) exactly, every element
    beyond count[i] (and every array not asked for) still the sentinel."""
    n = len(want_paths)
    for f in ALL:
        if f not in outputs:
            sent = {"xyz": SENT, "xyz32": SENT32, "count": SENTI}[f]
            assert (got[f] == sent).all(), (what, f, "written though not asked for")
    for i in range(n):
        want = stored_points(want_paths[i], every, P)
        cnt = len(want)
        if "count" in outputs:
            assert got["count"][i] == cnt, (what, i, int(got["count"][i]), cnt)
        if "xyz" in outputs:
            np.testing.assert_allclose(got["xyz"][i, :cnt], want, rtol=RTOL, atol=ATOL,
                                       err_msg=f"{what} ray {i}")
            assert (got["xyz"][i, cnt:] == SENT).all(), (what, i, "xyz tail written")
        if "xyz32" in outputs:
            if "xyz" in outputs:
                assert np.array_equal(got["xyz32"][i, :cnt], np.float32(got["xyz"][i, :cnt])), (what, i)
            else:
                np.testing.assert_allclose(got["xyz32"][i, :cnt], want, rtol=RTOL, atol=ATOL,
                                           err_msg=f"{what} ray {i}")
            assert (got["xyz32"][i, cnt:] == SENT32).all(), (what, i, "xyz32 tail written")


def check_hits(got, trace, what=""):
    for f in ("result", "steps"):
        assert np.array_equal(got[f], trace[f]), (what, f, got[f], trace[f])
    for f in ("hit_x", "hit_y", "hit_z", "distance", "time_dilation"):
        np.testing.assert_allclose(got[f], trace[f], rtol=RTOL, atol=ATOL, err_msg=f"{what} {f}")


def scene_args(s):
    return s["rays"], s["bh"], s["dk"], s["cfg"], s["method"]


@pytest.mark.parametrize("name", NAMES)
def test_fixture_scenes(bhrt_lib, name):
    """Every fixture ray against the compiled reference: positions P in {1, 2, 7, longer than any
    path} and decimations in {1, 3, 8, larger than any path} (8 = the staged form's ring, so a
    flush boundary coincides with a kept point), with the hits where the reference has them."""
    s = scenes()[name]
    want = fixture_paths(name)
    longer = s["cfg"].max_integration_steps + 5
    for every, P in ((1, longer), (3, longer), (8, longer), (BIG, longer), (1, 1), (1, 2), (1, 7),
                     (3, 7), (8, 2), (BIG, 1)):
        got = run_device(bhrt_lib, *scene_args(s), P, every)
        check_paths(got, want, every, P, what=f"{name} every {every} P {P}")
        if s["trace"] is not None:
            check_hits(got, s["trace"], name)
        else:  # integrate_photon_path's own hit
            assert np.array_equal(got["result"], s["res"][:, 2]), name
            assert np.array_equal(got["steps"], s["res"][:, 3]), name
            for k, f in enumerate(("hit_x", "hit_y", "hit_z", "distance", "time_dilation")):
                np.testing.assert_allclose(got[f], s["hit"][:, k], rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 1000])
def test_ray_counts(bhrt_lib, n):
    """A lone lane, partial waves, more rays than one claim and (1000) a grid of several waves
    claiming in turn, with path lengths from 2 points to the step budget inside every wave; the launch is
    counted like a trace launch."""
    rays, bh, dk, cfg, method, want = crop()
    lens = np.array([len(q) for q in want])
    assert lens.min() <= 3 and lens.max() == cfg.max_integration_steps + 1, (lens.min(), lens.max())
    P = cfg.max_integration_steps + 1
    bhrt_lib.stats(reset=True)
    got = run_device(bhrt_lib, rays[:n], bh, dk, cfg, method, P, 1, hits=False)
    st = bhrt_lib.stats(reset=True)
    check_paths(got, want[:n], 1, P, what=f"n {n}")
    assert st["launches"] == 1 and st["rays"] == n, st
    assert st["iterations"] == int((lens[:n] - 1).sum()), st  # RK4: one point per iteration
    run_device(bhrt_lib, rays[:n], bh, dk, cfg, method, 2, 1)   # with the hits: their trace
    st = bhrt_lib.stats(reset=True)                            # launch is counted too
    assert st["launches"] == 2 and st["rays"] == 2 * n, st
    got = run_device(bhrt_lib, rays[:n], bh, dk, cfg, method, 40, 8)
    check_paths(got, want[:n], 8, 40, what=f"n {n} every 8 P 40")


@pytest.mark.parametrize("every", [1, 3])
def test_fixed_point(bhrt_lib, every):
    """Stuck RKF45 rays (the repeated point is stored for every iteration jumped over) in more
    than one wave, beside rays of other lengths: full and truncated."""
    s = scenes()["rkf45_disk_stuck"]
    want = fixture_paths("rkf45_disk_stuck")
    reps = 7  # 70 rays
    rays = np.tile(s["rays"], reps)
    for P in (s["cfg"].max_integration_steps + 1, 7, 9):
        got = run_device(bhrt_lib, rays, s["bh"], s["dk"], s["cfg"], s["method"], P, every)
        check_paths(got, want * reps, every, P, what=f"stuck every {every} P {P}")


@pytest.mark.parametrize("outputs,hits", [(("xyz",), True), (("xyz32",), True), (("count",), True),
                                          (ALL, True), (ALL, False), (("xyz", "count"), False)])
def test_output_combinations(bhrt_lib, outputs, hits):
    s = scenes()["rk4_kerr_disk"]
    want = fixture_paths("rk4_kerr_disk")
    for every, P in ((1, 200), (3, 11)):
        got = run_device(bhrt_lib, *scene_args(s), P, every, outputs=outputs, hits=hits)
        check_paths(got, want, every, P, outputs, what=f"{outputs} hits {hits}")
        if hits:
            check_hits(got, s["trace"], str(outputs))
        else:
            for f in abi.PATH_HIT_FIELDS:
                assert (got[f] == SENTI).all(), (f, "written though hits was NULL")


def _trace_rays_device(lib, rays, bh, dk, cfg, method):
    import torch
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8)).cuda()
    h = {f: torch.full((n,), SENTI, dtype=torch.int32 if f in ("result", "steps")
                       else torch.float64, device="cuda") for f in abi.PATH_HIT_FIELDS}
    L = lib.load()
    assert L.bhrt_trace_rays_device(d_rays.data_ptr(), n, C.byref(bh), C.byref(dk) if dk else None,
                                    C.byref(cfg), method, 0, C.byref(lib.soa_from_tensors(h)),
                                    None) == 0, lib.last_error()
    return {f: v.cpu().numpy() for f, v in h.items()}


@pytest.mark.parametrize("name", NAMES + ["crop"])
def test_hits_equal_trace_rays_device(bhrt_lib, name):
    """The hit fields are bhrt_trace_rays_device's for the same rays, bit for bit."""
    args = crop()[:5] if name == "crop" else scene_args(scenes()[name])
    want = _trace_rays_device(bhrt_lib, *args)
    for every, P in ((1, 1001), (8, 3)):
        got = run_device(bhrt_lib, *args, P, every)
        for f in abi.PATH_HIT_FIELDS:
            assert np.array_equal(got[f], want[f], equal_nan=f not in ("result", "steps")), (name, f)


@pytest.mark.parametrize("name", ["rkf45_kerr099", "steps0", "leapfrog"])
def test_rows_equal_the_single_ray_call(bhrt_lib, name):
    """Without a disk, ray i's row is integrate_photon_path's own output, bit for bit."""
    s = scenes()[name]
    L = bhrt_lib.load()
    P = s["cfg"].max_integration_steps + 1
    got = run_device(bhrt_lib, *scene_args(s), P, 1)
    for i, ray in enumerate(s["rays"]):
        path = np.zeros((P, 3))
        num = C.c_int(0)
        hit = abi.RayTraceHit()
        o, d = [float(x) for x in ray["origin"]], [float(x) for x in ray["direction"]]
        res = L.integrate_photon_path(C.byref(abi.Vector4D(0.0, *o)), C.byref(abi.v3(*d)),
                                      C.byref(s["bh"]), C.byref(s["cfg"]), s["method"],
                                      path.ctypes.data, P, C.byref(num), C.byref(hit))
        assert (res, num.value) == (got["result"][i], got["count"][i]), (name, i)
        assert got["xyz"][i, :num.value].tobytes() == path[:num.value].tobytes(), (name, i)
        assert hit.steps == got["steps"][i], (name, i)  # (the hit floats are the trace kernel's)


def test_stream_ordering_and_determinism(bhrt_lib):
    """A NULL hip_stream is ordered like the default stream (the sentinel fills before it and
    the copies after it run there, with no synchronisation: run_device); an explicit stream and
    a second run give the same bytes."""
    import torch
    assert torch.cuda.current_stream().cuda_stream == 0  # (torch's default = the null stream)
    rays, bh, dk, cfg, method, want = crop()
    P = cfg.max_integration_steps + 1
    a = run_device(bhrt_lib, rays, bh, dk, cfg, method, P, 1)
    check_paths(a, want, 1, P, what="NULL stream")
    b = run_device(bhrt_lib, rays, bh, dk, cfg, method, P, 1, stream=torch.cuda.Stream())
    c = run_device(bhrt_lib, rays, bh, dk, cfg, method, P, 1)
    for f in a:
        assert a[f].tobytes() == b[f].tobytes(), ("explicit stream", f)
        assert a[f].tobytes() == c[f].tobytes(), ("second run", f)


def test_store_forms_agree(bhrt_lib, monkeypatch):
    """The direct and the staged store form (BHRT_PATHS_STORE) write the same bytes."""
    rays, bh, dk, cfg, method, want = crop()
    stuck = scenes()["rkf45_disk_stuck"]
    for args, P, every in ((crop()[:5], 1001, 1), (crop()[:5], 50, 8), (crop()[:5], 9, 3),
                           (scene_args(stuck), 61, 1), (scene_args(stuck), 5, 3)):
        out = {}
        for form in ("direct", "staged"):
            monkeypatch.setenv("BHRT_PATHS_STORE", form)
            out[form] = run_device(bhrt_lib, *args, P, every)
        for f in out["direct"]:
            assert out["direct"][f].tobytes() == out["staged"][f].tobytes(), (P, every, f)
    monkeypatch.delenv("BHRT_PATHS_STORE")
    check_paths(out["staged"], fixture_paths("rkf45_disk_stuck"), 3, 5, what="staged")


def test_host_form(bhrt_lib):
    """bhrt_trace_paths (host arrays) through the Python binding: the device form's bytes, and
    NaN-filled tails left alone; float32 on request."""
    rays, bh, dk, cfg, method, want = crop()
    n = 130
    dev = run_device(bhrt_lib, rays[:n], bh, dk, cfg, method, 300, 4)
    got = bhrt_lib.trace_paths(rays[:n], bh, dk, cfg, method, max_positions=300, every=4)
    assert np.array_equal(got["count"], dev["count"])
    for i in range(n):
        c = got["count"][i]
        assert got["xyz"][i, :c].tobytes() == dev["xyz"][i, :c].tobytes(), i
        assert np.isnan(got["xyz"][i, c:]).all(), i
    for f in abi.PATH_HIT_FIELDS:
        assert np.array_equal(got[f], dev[f], equal_nan=f not in ("result", "steps")), f
    g32 = bhrt_lib.trace_paths(rays[:n], bh, dk, cfg, method, max_positions=300, every=4, f32=True)
    assert g32["xyz"].dtype == np.float32
    for i in range(n):
        c = g32["count"][i]
        assert np.array_equal(g32["xyz"][i, :c], np.float32(got["xyz"][i, :c])), i
        assert np.isnan(g32["xyz"][i, c:]).all(), i


def test_device_refusals(bhrt_lib):
    """The error list once more on a machine with a device: -1 and nothing written."""
    import torch
    s = scenes()["rk4_disk"]
    n = len(s["rays"])
    d_rays = torch.from_numpy(s["rays"].view(np.uint8)).cuda()
    xyz = torch.full((n, 4, 3), SENT, dtype=torch.float64, device="cuda")
    rgb = torch.full((n,), SENT, dtype=torch.float64, device="cuda")
    ok = abi.Paths(xyz=xyz.data_ptr())
    L = bhrt_lib.load()
    call = lambda rp, nn, P, e, paths, hits: L.bhrt_trace_paths_device(
        rp, nn, C.byref(s["bh"]), C.byref(s["dk"]), C.byref(s["cfg"]), s["method"], P, e,
        C.byref(paths) if paths else None, C.byref(hits) if hits else None, None)
    for args in ((d_rays.data_ptr(), 0, 4, 1, ok, None), (None, n, 4, 1, ok, None),
                 (d_rays.data_ptr(), n, 0, 1, ok, None), (d_rays.data_ptr(), n, 65537, 1, ok, None),
                 (d_rays.data_ptr(), n, 4, 0, ok, None), (d_rays.data_ptr(), n, 4, 1, abi.Paths(), None),
                 (d_rays.data_ptr(), n, 4, 1, None, None),
                 (d_rays.data_ptr(), n, 4, 1, ok, abi.FrameSoA(rgb_r=rgb.data_ptr(),
                                                               rgb_g=rgb.data_ptr(),
                                                               rgb_b=rgb.data_ptr()))):
        assert call(*args) == -1, args
        assert bhrt_lib.last_error().startswith("paths:"), bhrt_lib.last_error()
    torch.cuda.synchronize()
    assert (xyz == SENT).all().item() and (rgb == SENT).all().item()
    assert call(d_rays.data_ptr(), n, 4, 1, ok, None) == 0, bhrt_lib.last_error()


def test_paths_demo_writes_a_fan_of_polylines(bhrt_lib, tmp_path):
    """examples/paths_demo.c end to end: 41 polylines from (0, -30, 0), each starting at the
    origin, as many points per ray as the program reports."""
    import subprocess
    r = subprocess.run([build_paths_demo(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "ray,point,x,y,z"
    rows = np.array([[float(v) for v in l.split(",")] for l in lines[1:]])
    assert set(rows[:, 0].astype(int)) == set(range(41))
    first = rows[rows[:, 1] == 0]
    np.testing.assert_allclose(first[:, 2:], np.tile([0.0, -30.0, 0.0], (41, 1)), atol=1e-12)
    assert np.isfinite(rows).all()
    import re
    said = {int(i): int(k) for i, k in re.findall(r"ray (\d+): class \d, (\d+) points", r.stderr)}
    assert len(said) == 41, r.stderr
    for i, k in said.items():  # every 4th point of at most 1001, and the last: 252 at the most
        assert 2 <= k <= 252 and int((rows[:, 0] == i).sum()) == k, (i, k)
