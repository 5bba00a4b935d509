"""The trace kernel on scenes off the five baseline configurations (tests/sweep_scenes.py).

The baseline fixes mass 1, spin 0 / 0.9 / 0.99, dt 0.1, distance 100, disk (ISCO, 20), tol 1e-6 /
1e-8, and the host (scene.c bhrt_fill_scene / bhrt_fill_origin) derives the step-size intervals, the
far-field switch, the bounded-state and no-evict proofs, the rotation bound, the accept-all
switch and the sqrt-free disk bounds from exactly those. The sweep moves each of them: 41 scenes,
70 camera frames of 48x27 and the 181 edge rays of rays_rk4_disk.npz in every scene.

CPU: the oracle equals the compiled reference on the sweep (fixtures sweep_*.npz), and the
sweep's inputs are decisive (no knife-edge ray that would excuse a GPU mismatch).
GPU: every frame and ray array against the oracle, integers exact, floats 1e-5, no exception
for any ray the oracle does not mark knife-edge; the A/B switches stay bit-identical.
"""
import ctypes as C
import functools
import glob
import os

import numpy as np
import pytest

import sweep_scenes as sw
from conftest import (FLOAT_FIELDS, GOLDEN, KNIFE_EDGE, SKY_FIELDS, compare, full_frame_report,
                      golden, rays_from, sky_pinned)
from bhrt import abi, configs

RTOL = 1e-5
REF_RTOL = 1e-12
THREADS = 16
N = sw.W * sw.H
HAND_RAYS = 21  # rays 0..20 of the edge-ray set are hand-written round-number rays
gpu = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _edge_rays():
    rays = rays_from(golden("rays_rk4_disk"))
    assert len(rays) == 181
    return rays


@functools.lru_cache(maxsize=None)
def _ray_fixtures():
    out = {}
    for p in sorted(glob.glob(os.path.join(GOLDEN, "sweep_rays_*.npz"))):
        with np.load(p, allow_pickle=False) as z:
            for k in z.files:
                name, f = k.split(".")
                out.setdefault(name, {})[f] = z[k]
    return out


_cache = {}


def _oracle_frame(oracle, name, cam):
    """(outputs, margin) of the oracle for one sweep frame; computed once, never modified."""
    key = ("frame", name, cam)
    if key not in _cache:
        bh, dk, cfg, method, flags, _ = sw.scene(name)
        _cache[key] = oracle.render_frame_margin(bh, dk, cfg, sw.camera(cam), sw.W, sw.H, method,
                                                 flags, threads=THREADS)
    return _cache[key]


def _oracle_rays(oracle, name):
    key = ("rays", name)
    if key not in _cache:
        bh, dk, cfg, method, flags, _ = sw.scene(name)
        _cache[key] = oracle.trace_rays_margin(_edge_rays(), bh, dk, cfg, method, flags,
                                               threads=THREADS)
    return _cache[key]


# --------------------------------------------------------------------------------- CPU ---

def test_sweep_table_shape():
    assert len(sw.SCENES) == 41 and len(sw.FRAMES) == 70
    assert set(sw.FRAME_FIXTURES) <= set(sw.SCENES)
    for name in sw.FRAME_FIXTURES:
        assert sw.fixture_camera(name) in sw.SCENES[name][9]
    for name, row in sw.SCENES.items():
        assert set(row[9]) <= set(sw.CAMERAS), name
    # a = spin * mass; the disk's "isco" is the black hole's
    bh, dk, cfg, method, flags, cams = sw.scene("m24_kerr_rk4")
    assert (bh.mass, bh.spin, dk.inner_radius, dk.outer_radius) == (2.4, 0.9, bh.isco_radius, 40.0)
    assert (cfg.max_ray_distance, flags, cams) == (150.0, abi.BHRT_FLAG_DOPPLER, ("B", "W", "S"))
    assert sw.scene("tol_below")[2].tolerance < 2.0**-30 == sw.scene("tol_2m30")[2].tolerance
    assert np.nextafter(sw.scene("tol_below")[2].tolerance, 1.0) == 2.0**-30


def test_ray_margin_driver_changes_no_value(oracle):
    """orc_trace_rays_margin: the outputs of orc_trace_rays bit for bit, and for rays that share
    a camera's origin the margins of orc_render_frame_margin's rays of the same direction."""
    for name in ("m24_rkf", "disk_neg", "tol_nan_kerr"):
        bh, dk, cfg, method, flags, _ = sw.scene(name)
        a = oracle.trace_rays(_edge_rays(), bh, dk, cfg, method, flags, threads=4)
        b, m = _oracle_rays(oracle, name)
        for f in a:
            assert np.array_equal(a[f], b[f], equal_nan=True), (name, f)
        assert m.shape == (181,)
    # oracle.c's camera directions through the ray-array driver: same margins as the frame's
    O = oracle.lib
    bh, dk, cfg, method, flags, _ = sw.scene("m24_rk4")
    cam = sw.camera("N")
    rays = np.zeros(N, dtype=abi.RAY_DTYPE)
    d = abi.Vector3D()
    O.orc_camera_ray_direction.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                                           C.c_int, C.POINTER(abi.Camera),
                                           C.POINTER(abi.Vector3D)]
    for i in range(N):
        O.orc_camera_ray_direction(i % sw.W, i // sw.W, 0.5, 0.5, sw.W, sw.H, C.byref(cam),
                                   C.byref(d))
        rays[i]["origin"] = (cam.position.x, cam.position.y, cam.position.z)
        rays[i]["direction"] = (d.x, d.y, d.z)
    fr, fm = _oracle_frame(oracle, "m24_rk4", "N")
    rr, rm = oracle.trace_rays_margin(rays, bh, dk, cfg, method, flags, threads=4)
    for f in fr:
        assert np.array_equal(fr[f], rr[f], equal_nan=True), f
    assert np.array_equal(fm, rm, equal_nan=True)


@pytest.mark.parametrize("name", list(sw.SCENES))
def test_oracle_sweep_vs_reference(oracle, name):
    """The oracle against the compiled reference's recorded outputs (gen_golden.py sweep):
    integers exact, floats rtol 1e-12 -- the 181 edge rays of every scene, and one 48x27 frame
    of the FRAME_FIXTURES scenes."""
    bh, dk, cfg, method, flags, _ = sw.scene(name)
    want = _ray_fixtures()[name]
    assert want["result"].dtype == np.int32 and len(want["result"]) == 181
    got, _ = _oracle_rays(oracle, name)
    compare(got, want, REF_RTOL, sky_pinned(method), name + " rays")
    if name in sw.FRAME_FIXTURES:
        cam = sw.fixture_camera(name)
        want = golden("sweep_frame_" + name)
        got, _ = _oracle_frame(oracle, name, cam)
        compare(got, want, REF_RTOL, sky_pinned(method), f"{name}/{cam} frame")


# the 14 frames of the grid on which the oracle ends every ray in the same class
SINGLE_CLASS_FRAMES = {
    ("m05_kerr_rkf", "B"), ("m05_kerr_rkf", "N"), ("a0998_rkf", "B"), ("a0998_rkf", "S"),
    ("tol_0_kerr", "B"), ("tol_nan_kerr", "B"), ("tol_1e301", "B"), ("dist_inf", "B"),
    ("disk_swapped", "B"), ("disk_nan", "B"), ("disk_all", "B"), ("disk_all", "E"),
    ("disk_wide", "B"), ("disk_wide", "W"),
}
# what integrate_photon_path / trace_ray can return for non-NULL arguments (oracle.c)
REACHABLE_CLASSES = {abi.RAY_HORIZON, abi.RAY_DISK, abi.RAY_MAX_DISTANCE, abi.RAY_MAX_STEPS}


def test_sweep_inputs_are_decisive(oracle):
    """Guards the GPU tests against excusing failures (oracle only): no frame of the sweep has a
    knife-edge ray or a NaN margin, so full_frame_report can excuse nothing there; of the edge
    rays only the 21 hand-written ones may be knife-edge; every class the reference can return
    appears, and every frame but the listed single-class ones has at least two."""
    seen = set()
    for name, cam in sw.FRAMES:
        out, margin = _oracle_frame(oracle, name, cam)
        assert len(margin) == N
        assert not np.isnan(margin).any(), (name, cam)
        assert int((margin < KNIFE_EDGE).sum()) == 0, (name, cam, float(margin.min()))
        classes = set(np.unique(out["result"]).tolist())
        seen |= classes
        if (name, cam) in SINGLE_CLASS_FRAMES:
            assert len(classes) == 1, (name, cam, classes)
        else:
            assert len(classes) >= 2, (name, cam, classes)
    for name in sw.SCENES:
        out, margin = _oracle_rays(oracle, name)
        m = margin[HAND_RAYS:]
        assert (m >= KNIFE_EDGE).all(), (name, HAND_RAYS + np.nonzero(~(m >= KNIFE_EDGE))[0])
        seen |= set(np.unique(out["result"]).tolist())
    assert seen == REACHABLE_CLASSES, seen


# --------------------------------------------------------------------------------- GPU ---

def _display_u8(v):
    """(unsigned char)(std::min(1.0f, v) * 255.0f), the visualizer's conversion, on x86."""
    v = v.astype(np.float32)
    m = np.where(v < np.float32(1.0), v, np.float32(1.0)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        return (np.trunc(m * np.float32(255.0)).astype(np.int64) & 0xFF).astype(np.uint8)


def _checked_stats(bhrt_lib, n):
    """The launch's counters; bhrt_get_stats fails ("lost redo rays") if a launch whose redo
    pass the host proved unnecessary handed a ray over: a wrong no-evict proof."""
    st = bhrt_lib.stats(reset=True)
    assert st["rays"] == n, st
    return st


def _assert_same_infinities(got, want, check_sky, rays):
    """full_frame_report's relative error of an infinite value is NaN, which violates nothing:
    infinities must sit at the same places with the same sign (on the selected rays)."""
    for f in FLOAT_FIELDS + (SKY_FIELDS if check_sky else ()):
        a, b = np.asarray(got[f])[rays], np.asarray(want[f])[rays]
        inf = np.isinf(a) | np.isinf(b)
        assert np.array_equal(a[inf], b[inf]), (f, np.nonzero(inf)[0][:10])


def _print_errors(tag, got, want, check_sky, margin):
    """The measured error of one sweep case (information for DESIGN.md section 5, no threshold):
    the worst relative error over the float values of magnitude >= 1e-4, where the contract's
    relative bound 1e-5 is the binding one, and the worst absolute difference over the smaller
    ones, where its absolute floor 1e-9 is."""
    rel, small = (0.0, "-"), (0.0, "-")
    for f in FLOAT_FIELDS + (SKY_FIELDS if check_sky else ()):
        a, b = np.asarray(got[f]), np.asarray(want[f])
        ok = ~(np.isnan(a) | np.isnan(b)) & ~(np.isinf(a) & (a == b))
        diff, scale = np.abs(a[ok] - b[ok]), np.maximum(np.abs(a[ok]), np.abs(b[ok]))
        big = scale >= 1e-4
        if big.any():
            rel = max(rel, (float((diff[big] / scale[big]).max()), f))
        if (~big).any():
            small = max(small, (float(diff[~big].max()), f))
    print(f"SWEEP_ERR {tag} rel {rel[0]:.3e} {rel[1]} abs_below_1e-4 {small[0]:.3e} {small[1]} "
          f"min_margin {float(np.nanmin(margin)):.3e}")


@gpu
@pytest.mark.parametrize("name,cam", sw.FRAMES, ids=[f"{n}-{c}" for n, c in sw.FRAMES])
def test_sweep_frames_vs_oracle(bhrt_lib, oracle, name, cam):
    """Every ray of every sweep frame against the oracle. test_sweep_inputs_are_decisive
    guarantees that no ray of these frames is knife-edge, so every ray must match."""
    bh, dk, cfg, method, flags, _ = sw.scene(name)
    bhrt_lib.stats(reset=True)
    got = bhrt_lib.render_frame(bh, dk, cfg, sw.camera(cam), sw.W, sw.H, method, flags,
                                fields=abi.SOA_FIELDS + abi.DISPLAY_FIELDS)
    _checked_stats(bhrt_lib, N)
    want, margin = _oracle_frame(oracle, name, cam)
    rep = full_frame_report(got, want, margin, sky_pinned(method), rtol=RTOL)
    _print_errors(f"frame {name} {cam}", got, want, sky_pinned(method), margin)
    _assert_same_infinities(got, want, sky_pinned(method), np.ones(N, dtype=bool))
    assert rep["rays"] == N
    assert rep["unexplained"] == 0, rep
    assert rep["mismatched_rays"] == 0, rep
    # the display path, as test_display_path_rgba checks it
    rgb = np.stack([got["rgb_r"], got["rgb_g"], got["rgb_b"]], axis=1)
    f32 = got["rgba32f"]
    assert np.array_equal(f32[:, :3], rgb.astype(np.float32), equal_nan=True)
    assert (f32[:, 3] == 1.0).all()
    assert np.array_equal(got["rgba8"], _display_u8(f32))


@gpu
@pytest.mark.parametrize("name", list(sw.SCENES))
def test_sweep_rays_vs_oracle(bhrt_lib, oracle, name):
    """The 181 edge rays through bhrt_trace_rays (the per-ray set-up, not fill_origin). The 160
    random rays (index >= 21) must match without exception; a hand-written ray may differ only
    where the oracle's margin is below KNIFE_EDGE."""
    bh, dk, cfg, method, flags, _ = sw.scene(name)
    rays = _edge_rays()
    bhrt_lib.stats(reset=True)
    got = bhrt_lib.trace_rays(rays, bh, dk, cfg, method, flags)
    _checked_stats(bhrt_lib, len(rays))
    want, margin = _oracle_rays(oracle, name)
    sky = sky_pinned(method)

    def part(lo, hi):
        return full_frame_report({f: v[lo:hi] for f, v in got.items()},
                                 {f: v[lo:hi] for f, v in want.items()}, margin[lo:hi], sky,
                                 rtol=RTOL)

    rep = part(HAND_RAYS, len(rays))
    _print_errors(f"rays {name}", {f: v[HAND_RAYS:] for f, v in got.items()},
                  {f: v[HAND_RAYS:] for f, v in want.items()}, sky, margin[HAND_RAYS:])
    _assert_same_infinities(got, want, sky, ~(margin < KNIFE_EDGE))
    assert rep["mismatched_rays"] == 0 and rep["knife_edge_rays"] == 0, rep
    hand = part(0, HAND_RAYS)
    differ = [i for i in range(HAND_RAYS) if part(i, i + 1)["mismatched_rays"]]
    print(f"SWEEP_KNIFE rays {name} knife-edge {hand['knife_edge_ids']} differ {differ}")
    assert hand["unexplained"] == 0, hand


@gpu
@pytest.mark.parametrize("name", sw.FRAME_FIXTURES)
def test_sweep_shared_origin_rays(bhrt_lib, oracle, name):
    """A camera's rays passed as Ray[] (set up in the trace kernel from the host's origin block,
    kparams.rays_shared) against the oracle's trace of the same array, every ray."""
    bh, dk, cfg, method, flags, _ = sw.scene(name)
    rays = configs.camera_rays(sw.camera(sw.fixture_camera(name)), sw.W, sw.H)
    want = oracle.trace_rays(rays, bh, dk, cfg, method, flags, threads=THREADS)
    bhrt_lib.stats(reset=True)
    got = bhrt_lib.trace_rays(rays, bh, dk, cfg, method, flags)
    _checked_stats(bhrt_lib, N)
    compare(got, want, RTOL, sky_pinned(method), f"{name} shared origin")


SWITCH_SCENES = ("m24_rkf", "m05_kerr_rkf", "a05_rkf_disk", "dt7_kerr_rkf", "tol_2m30",
                 "tol_below", "disk_neg", "m1e3")


@gpu
@pytest.mark.parametrize("switch", ["BHRT_ACCEPT_ALL", "BHRT_SKIP_REDO", "BHRT_FUSE_COLOUR"])
@pytest.mark.parametrize("name", SWITCH_SCENES)
def test_sweep_switches_are_bit_identical(bhrt_lib, monkeypatch, name, switch):
    """The A/B switches (accept test kept, redo launch kept, colour in a pass of its own) give
    every output field of the default run bit for bit, off the baseline too (camera B)."""
    bh, dk, cfg, method, flags, _ = sw.scene(name)
    cam = sw.camera("B")
    fields = abi.SOA_FIELDS + abi.DISPLAY_FIELDS
    bhrt_lib.stats(reset=True)
    base = bhrt_lib.render_frame(bh, dk, cfg, cam, sw.W, sw.H, method, flags, fields=fields)
    _checked_stats(bhrt_lib, N)
    monkeypatch.setenv(switch, "0")
    other = bhrt_lib.render_frame(bh, dk, cfg, cam, sw.W, sw.H, method, flags, fields=fields)
    _checked_stats(bhrt_lib, N)
    for f in fields:
        assert np.array_equal(other[f], base[f], equal_nan=True), (switch, f)


@gpu
@pytest.mark.parametrize("name", ["tol_2m30", "tol_below"])
def test_sweep_accept_all_threshold(bhrt_lib, name):
    """fill_scene's accept_all threshold from both sides: tol = 2^-30 runs attempts without the
    accept test (the zero-acceleration Kerr path of camera B's frame), one ulp below runs none."""
    bh, dk, cfg, method, flags, _ = sw.scene(name)
    bhrt_lib.stats(reset=True)
    bhrt_lib.render_frame(bh, dk, cfg, sw.camera("B"), sw.W, sw.H, method, flags)
    st = _checked_stats(bhrt_lib, N)
    assert st["iterations"] > 0, st
    if name == "tol_2m30":
        assert st["attempts_untested"] > 0, st
    else:
        assert st["attempts_untested"] == 0, st
