"""Adaptive physical geodesics on the GPU (bhrt_kerr_rk45_*; kerr.hip k_kerr_rk45) against the
numpy rule (tests/kerr_rk45_rule.py; stated in include/bhrt_api.h "Physical geodesics, adaptive
steps").

Frames: test_gpu_kerr.py's -- 48x27 and 49x27, camera at (0, -18, 4), first trial step 0.25, max
distance 60, 2000 attempts, M = 1, three (spin, disk) scenes -- all six at tolerance 1e-8 and the
two spin-0.9 ones at 1e-6. Class, attempts and rejected attempts must equal the rule's on every
ray outside the rule's knife-edge set (rays whose class, attempts or rejected count changes under
a +-1e-7 direction perturbation; at most 1% of a frame, and none here: test_kerr_rk45_cpu.py);
floats agree to the project's 1e-5 contract (conftest.compare). The kernel contracts products
into FMAs, differences of a few 1e-16 per operation; they enter err relative to the tolerance,
1e-8 of h at tolerance 1e-8, which is why no tolerance tighter than 1e-8 is compared here.

The worst observed ratios go to profiles/kerr_rk45/test_figures.txt."""
import os

import numpy as np
import pytest

from conftest import ROOT, compare
from bhrt import abi
import kerr_rule as kr
import kerr_rk45_rule as k5
import sky_rule as sr

pytestmark = pytest.mark.gpu
FIGURES = os.path.join(ROOT, "profiles", "kerr_rk45", "test_figures.txt")
RGB = ("rgb_r", "rgb_g", "rgb_b")
HITS = ("result", "steps", "hit_x", "hit_y", "hit_z", "distance", "sky_x", "sky_y", "sky_z")
ALL = HITS + RGB + ("rgba32f", "rgba8")
DIAG = ("h_residual", "lz_drift", "rejected")
EPS = 1e-5
KNIFE_CAP = 0.01
RK4_H_RESIDUAL = 4.8e-5     # the RK4 frames' worst (test_kerr_cpu.py)
FRAMES = [(spin, disk, W, H) for spin, disk in kr.SCENES for W, H in kr.FRAME_SIZES]
CASES = [f + (1e-8,) for f in FRAMES] + [f + (1e-6,) for f in FRAMES[4:]]
IDS = [f"spin{spin}-{W}x{H}-tol{tol:g}" for spin, _, W, H, tol in CASES]


def _figure(key, text):
    """One line per key in profiles/kerr_rk45/test_figures.txt, rewritten in place."""
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


def _tensors(n, fields, fill=7, diag=False):
    import torch
    dt = {"result": torch.int32, "steps": torch.int32, "rgba32f": torch.float32,
          "rgba8": torch.uint8, "rejected": torch.int32}
    t = {f: torch.full((n, 4) if f in abi.DISPLAY_FIELDS else (n,), fill,
                       dtype=dt.get(f, torch.float64), device="cuda") for f in fields}
    d = {f: torch.full((n,), fill, dtype=dt.get(f, torch.float64), device="cuda")
         for f in (DIAG if diag else ())}
    return t, d


def _kd(d):
    return abi.KerrRk45Diag(*(d[f].data_ptr() for f in DIAG)) if d else None


def _device_frame(lib, spin, disk, W, H, tol, rows=None, stream=None, fields=ALL, diag=True,
                  flags=None, offset=None, steps=None):
    """One bhrt_kerr_rk45_frame_device call into fresh device arrays (fill 7), as numpy arrays."""
    import torch
    bh, dk, cfg = k5.scene(spin, disk, tol)
    if steps is not None:
        cfg.max_integration_steps = steps
    cam = kr.camera()
    if offset is not None:
        cam.use_offset, cam.offset_x, cam.offset_y = 1, offset[0], offset[1]
    n = W * (H if rows is None else lib.shard_rows(H, rows))
    t, d = _tensors(n, fields, diag=diag)
    torch.cuda.synchronize()
    lib.kerr_rk45_frame_device(bh, dk, cfg, cam, W, H, rows,
                               _flags(spin) if flags is None else flags,
                               lib.soa_from_tensors(t), _kd(d), stream)
    torch.cuda.synchronize()
    out = {f: v.cpu().numpy() for f, v in t.items()}
    out.update({f: v.cpu().numpy() for f, v in d.items()})
    return out


_FRAMES = {}


def _frame(lib, case):
    """The whole device frame of a case, rendered once for the module and left unchanged."""
    if case not in _FRAMES:
        f = _device_frame(lib, *case)
        for v in f.values():
            v.setflags(write=False)
        _FRAMES[case] = f
    return _FRAMES[case]


def _same(a, b, fields, what=""):
    for f in fields:
        assert np.array_equal(a[f], b[f], equal_nan=True), (what, f)


def _rule_soa(rule, bh, dk, flags):
    """The rule's frame as SoA fields; sky_* where the kernel does not write them: the fill."""
    rgb = kr.colour(rule, bh, dk, flags)     # (reads the rule's tangent under "chord")
    md = rule["result"] == kr.MAX_DISTANCE
    want = {"result": rule["result"], "steps": rule["steps"], "rejected": rule["rejected"],
            "distance": rule["distance"]}
    for k, ax in enumerate("xyz"):
        want["hit_" + ax] = rule["hit"][:, k]
        want["sky_" + ax] = np.where(md, rule["chord"][:, k], 7.0)
        want[RGB[k]] = rgb[:, k]
    return want


# 1. frames against the rule ----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_frames_match_the_rule(bhrt_lib, case):
    spin, disk, W, H, tol = case
    name = IDS[CASES.index(case)]
    bh, dk, _ = k5.scene(spin, disk, tol)
    rule = k5.frame_rule(spin, disk, W, H, tol)
    knife = k5.knife_edge(spin, disk, W, H, tol)
    assert knife.sum() <= KNIFE_CAP * len(knife), int(knife.sum())
    got = _frame(bhrt_lib, case)
    want = _rule_soa(rule, bh, dk, _flags(spin))
    keep = ~knife
    for f in ("result", "steps", "rejected"):
        bad = np.nonzero((got[f] != want[f]) & keep)[0]
        print(f"{name}: {f} differs on {bad.size} rays outside the knife-edge set "
              f"({int(knife.sum())} in it)")
        assert bad.size == 0, (f, bad[:10], got[f][bad[:10]], want[f][bad[:10]])
    same = keep & (got["result"] == want["result"]) & (got["steps"] == want["steps"])
    fields = tuple(f for f in HITS + RGB if f not in ("result", "steps"))
    worst = max(float(np.max(np.abs(got[f][same] - want[f][same]) /
                             (EPS * np.maximum(np.abs(got[f][same]), np.abs(want[f][same])) + 1e-9)))
                for f in fields)
    counts = np.bincount(got["result"], minlength=6).tolist()
    print(f"classes {counts}, {int(got['steps'].sum())} attempts, {int(got['rejected'].sum())} "
          f"rejected, worst |diff| / tol {worst:.3e}")
    _figure(f"frame {name}",
            f"classes {counts}, attempts {int(got['steps'].sum())}, rejected "
            f"{int(got['rejected'].sum())}, longest {int(got['steps'].max())}, knife-edge "
            f"{int(knife.sum())}, worst |diff| / tol {worst:.3e}")
    compare({f: got[f][same] for f in fields}, {f: want[f][same] for f in fields}, EPS,
            check_sky=True, what=str(case), fields=fields)
    # the display fields are the frame's conversions of rgb, and horizon pixels are black
    assert np.array_equal(got["rgba32f"][:, :3], np.stack([got[c] for c in RGB], 1).astype(np.float32))
    assert (got["rgba32f"][:, 3] == 1.0).all()
    assert np.array_equal(got["rgba8"], abi.rgba8_from_rgb(*[got[c] for c in RGB]))
    assert (np.stack([got[c] for c in RGB], 1)[got["result"] == kr.HORIZON] == 0.0).all()


# 2. the diagnostics ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [CASES[1], CASES[5], CASES[7]], ids=[IDS[1], IDS[5], IDS[7]])
def test_diag_within_ten_times_the_rule(bhrt_lib, case):
    rule = k5.frame_rule(*case)
    got = _frame(bhrt_lib, case)
    for f in ("h_residual", "lz_drift"):
        g, w = float(got[f].max()), float(rule[f].max())
        print(f"{case}: {f} GPU {g:.3e}, rule {w:.3e}")
        assert np.isfinite(got[f]).all() and (got[f] >= 0.0).all()
        assert g <= 10.0 * w, (f, g, w)
        _figure(f"diag {f} {IDS[CASES.index(case)]}", f"GPU {g:.3e}, rule {w:.3e}")
    if case[4] == 1e-8:     # below the fixed-step frames' residual at their time_step 0.25
        assert float(got["h_residual"].max()) < RK4_H_RESIDUAL


# 3. bit identity ---------------------------------------------------------------------------------
def test_same_bits_run_to_run_and_on_two_streams(bhrt_lib):
    import torch
    case = CASES[5]
    first = _frame(bhrt_lib, case)
    again = _device_frame(bhrt_lib, *case)
    _same(first, again, ALL + DIAG, "run to run")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for s in (s1, s2):
        _same(first, _device_frame(bhrt_lib, *case, stream=s.cuda_stream), ALL, "stream")
    # without the diagnostics and with fewer outputs: the same rays
    few = _device_frame(bhrt_lib, *case, fields=("result", "hit_x", "rgba8"), diag=False)
    _same(first, few, ("result", "hit_x", "rgba8"), "fewer outputs")


@pytest.mark.parametrize("case", [CASES[0], CASES[7]], ids=[IDS[0], IDS[7]])
def test_three_shards_are_the_whole_frames_rows(bhrt_lib, case):
    spin, disk, W, H, tol = case
    whole = _frame(bhrt_lib, case)
    seen = np.zeros(W * H, dtype=bool)
    for shard in range(3):
        rows = abi.Rows(4, shard, 3)     # 27 rows in blocks of 4: the last block has 3 rows
        part = _device_frame(bhrt_lib, spin, disk, W, H, tol, rows=rows)
        ys = np.arange(H)
        ys = ys[(ys // 4) % 3 == shard]
        idx = (ys[:, None] * W + np.arange(W)[None, :]).reshape(-1)
        assert len(idx) == len(part["result"])
        _same(part, {f: whole[f][idx] for f in whole}, ALL + DIAG, shard)
        seen[idx] = True
    assert seen.all()


@pytest.mark.parametrize("case", [CASES[3], CASES[6]], ids=[IDS[3], IDS[6]])
def test_ray_arrays_and_host_forms_equal_the_frame(bhrt_lib, case):
    import torch
    spin, disk, W, H, tol = case
    bh, dk, cfg = k5.scene(spin, disk, tol)
    cam = kr.camera()
    frame = _frame(bhrt_lib, case)
    rays = np.zeros(W * H, dtype=abi.RAY_DTYPE)
    rays["origin"] = (cam.position.x, cam.position.y, cam.position.z)
    rays["direction"] = kr.camera_dirs(cam, W, H)
    t, d = _tensors(W * H, ALL, diag=True)
    d_rays = torch.from_numpy(rays.view(np.float64).reshape(-1, 6)).cuda()
    torch.cuda.synchronize()
    bhrt_lib.kerr_rk45_rays_device(d_rays.data_ptr(), W * H, bh, dk, cfg, _flags(spin),
                                   bhrt_lib.soa_from_tensors(t), _kd(d), None)
    torch.cuda.synchronize()
    got = {f: v.cpu().numpy() for f, v in {**t, **d}.items()}
    _same(frame, got, ALL + DIAG, "rays_device")
    # the host forms: sky_* elements the kernel does not write keep what the arrays held (0)
    md = frame["result"] == kr.MAX_DISTANCE
    expect = {f: (np.where(md, frame[f], 0.0) if f.startswith("sky_") else frame[f]) for f in frame}
    host = bhrt_lib.kerr_rk45_frame(bh, dk, cfg, cam, W, H, _flags(spin), fields=ALL, diag=True)
    _same(expect, host, ALL + DIAG, "host frame")
    host = bhrt_lib.kerr_rk45_rays(rays, bh, dk, cfg, _flags(spin), fields=ALL, diag=True)
    _same(expect, host, ALL + DIAG, "host rays")


def test_offset_frames_edge_scenes_and_statistics(bhrt_lib):
    """A sub-pixel offset moves the frame and is itself reproducible from the ray-array call;
    max_integration_steps == 0 and a device ray without a static observer follow the rule; a
    launch counts as one trace launch whose iterations are the attempts."""
    import torch
    spin, disk, W, H, tol = CASES[4]
    bh, dk, cfg = k5.scene(spin, disk, tol)
    cam = kr.camera()
    centre = _frame(bhrt_lib, CASES[4])
    bhrt_lib.stats(reset=True)
    moved = _device_frame(bhrt_lib, spin, disk, W, H, tol, offset=(0.25, 0.75))
    st = bhrt_lib.stats(reset=True)
    assert st["launches"] == 1 and st["rays"] == W * H
    assert st["iterations"] == int(moved["steps"].sum())
    assert not np.array_equal(centre["hit_x"], moved["hit_x"])
    cam.use_offset, cam.offset_x, cam.offset_y = 1, 0.25, 0.75
    rays = np.zeros(W * H + 2, dtype=abi.RAY_DTYPE)
    rays["origin"] = (cam.position.x, cam.position.y, cam.position.z)
    rays["direction"][:W * H] = kr.camera_dirs(cam, W, H)
    rays["direction"][W * H:] = (0.0, 1.0, 0.0)
    rays["origin"][W * H] = (1.5, 0.0, 0.0)           # inside the ergosphere: no static observer
    rays["origin"][W * H + 1] = (0.3, 0.2, 0.1)       # inside the horizon
    t, d = _tensors(W * H + 2, HITS + RGB, diag=True)
    d_rays = torch.from_numpy(rays.view(np.float64).reshape(-1, 6)).cuda()
    torch.cuda.synchronize()
    bhrt_lib.kerr_rk45_rays_device(d_rays.data_ptr(), W * H + 2, bh, dk, cfg, _flags(spin),
                                   bhrt_lib.soa_from_tensors(t), _kd(d), None)
    torch.cuda.synchronize()
    got = {f: v.cpu().numpy() for f, v in {**t, **d}.items()}
    _same(moved, {f: v[:W * H] for f, v in got.items()}, HITS + RGB + DIAG, "offset rays")
    assert got["result"][W * H:].tolist() == [kr.ERROR, kr.ERROR]
    assert got["steps"][W * H:].tolist() == [0, 0] and (got["distance"][W * H:] == 0.0).all()
    assert got["rejected"][W * H:].tolist() == [0, 0]
    assert got["hit_x"][W * H:].tolist() == [1.5, 0.3]
    assert (got["sky_x"][W * H:] == 7.0).all()
    # the host form refuses the same array before any launch
    with pytest.raises(bhrt_lib.BhrtError, match="no static observer"):
        bhrt_lib.kerr_rk45_rays(rays, bh, dk, cfg, 0)
    # zero attempts: every ray ends at the origin, and reads the gradient on n
    cfg0 = abi.sim_config(kr.SCENE_DT, kr.SCENE_DIST, 0, tol)
    zero = bhrt_lib.kerr_rk45_frame(bh, dk, cfg0, kr.camera(), W, H, 0, diag=True)
    assert (zero["result"] == kr.MAX_STEPS).all() and (zero["steps"] == 0).all()
    assert (zero["rejected"] == 0).all()
    assert (zero["hit_y"] == -18.0).all() and (zero["distance"] == 0.0).all()
    n = kr.normalise(kr.camera_dirs(kr.camera(), W, H))
    tt = 0.5 * (n[:, 1] + 1.0)
    assert np.array_equal(zero["rgb_r"], (1.0 - tt) * 1.0 + tt * 0.5)
    # a short budget ends by attempts, rejected ones included, as the rule's
    few = _device_frame(bhrt_lib, spin, disk, W, H, tol, steps=9)
    rule = k5.frame_rule(spin, disk, W, H, tol, max_steps=9)
    keep = ~k5.knife_edge(spin, disk, W, H, tol)    # (the first nine attempts of the same rays)
    assert (few["result"] == kr.MAX_STEPS).any() and few["steps"].max() == 9
    for f in ("result", "steps", "rejected"):
        assert np.array_equal(few[f][keep], rule[f][keep]), f


def test_tolerance_refusals_raise(bhrt_lib):
    spin, disk, W, H, _ = CASES[0]
    for tol in (0.0, -1e-8, 9e-13, 2e-2, float("nan"), float("inf")):
        with pytest.raises(bhrt_lib.BhrtError, match="tolerance"):
            _device_frame(bhrt_lib, spin, disk, W, H, tol, fields=("result",), diag=False)
        bh, dk, cfg = k5.scene(spin, disk, tol)
        with pytest.raises(bhrt_lib.BhrtError, match="tolerance"):
            bhrt_lib.kerr_rk45_frame(bh, dk, cfg, kr.camera(), W, H, 0, fields=("result",))
    for tol in (1e-12, 1e-2):     # the bounds themselves are taken
        got = _device_frame(bhrt_lib, spin, disk, 8, 8, tol, fields=("result",), diag=False,
                            steps=50 if tol > 1e-3 else 4000)
        assert (got["result"] != 7).all()


# 4. sky maps -------------------------------------------------------------------------------------
def test_sky_flag_looks_up_the_rules_tangents(bhrt_lib):
    """The lookup vector is the exit tangent, which the GPU has to the 1e-5 contract per
    component: an angle of at most about 1e-5 rad, on a map that changes by <= 0.25 per radian
    (sky_rule.smooth_map) -- the bound is twice that product plus the 1e-9 floor; rays that fall
    back on n use test_gpu_kerr.py's bound."""
    data = sr.smooth_map()
    sky = bhrt_lib.sky_create(data)
    fallback_tol = 1e-9 + 0.5 * np.sqrt(3.0) * 1e-15
    try:
        bhrt_lib.set_sky(sky)
        worst = 0.0
        for case in (CASES[1], CASES[5]):
            spin, disk, W, H, tol = case
            rule = k5.frame_rule(*case)
            plain = _frame(bhrt_lib, case)
            got = _device_frame(bhrt_lib, *case, flags=_flags(spin) | abi.BHRT_FLAG_SKY, diag=False)
            _same(plain, got, HITS, "the flag changes no hit field")
            rgb = np.stack([got[c] for c in RGB], 1)
            res = rule["result"]
            assert np.array_equal(got["result"], res)
            keep = ~sr.uses_sky(res)     # disk and horizon pixels: the flagless frame's bits
            assert keep.any() and np.array_equal(rgb[keep], np.stack([plain[c] for c in RGB], 1)[keep])
            vec, took = sr.vectors(res, rule["chord"], rule["n"])
            want = sr.lookup(data, vec)
            tol_px = np.where(took, 1e-9 + 0.5 * EPS, fallback_tol)
            use = sr.uses_sky(res)
            ratio = np.where(use, np.abs(rgb - want).max(axis=1) / tol_px, 0.0)
            print(f"{case}: {int(took.sum())} tangent pixels, worst |diff| / tol {ratio.max():.3e}")
            assert took.sum() > 500 and (ratio <= 1.0).all(), (case, ratio.max())
            worst = max(worst, float(ratio.max()))
            assert np.array_equal(got["rgba8"], abi.rgba8_from_rgb(*[got[c] for c in RGB]))
        _figure("sky", f"worst |diff| / tol over the tangent pixels of two frames {worst:.3e}")
        bhrt_lib.set_sky(None)
        with pytest.raises(bhrt_lib.BhrtError, match="no sky map is bound"):
            _device_frame(bhrt_lib, *CASES[1], flags=abi.BHRT_FLAG_SKY, diag=False)
    finally:
        bhrt_lib.sky_destroy(sky)


# 5. streams --------------------------------------------------------------------------------------
def test_null_stream_orders_after_a_default_stream_fill(bhrt_lib):
    """A NULL hip_stream is ordered like the legacy default stream (as test_gpu_kerr.py's test,
    at its 192x108)."""
    spin, disk, _, _, tol = CASES[5]
    W, H = 192, 108
    bh, dk, cfg = k5.scene(spin, disk, tol)
    few = ("result", "hit_x", "rgba8")
    ref = _device_frame(bhrt_lib, spin, disk, W, H, tol, fields=few, diag=False)
    for _ in range(3):
        t, _d = _tensors(W * H, few)
        for v in t.values():       # default-stream fills of the outputs, right before the call
            v.fill_(3)
        bhrt_lib.kerr_rk45_frame_device(bh, dk, cfg, kr.camera(), W, H, None, _flags(spin),
                                        bhrt_lib.soa_from_tensors(t), None, None)
        got = {f: v.cpu().numpy() for f, v in t.items()}   # default-stream copies after it
        _same(ref, got, few, "NULL stream")
