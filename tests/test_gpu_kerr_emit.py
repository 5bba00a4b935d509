"""Kerr disk emission on the GPU (bhrt_kerr_emit_*; kerr.hip k_kerr_emit) against the numpy rule
(tests/kerr_emit_rule.py; stated in include/bhrt_api.h "Kerr disk emission").

Frames: test_gpu_kerr_rk45.py's six -- 48x27 and 49x27, camera at (0, -18, 4), three (spin, disk)
scenes -- at tolerance 1e-8 with K = 4, q = 3, and the 64-ray fan of kerr_emit_rule that grazes the
photon orbit of a spin-0.9 hole, extended by two device rays without a static observer. Class,
attempts, rejected attempts and the crossing count must equal the rule's on every ray outside the
rule's knife-edge sets (test_kerr_emit_cpu.py bounds them; none here); floats agree to the
project's 1e-5 contract (conftest.compare), the intensity to (4 + q) 1e-5: four times g's error
plus q times r's.

The worst observed ratios go to profiles/kerr_emit/test_figures.txt."""
import os

import numpy as np
import pytest

from conftest import ROOT, compare
from bhrt import abi
import kerr_rule as kr
import kerr_rk45_rule as k5
import kerr_emit_rule as ke

pytestmark = pytest.mark.gpu
FIGURES = os.path.join(ROOT, "profiles", "kerr_emit", "test_figures.txt")
RGB = ("rgb_r", "rgb_g", "rgb_b")
HITS = ("result", "steps", "hit_x", "hit_y", "hit_z", "distance", "sky_x", "sky_y", "sky_z")
ALL = HITS + RGB + ("rgba32f", "rgba8")
DIAG = ("h_residual", "lz_drift", "rejected")
EMIT = abi.EMIT_FIELDS
EPS = 1e-5
K4 = ke.MAX_CROSSINGS
Q, GAIN = ke.Q, 0.25          # (a gain that leaves most disk pixels below the clamp)
FRAMES = [(spin, disk, W, H) for spin, disk in kr.SCENES for W, H in kr.FRAME_SIZES]
IDS = [f"spin{spin}-{W}x{H}" for spin, _, W, H in FRAMES]


def _figure(key, text):
    """One line per key in profiles/kerr_emit/test_figures.txt, rewritten in place."""
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


def _tensors(n, K, fields, emit=EMIT, fill=7, diag=False):
    import torch
    dt = {"result": torch.int32, "steps": torch.int32, "rgba32f": torch.float32,
          "rgba8": torch.uint8, "rejected": torch.int32, "count": torch.int32}
    shape = {"rgba32f": (n, 4), "rgba8": (n, 4), "radius": (K, n), "redshift": (K, n)}
    mk = lambda f: torch.full(shape.get(f, (n,)), fill, dtype=dt.get(f, torch.float64), device="cuda")
    return ({f: mk(f) for f in fields}, {f: mk(f) for f in (DIAG if diag else ())},
            {f: mk(f) for f in emit})


def _structs(lib, t, d, e):
    soa = lib.soa_from_tensors(t)
    kd = abi.KerrRk45Diag(*(d[f].data_ptr() for f in DIAG)) if d else None
    eo = abi.KerrEmitOut(**{f: v.data_ptr() for f, v in e.items()}) if e else None
    return soa, kd, eo


def _numpy(*groups):
    return {f: v.cpu().numpy() for g in groups for f, v in g.items()}


def _device_frame(lib, spin, disk, W, H, K=K4, rows=None, stream=None, fields=ALL, emit=EMIT,
                  diag=True, flags=0, q=Q, gain=GAIN):
    """One bhrt_kerr_emit_frame_device call into fresh device arrays (fill 7), as numpy arrays."""
    import torch
    bh, dk, cfg = k5.scene(spin, disk, ke.TOL)
    n = W * (H if rows is None else lib.shard_rows(H, rows))
    t, d, e = _tensors(n, K, fields, emit, diag=diag)
    soa, kd, eo = _structs(lib, t, d, e)
    torch.cuda.synchronize()
    lib.kerr_emit_frame_device(bh, dk, cfg, kr.camera(), W, H, rows, flags, soa,
                               abi.KerrEmitParams(K, q, gain), eo, kd, stream)
    torch.cuda.synchronize()
    return _numpy(t, d, e)


_FRAMES = {}


def _frame(lib, frame, K=K4):
    """The whole device frame of a case, rendered once for the module and left unchanged."""
    key = frame + (K,)
    if key not in _FRAMES:
        f = _device_frame(lib, *frame, K=K)
        for v in f.values():
            v.setflags(write=False)
        _FRAMES[key] = f
    return _FRAMES[key]


def _same(a, b, fields, what=""):
    for f in fields:
        assert np.array_equal(a[f], b[f], equal_nan=True), (what, f)


def _against_rule(name, got, rule, knife, q):
    """Integers equal outside the knife-edge set, floats to the contract, the fill kept beyond a
    ray's count; returns the worst |diff| / tolerance."""
    K = rule["radius"].shape[0]
    keep = ~knife
    for f in ("result", "steps", "rejected", "count"):
        bad = np.nonzero((got[f] != rule[f]) & keep)[0]
        print(f"{name}: {f} differs on {bad.size} rays outside the knife-edge set "
              f"({int(knife.sum())} in it)")
        assert bad.size == 0, (f, bad[:10], got[f][bad[:10]], rule[f][bad[:10]])
    same = keep & (got["result"] == rule["result"]) & (got["steps"] == rule["steps"]) & \
        (got["count"] == rule["count"])
    md = rule["result"] == kr.MAX_DISTANCE
    want = {"distance": rule["distance"]}
    for k, ax in enumerate("xyz"):
        want["hit_" + ax] = rule["hit"][:, k]
        want["sky_" + ax] = np.where(md, rule["chord"][:, k], 7.0)
    # (the colour is checked on the GPU's own crossings: test_colour_is_the_formula_...)
    beyond = np.arange(K)[:, None] >= got["count"][None, :]
    for f in ("radius", "redshift"):
        assert (got[f][beyond] == 7.0).all(), f          # not written: the fill
        for k in range(K):
            want[f"{f}{k}"] = np.where(rule["count"] > k, rule[f][k], 7.0)
            got = dict(got, **{f"{f}{k}": got[f][k]})
    fields = tuple(want)
    worst = max(float(np.max(np.abs(got[f][same] - want[f][same]) /
                             (EPS * np.maximum(np.abs(got[f][same]), np.abs(want[f][same])) + 1e-9)))
                for f in fields)
    compare({f: got[f][same] for f in fields}, {f: want[f][same] for f in fields}, EPS,
            check_sky=True, what=name, fields=fields)
    # the intensity: four times g's error plus q times r's
    a, b = got["intensity"][same], rule["intensity"][same]
    tol = (4.0 + q) * EPS * np.maximum(np.abs(a), np.abs(b)) + 1e-300
    ratio = float(np.max(np.abs(a - b) / tol))
    print(f"{name}: worst |diff| / tol {worst:.3e}, intensity {ratio:.3e}")
    assert ratio <= 1.0, ratio
    assert (got["intensity"][got["count"] == 0] == 0.0).all()
    return worst, ratio


# 1. frames and fan against the rule --------------------------------------------------------------
@pytest.mark.parametrize("frame", FRAMES, ids=IDS)
def test_frames_match_the_rule(bhrt_lib, frame):
    spin, disk, W, H = frame
    name = IDS[FRAMES.index(frame)]
    rule = ke.frame_rule(spin, disk, W, H, K4)
    knife = ke.knife_edge(spin, disk, W, H, K4)
    assert knife.sum() <= 0.01 * len(knife), int(knife.sum())
    got = _frame(bhrt_lib, frame)
    worst, ratio = _against_rule(name, got, rule, knife, Q)
    counts = np.bincount(got["count"], minlength=K4 + 1).tolist()
    classes = np.bincount(got["result"], minlength=6).tolist()
    assert (got["count"] >= 2).sum() >= 10
    _figure(f"frame {name}",
            f"classes {classes}, crossings {counts}, attempts {int(got['steps'].sum())}, rejected "
            f"{int(got['rejected'].sum())}, knife-edge {int(knife.sum())}, worst |diff| / tol "
            f"{worst:.3e}, intensity |diff| / tol {ratio:.3e}")


def test_fan_and_two_rays_without_an_observer(bhrt_lib):
    """The fan's 64 rays and two device rays whose origins have no static observer (inside the
    ergosphere, inside the horizon): 66 rays, so the last wave runs with 62 dead lanes."""
    import torch
    bh, dk, cfg = ke.fan_scene()
    rule = ke.fan_trace()
    knife = ke.fan_knife_edge()
    assert knife.sum() <= 2
    n = ke.FAN_RAYS + 2
    rays = np.zeros(n, dtype=abi.RAY_DTYPE)
    rays["origin"] = ke.FAN_ORIGIN
    rays["direction"][:ke.FAN_RAYS] = ke.fan_dirs()
    rays["direction"][ke.FAN_RAYS:] = (0.0, 1.0, 0.0)
    rays["origin"][ke.FAN_RAYS] = (1.5, 0.0, 0.0)
    rays["origin"][ke.FAN_RAYS + 1] = (0.3, 0.2, 0.1)
    fields = HITS + RGB
    t, d, e = _tensors(n, K4, fields, diag=True)
    soa, kd, eo = _structs(bhrt_lib, t, d, e)
    d_rays = torch.from_numpy(rays.view(np.float64).reshape(-1, 6)).cuda()
    torch.cuda.synchronize()
    bhrt_lib.stats(reset=True)
    bhrt_lib.kerr_emit_rays_device(d_rays.data_ptr(), n, bh, dk, cfg, 0, soa,
                                   abi.KerrEmitParams(K4, Q, GAIN), eo, kd, None)
    torch.cuda.synchronize()
    st = bhrt_lib.stats(reset=True)
    got = _numpy(t, d, e)
    assert st["launches"] == 1 and st["rays"] == n and st["iterations"] == int(got["steps"].sum())
    head = {f: (v[:, :ke.FAN_RAYS] if v.ndim == 2 and v.shape[0] == K4 else v[:ke.FAN_RAYS])
            for f, v in got.items()}
    worst, ratio = _against_rule("fan", head, rule, knife, Q)
    counts = np.bincount(head["count"], minlength=K4 + 1).tolist()
    assert (head["count"] >= 3).sum() >= 10 and (head["result"] == kr.DISK).sum() >= 1
    _figure("fan", f"crossings {counts}, classes {np.bincount(head['result'], minlength=6).tolist()}, "
                   f"knife-edge {int(knife.sum())}, worst |diff| / tol {worst:.3e}, intensity "
                   f"|diff| / tol {ratio:.3e}")
    tail = slice(ke.FAN_RAYS, n)
    assert got["result"][tail].tolist() == [kr.ERROR, kr.ERROR]
    assert got["steps"][tail].tolist() == [0, 0] and got["count"][tail].tolist() == [0, 0]
    assert (got["intensity"][tail] == 0.0).all() and (got["radius"][:, tail] == 7.0).all()
    assert got["hit_x"][tail].tolist() == [1.5, 0.3] and (got["sky_x"][tail] == 7.0).all()


# 2. K = 1 against bhrt_kerr_rk45_frame_device ----------------------------------------------------
@pytest.mark.parametrize("frame", [FRAMES[1], FRAMES[4]], ids=[IDS[1], IDS[4]])
def test_one_crossing_is_the_adaptive_frame(bhrt_lib, frame):
    """Two compilations of one step: classes, attempts and rejected equal outside the knife-edge
    set, floats to 1e-5; count is 1 exactly on the disk rays."""
    import torch
    spin, disk, W, H = frame
    bh, dk, cfg = k5.scene(spin, disk, ke.TOL)
    got = _frame(bhrt_lib, frame, K=1)
    t, d, _ = _tensors(W * H, 1, HITS, emit=(), diag=True)
    soa, kd, _ = _structs(bhrt_lib, t, d, {})
    torch.cuda.synchronize()
    bhrt_lib.kerr_rk45_frame_device(bh, dk, cfg, kr.camera(), W, H, None, 0, soa, kd, None)
    torch.cuda.synchronize()
    ref = _numpy(t, d)
    keep = ~k5.knife_edge(spin, disk, W, H, ke.TOL)
    for f in ("result", "steps", "rejected"):
        assert np.array_equal(got[f][keep], ref[f][keep]), f
    assert np.array_equal(got["count"], (got["result"] == kr.DISK).astype(np.int32))
    fields = tuple(f for f in HITS if f not in ("result", "steps"))
    same = keep & (got["result"] == ref["result"]) & (got["steps"] == ref["steps"])
    worst = compare({f: got[f][same] for f in fields}, {f: ref[f][same] for f in fields}, EPS,
                    check_sky=True, what=str(frame), fields=fields)
    _figure(f"K1 {IDS[FRAMES.index(frame)]}", f"worst relative difference from the adaptive frame "
                                              f"{worst:.3e}")


# 3. colour ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", [FRAMES[0], FRAMES[5]], ids=[IDS[0], IDS[5]])
def test_colour_is_the_formula_on_the_gpus_own_crossings(bhrt_lib, frame):
    """rgb equals the colour formula in numpy on the GPU's own count, radius and redshift (base_k
    at rxy = sqrt(radius^2 + a^2)) to 1e-9 absolute, so the trace's differences are not amplified
    through the temperature ramp; count-0 pixels are the adaptive frame's bits; rgba32f and rgba8
    are the conversions of rgb."""
    import torch
    spin, disk, W, H = frame
    bh, dk, cfg = k5.scene(spin, disk, ke.TOL)
    got = _frame(bhrt_lib, frame)
    rgb = np.stack([got[c] for c in RGB], 1)
    a = bh.spin * bh.mass
    want = ke.emission_colour(got["count"], got["radius"], got["redshift"], a * a, dk, Q, GAIN)
    has = got["count"] > 0
    err = float(np.abs(rgb[has] - want[has]).max())
    print(f"{frame}: {int(has.sum())} emission pixels, colour off by {err:.2e}; "
          f"{int((want[has] == 1.0).any(axis=1).sum())} clamped")
    assert has.sum() >= 200 and err <= 1e-9      # (the disk covers 240 pixels and more)
    assert ((want[has] > 0.0) & (want[has] < 1.0)).any(axis=1).sum() >= 100  # not all clamped
    t, _, _ = _tensors(W * H, 1, RGB + ("result",), emit=())
    torch.cuda.synchronize()
    bhrt_lib.kerr_rk45_frame_device(bh, dk, cfg, kr.camera(), W, H, None, 0,
                                    bhrt_lib.soa_from_tensors(t), None, None)
    torch.cuda.synchronize()
    ref = _numpy(t)
    assert (~has).sum() > 300
    for c in RGB:
        assert np.array_equal(got[c][~has], ref[c][~has]), c
    assert np.array_equal(got["rgba32f"][:, :3], rgb.astype(np.float32))
    assert (got["rgba32f"][:, 3] == 1.0).all()
    assert np.array_equal(got["rgba8"], abi.rgba8_from_rgb(*[got[c] for c in RGB]))
    _figure(f"colour {IDS[FRAMES.index(frame)]}", f"{int(has.sum())} emission pixels off by {err:.2e}")


# 4. bit identity and sharding --------------------------------------------------------------------
def test_same_bits_run_to_run_on_two_streams_and_with_fewer_outputs(bhrt_lib):
    import torch
    frame = FRAMES[5]
    first = _frame(bhrt_lib, frame)
    _same(first, _device_frame(bhrt_lib, *frame), ALL + DIAG + EMIT, "run to run")
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        _same(first, _device_frame(bhrt_lib, *frame, stream=s.cuda_stream), ALL + EMIT, "stream")
    few = _device_frame(bhrt_lib, *frame, fields=("result", "rgba8"), emit=("redshift",), diag=False)
    _same(first, few, ("result", "rgba8", "redshift"), "fewer outputs")
    only = _device_frame(bhrt_lib, *frame, fields=(), emit=("intensity",), diag=False)
    _same(first, only, ("intensity",), "intensity alone")


def test_three_shards_are_the_whole_frames_rows(bhrt_lib):
    frame = FRAMES[5]
    spin, disk, W, H = frame
    whole = _frame(bhrt_lib, frame)
    seen = np.zeros(W * H, dtype=bool)
    for shard in range(3):
        rows = abi.Rows(4, shard, 3)     # 27 rows in blocks of 4: the last block has 3 rows
        part = _device_frame(bhrt_lib, spin, disk, W, H, rows=rows)
        ys = np.arange(H)
        ys = ys[(ys // 4) % 3 == shard]
        idx = (ys[:, None] * W + np.arange(W)[None, :]).reshape(-1)
        assert len(idx) == len(part["result"])
        _same(part, {f: (v[:, idx] if f in ("radius", "redshift") else v[idx])
                     for f, v in whole.items()}, ALL + DIAG + EMIT, shard)
        seen[idx] = True
    assert seen.all()


def test_ray_arrays_and_host_forms_equal_the_frame(bhrt_lib):
    import torch
    frame = FRAMES[2]
    spin, disk, W, H = frame
    bh, dk, cfg = k5.scene(spin, disk, ke.TOL)
    cam = kr.camera()
    ep = abi.KerrEmitParams(K4, Q, GAIN)
    whole = _frame(bhrt_lib, frame)
    rays = np.zeros(W * H, dtype=abi.RAY_DTYPE)
    rays["origin"] = (cam.position.x, cam.position.y, cam.position.z)
    rays["direction"] = kr.camera_dirs(cam, W, H)
    t, d, e = _tensors(W * H, K4, ALL, diag=True)
    soa, kd, eo = _structs(bhrt_lib, t, d, e)
    d_rays = torch.from_numpy(rays.view(np.float64).reshape(-1, 6)).cuda()
    torch.cuda.synchronize()
    bhrt_lib.kerr_emit_rays_device(d_rays.data_ptr(), W * H, bh, dk, cfg, 0, soa, ep, eo, kd, None)
    torch.cuda.synchronize()
    _same(whole, _numpy(t, d, e), ALL + DIAG + EMIT, "rays_device")
    # the host forms leave unwritten elements as they were: sky_* held 0, the planes the fill
    md = whole["result"] == kr.MAX_DISTANCE
    expect = {f: (np.where(md, v, 0.0) if f.startswith("sky_") else v) for f, v in whole.items()}
    host = bhrt_lib.kerr_emit_frame(bh, dk, cfg, cam, W, H, ep, 0, fields=ALL, diag=True, fill=7.0)
    _same(expect, host, ALL + DIAG + EMIT, "host frame")
    host = bhrt_lib.kerr_emit_rays(rays, bh, dk, cfg, ep, 0, fields=ALL, diag=True, fill=7.0)
    _same(expect, host, ALL + DIAG + EMIT, "host rays")
    beyond = np.arange(K4)[:, None] >= host["count"][None, :]
    assert beyond.any() and (host["radius"][beyond] == 7.0).all()


# 5. stream order, statistics, refusals -----------------------------------------------------------
def test_null_stream_orders_after_a_default_stream_fill_and_counts_one_launch(bhrt_lib):
    """A NULL hip_stream is ordered like the legacy default stream (as test_gpu_kerr_rk45.py's
    test, at its 192x108); the launch is one trace launch whose iterations are the attempts."""
    spin, disk = kr.SCENES[2]
    W, H = 192, 108
    bh, dk, cfg = k5.scene(spin, disk, ke.TOL)
    ep = abi.KerrEmitParams(K4, Q, GAIN)
    few, emit = ("result", "steps", "rgba8"), ("count", "intensity")
    bhrt_lib.stats(reset=True)
    ref = _device_frame(bhrt_lib, spin, disk, W, H, fields=few, emit=emit, diag=False)
    st = bhrt_lib.stats(reset=True)
    assert st["launches"] == 1 and st["rays"] == W * H
    assert st["iterations"] == int(ref["steps"].sum())
    for _ in range(3):
        t, _d, e = _tensors(W * H, K4, few, emit)
        for v in list(t.values()) + list(e.values()):   # default-stream fills right before the call
            v.fill_(3)
        soa, _kd, eo = _structs(bhrt_lib, t, {}, e)
        bhrt_lib.kerr_emit_frame_device(bh, dk, cfg, kr.camera(), W, H, None, 0, soa, ep, eo, None,
                                        None)
        _same(ref, _numpy(t, e), few + emit, "NULL stream")   # default-stream copies after it


def test_refusals_raise(bhrt_lib):
    spin, disk, W, H = FRAMES[0]
    bh, dk, cfg = k5.scene(spin, disk, ke.TOL)
    cam = kr.camera()
    for ep, needle in ((abi.KerrEmitParams(0), "max_crossings"), (abi.KerrEmitParams(5), "max_crossings"),
                       (abi.KerrEmitParams(1, -1.0), "emissivity_index"),
                       (abi.KerrEmitParams(1, 3.0, float("nan")), "gain"), (None, "params")):
        with pytest.raises(bhrt_lib.BhrtError, match=needle):
            bhrt_lib.kerr_emit_frame(bh, dk, cfg, cam, W, H, ep)
    good = abi.KerrEmitParams(2)
    with pytest.raises(bhrt_lib.BhrtError, match="BHRT_FLAG_DOPPLER"):
        _device_frame(bhrt_lib, spin, disk, W, H, K=2, flags=abi.BHRT_FLAG_DOPPLER)
    with pytest.raises(bhrt_lib.BhrtError, match="disk"):
        bhrt_lib.kerr_emit_frame(bh, None, cfg, cam, W, H, good)
    with pytest.raises(bhrt_lib.BhrtError, match="no output"):
        _device_frame(bhrt_lib, spin, disk, W, H, K=2, fields=(), emit=(), diag=False)
    with pytest.raises(bhrt_lib.BhrtError, match="tolerance"):
        bhrt_lib.kerr_emit_frame(*k5.scene(spin, disk, 1e-13), cam, W, H, good)
