"""Supersampled camera frames (bhrt_render_frame_ss_device / bhrt_render_frame_ss): every pixel
is trace_pixel's sample average (raytracer.c:1044-1167).

All frames use camera B. Reference for a frame: for s in 0..S-1 the oracle's frame at the offset
orc_jittered_offset(s, spp, method, strength), accumulated acc = acc + plane_s in that order and
divided by S; the class is plane 0's. On every case below the oracle has no sample whose
knife-edge margin is below KNIFE_EDGE (asserted), so no pixel is exempt.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import KNIFE_EDGE, compare
from bhrt import abi, configs

pytestmark = pytest.mark.gpu
RTOL = 1e-5
THREADS = 16
GRID, HALTON = abi.JITTER_REGULAR_GRID, abi.JITTER_HALTON
RGB = ("rgb_r", "rgb_g", "rgb_b")
SS_FIELDS = ("result",) + RGB + ("rgba32f", "rgba8")


def _scene(name):
    """(bh, dk, cfg, method, flags)"""
    if name == "kerr099":  # the disk down to the ISCO of a = 0.99: hits at r_xy < 2 are NaN
        bh = abi.black_hole(1.0, 0.99)
        return (bh, abi.disk(bh.isco_radius, 20.0, 1.0, 1.0), abi.sim_config(0.1, 100.0, 1000, 1e-6),
                abi.INTEGRATOR_RK4, abi.BHRT_FLAG_DOPPLER)
    c = configs.CONFIGS[name]
    return c.scene() + (c.method, c.flags)


def _orc_offsets(oracle, ss):
    fn = oracle.lib.orc_jittered_offset
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    fn.restype = None
    out = []
    for s in range(ss.samples_per_pixel):
        ox, oy = C.c_double(), C.c_double()
        fn(s, ss.samples_per_pixel, ss.jitter_method, ss.jitter_strength, C.byref(ox), C.byref(oy))
        out.append((ox.value, oy.value))
    return out


_cache = {}


def _oracle_frame(oracle, name, W, H, jm, spp, strength):
    """The oracle's supersampled frame and the smallest margin of its samples; computed once
    per case, never modified."""
    key = (name, W, H, jm, spp, strength)
    if key not in _cache:
        bh, dk, cfg, method, flags = _scene(name)
        ss = abi.SupersamplingParams(spp, jm, strength)
        acc = {f: np.zeros(W * H) for f in RGB}
        result, margin_min = None, np.inf
        for s, (ox, oy) in enumerate(_orc_offsets(oracle, ss)):
            cam = configs.camera("B")
            cam.use_offset, cam.offset_x, cam.offset_y = 1, ox, oy
            plane, margin = oracle.render_frame_margin(bh, dk, cfg, cam, W, H, method, flags,
                                                       threads=THREADS)
            assert not (margin < KNIFE_EDGE).any(), (key, s)
            margin_min = min(margin_min, float(np.nanmin(margin)))
            if s == 0:
                result = plane["result"].copy()
            for f in RGB:
                acc[f] = acc[f] + plane[f]
        want = {f: acc[f] / spp for f in RGB}
        want["result"] = result
        for v in want.values():
            v.setflags(write=False)
        _cache[key] = (want, margin_min)
    return _cache[key]


def _tensors(n, fields, fill=7):
    import torch
    dt = {"result": torch.int32, "steps": torch.int32, "rgba32f": torch.float32,
          "rgba8": torch.uint8}
    return {f: torch.full((n, 4) if f in abi.DISPLAY_FIELDS else (n,), fill,
                          dtype=dt.get(f, torch.float64), device="cuda") for f in fields}


def _ss_device(lib, name, W, H, ss, as_=None, rows=None, fields=SS_FIELDS, stream=None):
    """One supersampled device frame (a shard with rows) as numpy arrays."""
    import torch
    bh, dk, cfg, method, flags = _scene(name)
    n = W * (H if rows is None else lib.shard_rows(H, rows))
    t = _tensors(n, fields)
    torch.cuda.synchronize()
    lib.render_frame_ss_device(bh, dk, cfg, configs.camera("B"), W, H, rows, method, flags, ss,
                               as_, lib.soa_from_tensors(t), stream)
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in t.items()}


def _plain_device(lib, name, W, H, offset=None, fields=("result", "hit_x", "hit_y") + RGB):
    """One bhrt_render_frame_device frame, at a sub-pixel offset if given."""
    import torch
    bh, dk, cfg, method, flags = _scene(name)
    cam = configs.camera("B")
    if offset is not None:
        cam.use_offset, cam.offset_x, cam.offset_y = 1, float(offset[0]), float(offset[1])
    t = _tensors(W * H, fields)
    torch.cuda.synchronize()
    lib.render_frame_device(bh, dk, cfg, cam, W, H, None, method, flags, lib.soa_from_tensors(t),
                            None)
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in t.items()}


def _same(a, b, fields, what=""):
    for f in fields:
        assert np.array_equal(a[f], b[f], equal_nan=True), (what, f)


# 1. against the oracle ---------------------------------------------------------------------
ORACLE_CASES = [
    ("C2", 40, 24, GRID, 4, 1.0),
    ("C2", 23, 7, HALTON, 5, 0.5),     # 805 sample rays: a partial last wave
    ("C4", 48, 27, GRID, 5, 1.0),      # the fifth sample of a "2x2" grid, off the pixel; Doppler
    ("C3", 32, 18, HALTON, 4, 1.0),    # RKF45 + disk
    ("C1", 16, 16, GRID, 2, 1.0),      # grid size 1: second sample at (0.5, 1.5); no-disk kernel
    ("C5", 32, 18, HALTON, 3, 0.75),
    ("kerr099", 64, 36, GRID, 4, 1.0),  # NaN disk colours
]


@pytest.mark.parametrize("name,W,H,jm,spp,strength", ORACLE_CASES)
def test_frame_vs_oracle(bhrt_lib, oracle, name, W, H, jm, spp, strength):
    want, margin_min = _oracle_frame(oracle, name, W, H, jm, spp, strength)
    nan_pixels = int(np.isnan(want["rgb_r"]).sum())
    if name == "kerr099":
        assert nan_pixels > 0  # (24 on the oracle: one NaN sample makes the pixel NaN)
    got = _ss_device(bhrt_lib, name, W, H, abi.SupersamplingParams(spp, jm, strength))
    worst = compare(got, want, RTOL, False, f"{name} {W}x{H} S={spp}", fields=("result",) + RGB)
    print(f"{name} {W}x{H} S={spp}: oracle min margin {margin_min:.2e}, NaN pixels {nan_pixels}, "
          f"max rel err {worst:.2e}")
    assert np.array_equal(got["rgba8"], abi.rgba8_from_rgb(*(got[f] for f in RGB)))
    rgb32 = np.stack([got[f] for f in RGB], axis=1).astype(np.float32)
    assert np.array_equal(got["rgba32f"][:, :3], rgb32, equal_nan=True)
    assert (got["rgba32f"][:, 3] == 1.0).all()


# 2. against libbhrt's own sample frames -------------------------------------------------------
# The sample rays' directions are the camera path's bit for bit (k_ss_rays runs camera_dir on a
# camera block read in place, as k_trace does), but the trace kernel's shared-origin
# instantiation (ray_init_shared) and its camera instantiation (ray_init_camera) are two
# compilations of the same second normalisation, and hipcc contracts the squared length in
# them in different orders (y*y first / x*x first): initial velocities one ulp apart, seen at
# the end of a path as ~1e-14 (hit point, disk colour). That lies in k_trace, which this feature
# does not touch, so the comparison with the camera path's frames is at RTOL (classes exact);
# the measured deviation is printed, and recorded in DESIGN.md section 11. The accumulation
# itself is pinned bit for bit by test_average_is_sequential_bit_for_bit.
@pytest.mark.parametrize("name,W,H,jm,spp", [("C2", 40, 24, GRID, 4), ("C4", 40, 40, HALTON, 3)])
def test_frame_is_the_sequential_mean_of_its_sample_frames(bhrt_lib, name, W, H, jm, spp):
    ss = abi.SupersamplingParams(spp, jm, 1.0)
    offsets = bhrt_lib.sample_offsets(ss)
    assert len(offsets) == spp
    planes = [_plain_device(bhrt_lib, name, W, H, off) for off in offsets]
    got = _ss_device(bhrt_lib, name, W, H, ss)
    want = {"result": planes[0]["result"]}
    for f in RGB:
        acc = np.zeros(W * H)
        for p in planes:
            acc = acc + p[f]
        want[f] = acc / spp
    exact = all(np.array_equal(got[f], want[f], equal_nan=True) for f in RGB)
    worst = compare(got, want, RTOL, False, f"{name} own samples", fields=("result",) + RGB)
    print(f"{name} {W}x{H} S={spp} vs the mean of {spp} camera frames: bit-identical {exact}, "
          f"max rel deviation {worst:.2e}")


def test_no_supersampling_is_the_plain_frame(bhrt_lib):
    W, H = 64, 36
    got = _ss_device(bhrt_lib, "C2", W, H, None)
    want = _plain_device(bhrt_lib, "C2", W, H, fields=("result", "hit_x", "hit_y") + RGB +
                         abi.DISPLAY_FIELDS)
    exact = all(np.array_equal(got[f], want[f], equal_nan=True) for f in SS_FIELDS)
    worst = compare(got, want, RTOL, False, "C2 ss = NULL", fields=("result",) + RGB)
    print(f"C2 {W}x{H} ss = NULL vs the plain frame: bit-identical {exact}, max rel deviation "
          f"{worst:.2e}")
    np.testing.assert_allclose(got["rgba32f"], want["rgba32f"], rtol=RTOL, atol=1e-9)
    # (the byte is a truncation: a last-bit difference of the colour can move it by one)
    assert np.abs(got["rgba8"].astype(int) - want["rgba8"].astype(int)).max() <= 1


def test_average_is_sequential_bit_for_bit(bhrt_lib):
    """The accumulation order and the division, bit for bit, on sample planes that are known
    exactly: adaptive sampling without SupersamplingParams takes max_samples copies of the
    centre sample, so every plane is the one-sample frame X of the same path, and the pixel is
    ((0.0 + X) + X + X) / 3 -- not X's bits in general -- with every output converted from it."""
    W, H = 64, 36
    for name in ("C2", "C4"):
        one = _ss_device(bhrt_lib, name, W, H, None)
        got = _ss_device(bhrt_lib, name, W, H, None,
                         as_=abi.AdaptiveSamplingParams(1, 1, 3, 0.0, 0.0))
        assert np.array_equal(got["result"], one["result"])
        changed = 0
        for f in RGB:
            want = (((0.0 + one[f]) + one[f]) + one[f]) / 3
            assert np.array_equal(got[f], want, equal_nan=True), (name, f)
            changed += int((want != one[f]).sum())
        assert changed > 0  # (the case is decisive: the average is not the sample's own bits)
        rgb32 = np.stack([got[f] for f in RGB], axis=1).astype(np.float32)
        assert np.array_equal(got["rgba32f"][:, :3], rgb32, equal_nan=True)
        assert np.array_equal(got["rgba8"], abi.rgba8_from_rgb(*(got[f] for f in RGB)))


# 3. determinism -------------------------------------------------------------------------------
def test_same_frame_twice_and_on_any_stream(bhrt_lib):
    import torch
    ss = abi.SupersamplingParams(4, GRID, 1.0)
    a = _ss_device(bhrt_lib, "C2", 40, 24, ss)
    b = _ss_device(bhrt_lib, "C2", 40, 24, ss)
    _same(a, b, SS_FIELDS, "twice")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c = _ss_device(bhrt_lib, "C2", 40, 24, ss, stream=s.cuda_stream)
    _same(a, c, SS_FIELDS, "torch stream")


def test_null_stream_orders_after_default_stream_fills(bhrt_lib):
    """Outputs poison-filled on the default stream behind a busy kernel, no sync before the
    NULL-stream call, read back on the default stream: the frame, not the fill."""
    import torch
    assert torch.cuda.current_stream().cuda_stream == 0
    W, H = 40, 24
    ss = abi.SupersamplingParams(4, GRID, 1.0)
    want = _ss_device(bhrt_lib, "C2", W, H, ss)
    bh, dk, cfg, method, flags = _scene("C2")
    t = _tensors(W * H, SS_FIELDS, fill=0)
    torch.cuda.synchronize()  # (allocation done; everything below stays queued)
    sleep = getattr(torch.cuda, "_sleep", None)
    if sleep is not None:
        sleep(20_000_000)
    else:
        a = torch.ones(2048, 2048, device="cuda")
        for _ in range(8):
            a = a @ a * 1e-3
    for v in t.values():
        v.fill_(3)
    bhrt_lib.render_frame_ss_device(bh, dk, cfg, configs.camera("B"), W, H, None, method, flags,
                                    ss, None, bhrt_lib.soa_from_tensors(t), None)
    got = {f: v.cpu().numpy() for f, v in t.items()}
    _same(got, want, SS_FIELDS)


# 4. shards ------------------------------------------------------------------------------------
def test_uneven_shards_reassemble_to_the_frame(bhrt_lib):
    W, H, B, S = 40, 40, 8, 3
    ss = abi.SupersamplingParams(4, GRID, 1.0)
    whole = _ss_device(bhrt_lib, "C2", W, H, ss)
    built = {f: np.full_like(whole[f], 9) for f in SS_FIELDS}
    rows_of = []
    for k in range(S):
        rows = abi.Rows(B, k, S)
        shard = _ss_device(bhrt_lib, "C2", W, H, ss, rows=rows)
        nrows = bhrt_lib.shard_rows(H, rows)
        rows_of.append(nrows)
        for r in range(nrows):
            g = ((r // B) * S + k) * B + r % B  # local row r is image row g
            for f in SS_FIELDS:
                built[f][g * W:(g + 1) * W] = shard[f][r * W:(r + 1) * W]
    assert rows_of == [16, 16, 8]
    _same(built, whole, SS_FIELDS)


# 5. trace_pixel -------------------------------------------------------------------------------
def test_pixels_equal_trace_pixel(bhrt_lib):
    L = bhrt_lib.load()
    W, H = 24, 16
    ss = abi.SupersamplingParams(5, HALTON, 0.5)
    got = _ss_device(bhrt_lib, "C2", W, H, ss)
    bh, dk, cfg, method, flags = _scene("C2")
    assert method == abi.INTEGRATOR_RK4 and flags == 0  # (what trace_pixel traces with)
    c = configs.camera("B")
    for px, py in ((3, 5), (12, 8), (0, 0), (23, 15)):
        col = (C.c_double * 3)()
        res = L.trace_pixel(px, py, W, H, C.byref(c.position), C.byref(c.direction), C.byref(c.up),
                            c.fov_deg, C.byref(bh), C.byref(dk), C.byref(cfg), C.byref(ss), None,
                            C.byref(col))
        i = py * W + px
        assert res == got["result"][i], (px, py)
        np.testing.assert_allclose([got[f][i] for f in RGB], list(col), rtol=RTOL, atol=1e-9)


# 6. host variant ------------------------------------------------------------------------------
@pytest.mark.parametrize("fields", [("rgba8",), SS_FIELDS])
def test_host_frame_equals_device_frame(bhrt_lib, fields):
    W, H = 40, 24
    ss = abi.SupersamplingParams(4, GRID, 1.0)
    bh, dk, cfg, method, flags = _scene("C2")
    host = bhrt_lib.render_frame_ss(bh, dk, cfg, configs.camera("B"), W, H, method, flags, ss,
                                    None, fields=fields)
    dev = _ss_device(bhrt_lib, "C2", W, H, ss, fields=fields)
    assert tuple(host) == tuple(fields)
    _same(host, dev, fields)


# 7. arguments ---------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["steps", "random", "use_offset", "65 samples", "rgb_r alone"])
def test_bad_arguments_are_refused_and_write_nothing(bhrt_lib, what):
    import torch
    L = bhrt_lib.load()
    W, H = 16, 8
    bh, dk, cfg, method, flags = _scene("C2")
    cam = configs.camera("B")
    ss = abi.SupersamplingParams(4, GRID, 1.0)
    fields = SS_FIELDS
    if what == "steps":
        fields = SS_FIELDS + ("steps",)
    elif what == "random":
        ss = abi.SupersamplingParams(4, abi.JITTER_RANDOM, 1.0)
    elif what == "use_offset":
        cam.use_offset, cam.offset_x, cam.offset_y = 1, 0.25, 0.25
    elif what == "65 samples":
        ss = abi.SupersamplingParams(65, HALTON, 1.0)
    elif what == "rgb_r alone":
        fields = ("result", "rgb_r")
    t = _tensors(W * H, fields)
    host, host_soa = abi.alloc_soa(W * H, fields)
    for v in host.values():
        v[...] = 7
    torch.cuda.synchronize()
    soa = bhrt_lib.soa_from_tensors(t)
    assert L.bhrt_render_frame_ss_device(C.byref(bh), C.byref(dk), C.byref(cfg), C.byref(cam), W,
                                         H, None, method, flags, C.byref(ss), None, C.byref(soa),
                                         None) == -1
    assert bhrt_lib.last_error()
    assert L.bhrt_render_frame_ss(C.byref(bh), C.byref(dk), C.byref(cfg), C.byref(cam), W, H,
                                  method, flags, C.byref(ss), None, C.byref(host_soa)) == -1
    assert bhrt_lib.last_error()
    torch.cuda.synchronize()
    for f in fields:
        assert (t[f].cpu().numpy() == 7).all(), f
        assert (host[f] == 7).all(), f


# 8. statistics --------------------------------------------------------------------------------
def test_stats_count_the_sample_rays(bhrt_lib):
    W, H, spp = 23, 7, 5
    bhrt_lib.stats(reset=True)
    _ss_device(bhrt_lib, "C2", W, H, abi.SupersamplingParams(spp, HALTON, 0.5))
    st = bhrt_lib.stats(reset=True)
    assert st["rays"] == W * H * spp and st["launches"] == 1, st


# 9. the separate colour pass ------------------------------------------------------------------
def test_separate_colour_pass_gives_the_same_frame(bhrt_lib, monkeypatch):
    ss = abi.SupersamplingParams(4, GRID, 1.0)
    fused = _ss_device(bhrt_lib, "C2", 40, 24, ss)
    monkeypatch.setenv("BHRT_FUSE_COLOUR", "0")
    separate = _ss_device(bhrt_lib, "C2", 40, 24, ss)
    _same(separate, fused, SS_FIELDS)
