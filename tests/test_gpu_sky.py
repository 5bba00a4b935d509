"""Sky maps on the GPU (bhrt_sky_*, BHRT_FLAG_SKY): the bilinear lookup of an equirectangular
map where a ray leaves the scene. The rule is stated in include/bhrt_api.h ("Sky maps");
tests/sky_rule.py restates it in numpy.

Frames are checked against the COMPILED REFERENCE through tests/golden/sky_frames.npz
(gen_sky_frames.py): every pixel's trace_ray class and, for RAY_MAX_DISTANCE pixels, the last two
points of integrate_photon_path's path, whose difference is the exit chord. No pixel of the four
scenes is a knife-edge pixel on the oracle (the generator asserts it), so nothing is exempt.

Tolerances, on the smooth map (sky_rule.smooth_map: <= 0.25 per radian):
  chord pixels     1e-9 + 0.5 eps |p_k| / |chord|, eps = 1e-5 the project's float contract: each
                   of the two points may be off by eps |p|, which turns the chord by at most
                   2 eps |p_k| / |chord|, times 0.25 per radian;
  fallback pixels  1e-9 + 0.5 sqrt(3) 1e-15: the direction agreement of 1e-15 per component that
                   test_oracle_golden.py::test_numpy_camera_rays_match_the_oracle allows between
                   configs.camera_rays and the reference's directions, as an angle, times 0.25 --
                   below the 1e-9 floor conftest.compare uses.
The worst observed ratio to the tolerance goes to profiles/skymap/test_figures.txt.
"""
import os

import numpy as np
import pytest

from conftest import ROOT, camera_from, compare, golden, rays_from, scene_from
from bhrt import abi, configs
import sky_rule as sr

pytestmark = pytest.mark.gpu
RGB = ("rgb_r", "rgb_g", "rgb_b")
FRAME_FIELDS = ("result", "hit_x", "hit_y") + RGB + ("rgba32f", "rgba8")
SKY = abi.BHRT_FLAG_SKY
EPS = 1e-5
FALLBACK_TOL = 1e-9 + 0.5 * np.sqrt(3.0) * 1e-15
FIGURES = os.path.join(ROOT, "profiles", "skymap", "test_figures.txt")
W, H = 48, 27


def _figure(key, text):
    """One line per key in profiles/skymap/test_figures.txt, rewritten in place."""
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


_G = {}


def _fixture(k):
    """Scene k of sky_frames.npz: (bh, dk, cfg, cam, method, flags, result, last2, name)."""
    if "g" not in _G:
        _G["g"] = golden("sky_frames")
    g = {key[len(f"s{k}_"):]: v for key, v in _G["g"].items() if key.startswith(f"s{k}_")}
    bh, dk, cfg = scene_from(g)
    return (bh, dk, cfg, camera_from(g), int(g["method"]), int(g["flags"]), g["result"],
            g["last2"], str(g["name"]))


@pytest.fixture(scope="module")
def smooth_sky(bhrt_lib):
    """The smooth map on the device, made once for the module."""
    data = sr.smooth_map()
    data.setflags(write=False)
    sky = bhrt_lib.sky_create(data)
    yield data, sky
    bhrt_lib.sky_destroy(sky)   # (unbinds)


@pytest.fixture
def smooth(bhrt_lib, smooth_sky):
    """The smooth map, bound for the test (a test before it may have unbound it)."""
    bhrt_lib.set_sky(smooth_sky[1])
    return smooth_sky[0]


def _tensors(n, fields, fill=7):
    import torch
    dt = {"result": torch.int32, "steps": torch.int32, "rgba32f": torch.float32,
          "rgba8": torch.uint8}
    return {f: torch.full((n, 4) if f in abi.DISPLAY_FIELDS else (n,), fill,
                          dtype=dt.get(f, torch.float64), device="cuda") for f in fields}


def _frame(lib, k, flags_extra=SKY, rows=None, stream=None, offset=None, fields=FRAME_FIELDS):
    import torch
    bh, dk, cfg, cam, method, flags = _fixture(k)[:6]
    if offset is not None:
        cam.use_offset, cam.offset_x, cam.offset_y = 1, float(offset[0]), float(offset[1])
    n = W * (H if rows is None else lib.shard_rows(H, rows))
    t = _tensors(n, fields)
    torch.cuda.synchronize()
    lib.render_frame_device(bh, dk, cfg, cam, W, H, rows, method, flags | flags_extra,
                            lib.soa_from_tensors(t), stream)
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in t.items()}


def _same(a, b, fields, what=""):
    for f in fields:
        assert np.array_equal(a[f], b[f], equal_nan=True), (what, f)


def _check_colours(got_rgb, result, last2, dirs, data, what):
    """rgb [n, 3] of the sky pixels against the rule on the reference's chords / the ray
    directions; returns the worst ratio of |difference| to the pixel's tolerance."""
    chord = last2[:, 1] - last2[:, 0]
    vec, took = sr.vectors(result, chord, dirs)
    want = sr.lookup(data, vec)
    with np.errstate(invalid="ignore", divide="ignore"):
        lever = np.linalg.norm(last2[:, 1], axis=1) / np.linalg.norm(chord, axis=1)
    tol = np.where(took, 1e-9 + 0.5 * EPS * np.where(took, lever, 0.0), FALLBACK_TOL)
    sky = sr.uses_sky(result)
    diff = np.abs(got_rgb - want).max(axis=1)
    ratio = np.where(sky, diff / tol, 0.0)
    worst = int(np.argmax(ratio))
    print(f"{what}: {int(took.sum())} chord pixels (largest lever {np.nanmax(np.where(took, lever, 0)):.1f}), "
          f"{int((sky & ~took).sum())} fallback pixels; worst |diff| / tol = {ratio[worst]:.3e} at "
          f"pixel {worst} (diff {diff[worst]:.3e}, tol {tol[worst]:.3e}, chord {bool(took[worst])}); "
          f"worst fallback diff {np.max(np.where(sky & ~took, diff, 0.0)):.3e}")
    assert (ratio <= 1.0).all(), (what, worst, diff[worst], tol[worst])
    return float(ratio[worst]), int(took.sum()), int((sky & ~took).sum())


# 1. the sampler alone ---------------------------------------------------------------------------
def _directions():
    rng = np.random.default_rng(11)
    special = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                        [-1, 1e-300, 0], [-1, -1e-300, 0], [3, -4, 12], [-0.001, 0.002, 0.0005],
                        [1e150, -2e150, 0.5e150], [-3e149, 1e150, -1e150], [1e-150, 2e-150, -1e-150]],
                       dtype=np.float64)
    return np.concatenate([special, rng.normal(size=(130 - len(special), 3))])


@pytest.mark.parametrize("fmt", ["rgb32f", "rgba8"])
@pytest.mark.parametrize("size", [(1, 1), (2, 1), (4, 2), (64, 32)])
def test_sampler_against_the_rule(bhrt_lib, size, fmt):
    import torch
    w, h = size
    rng = np.random.default_rng(w * 100 + h)
    if fmt == "rgb32f":
        data = rng.random((h, w, 3), dtype=np.float32)
    else:
        data = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    sky = bhrt_lib.sky_create(data)
    try:
        st = bhrt_lib.sky_state(sky)
        assert (st["width"], st["height"]) == (w, h) and st["device"] == torch.cuda.current_device()
        assert st["format"] == (abi.BHRT_SKY_RGB32F if fmt == "rgb32f" else abi.BHRT_SKY_RGBA8)
        pool = _directions()
        worst = 0.0
        for n in (1, 63, 64, 65, 130):
            for start in ((0, 6, 10) if n == 1 else (0,)):   # (n = 1: an axis, the seam, a long one)
                d = np.ascontiguousarray(np.roll(pool, -start, axis=0)[:n])
                td = torch.tensor(d, dtype=torch.float64, device="cuda")
                out = torch.full((n, 3), 7.0, dtype=torch.float64, device="cuda")
                torch.cuda.synchronize()
                bhrt_lib.sky_lookup_device(sky, td.data_ptr(), n, out.data_ptr(), None)
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                want = sr.lookup(data, d)
                worst = max(worst, float(np.abs(got - want).max()))
                assert np.abs(got - want).max() <= 1e-9, (size, fmt, n, np.abs(got - want).max())
                host = bhrt_lib.sky_lookup(sky, d)
                assert np.array_equal(host, got), (size, fmt, n)
        print(f"sampler {w}x{h} {fmt}: max |device - rule| = {worst:.3e}")
        _figure(f"sampler {w}x{h} {fmt}", f"max |device - rule| {worst:.3e} (bound 1e-9)")
    finally:
        bhrt_lib.sky_destroy(sky)


def test_sampler_refusals_and_zero_vector(bhrt_lib):
    L = bhrt_lib.load()
    sky = bhrt_lib.sky_create(np.full((2, 4, 3), 0.5, dtype=np.float32))
    try:
        got = bhrt_lib.sky_lookup(sky, [[0, 0, 0], [np.nan, 1, 0], [1e200, 0, 0], [0, 0, 2]])
        assert np.array_equal(got[:3], np.zeros((3, 3))) and np.array_equal(got[3], [0.5] * 3)
        d = np.zeros(3)
        assert L.bhrt_sky_lookup(sky, d.ctypes.data, 0, d.ctypes.data) == -1
        assert "n 0" in bhrt_lib.last_error()
        assert L.bhrt_sky_lookup_device(sky, None, 1, d.ctypes.data, None) == -1
    finally:
        bhrt_lib.sky_destroy(sky)


# 2. frames against the reference ----------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_frames_against_the_reference(bhrt_lib, smooth, k):
    result, last2, name = _fixture(k)[6:]
    got = _frame(bhrt_lib, k)
    plain = _frame(bhrt_lib, k, flags_extra=0)
    assert np.array_equal(got["result"], result), np.nonzero(got["result"] != result)[0][:10]
    dirs = configs.camera_rays(_fixture(k)[3], W, H)["direction"]
    rgb = np.stack([got[f] for f in RGB], axis=1)
    worst, nchord, nfall = _check_colours(rgb, result, last2, dirs, smooth, name)
    _figure(f"frame {name}", f"{nchord} chord pixels, {nfall} fallback pixels, worst |diff| / tol "
            f"{worst:.3e}")
    assert np.array_equal(got["rgba32f"][:, :3], rgb.astype(np.float32), equal_nan=True)
    assert (got["rgba32f"][:, 3] == 1.0).all()
    assert np.array_equal(got["rgba8"], abi.rgba8_from_rgb(*(got[f] for f in RGB)))
    sky = sr.uses_sky(result)
    if sky.any():                    # (the map is in use: not the gradient)
        assert not np.array_equal(got["rgb_r"][sky], plain["rgb_r"][sky])
    # disk and horizon pixels: the flagless frame's colours within the colour contract here; bit
    # for bit in test_disk_and_horizon_pixels_keep_the_flagless_bits
    keep = ~sky
    compare({f: got[f][keep] for f in RGB}, {f: plain[f][keep] for f in RGB}, 1e-5, False, name,
            fields=RGB)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_disk_and_horizon_pixels_keep_the_flagless_bits(bhrt_lib, smooth, k):
    """Disk and horizon pixels of the frame with the flag equal the flagless frame bit for bit:
    the sky launch runs its own instantiation of the trace kernel, and its iterations must compile
    as the plain one's (the lookup is kept out of line for that: bhrt_colour.h colour_of_sky)."""
    result, _, name = _fixture(k)[6:]
    got = _frame(bhrt_lib, k)
    plain = _frame(bhrt_lib, k, flags_extra=0)
    keep = ~sr.uses_sky(result)
    bad = {f: int((~((got[f][keep] == plain[f][keep]) | ((got[f][keep] != got[f][keep]) &
                                                        (plain[f][keep] != plain[f][keep])))).sum())
           for f in RGB}
    print(f"{name}: disk / horizon pixels {int(keep.sum())}, differing from the flagless frame {bad}")
    for f in RGB + ("rgba32f", "rgba8"):
        assert np.array_equal(got[f][keep], plain[f][keep], equal_nan=True), (name, f)


# 3. ray arrays ----------------------------------------------------------------------------------
def _trace_rays_device(lib, rays, bh, dk, cfg, method, flags):
    import torch
    n = len(rays)
    d_rays = torch.tensor(np.ascontiguousarray(rays).view(np.float64).reshape(n, 6), device="cuda")
    t = _tensors(n, ("result", "hit_x", "hit_y") + RGB)
    torch.cuda.synchronize()
    rc = lib.load().bhrt_trace_rays_device(d_rays.data_ptr(), n, bh, dk, cfg, method, flags,
                                           lib.soa_from_tensors(t), None)
    assert rc == 0, lib.last_error()
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in t.items()}


@pytest.mark.parametrize("k", range(6))
def test_ray_arrays_against_the_stored_paths(bhrt_lib, smooth, k):
    g_all = golden("path_batch")
    g = {key[len(f"s{k}_"):]: v for key, v in g_all.items() if key.startswith(f"s{k}_")}
    name = str(g["name"])
    bh, dk, cfg = scene_from(g)
    rays = rays_from(g)
    method = int(g["method"])
    got = _trace_rays_device(bhrt_lib, rays, bh, dk, cfg, method, SKY)
    want_class = g["trace_result"] if dk is not None else g["res"][:, 2]
    assert np.array_equal(got["result"], want_class), (name, got["result"], want_class)
    n = len(rays)
    count = g["res"][:, 1]
    last2 = np.full((n, 2, 3), np.nan)
    for i in np.nonzero(want_class == abi.RAY_MAX_DISTANCE)[0]:
        last2[i] = g["path"][i, count[i] - 2:count[i]]
    rgb = np.stack([got[f] for f in RGB], axis=1)
    worst, nchord, nfall = _check_colours(rgb, want_class, last2, rays["direction"], smooth, name)
    _figure(f"rays {name}", f"{nchord} chord rays, {nfall} fallback rays, worst |diff| / tol "
            f"{worst:.3e}")
    if name in ("steps0", "leapfrog"):       # no iteration moves: the direction, whatever the class
        assert nchord == 0 and nfall == n
    if name == "rkf45_disk_stuck":           # stuck rays end on a repeated point: MAX_STEPS
        last = g["path"][np.arange(n), count - 1], g["path"][np.arange(n), count - 2]
        stuck = (want_class == abi.RAY_MAX_STEPS) & (last[0] == last[1]).all(axis=1)
        assert stuck.any()
        assert np.abs(rgb[stuck] - sr.lookup(smooth, rays["direction"][stuck])).max() <= FALLBACK_TOL


# 4. equalities ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_separate_colour_pass_gives_the_same_bits(bhrt_lib, smooth, monkeypatch, k):
    fused = _frame(bhrt_lib, k)
    monkeypatch.setenv("BHRT_FUSE_COLOUR", "0")
    separate = _frame(bhrt_lib, k)
    _same(separate, fused, FRAME_FIELDS, _fixture(k)[8])


def test_streams_and_repeats(bhrt_lib, smooth):
    import torch
    a = _frame(bhrt_lib, 0)
    b = _frame(bhrt_lib, 0)
    _same(a, b, FRAME_FIELDS, "twice")
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            c = _frame(bhrt_lib, 0, stream=s.cuda_stream)
        _same(a, c, FRAME_FIELDS, "torch stream")


@pytest.mark.parametrize("k", [0, 1])
def test_two_shards_reassemble_to_the_frame(bhrt_lib, smooth, k):
    B, S = 8, 2
    whole = _frame(bhrt_lib, k)
    built = {f: np.full_like(whole[f], 9) for f in FRAME_FIELDS}
    for s in range(S):
        rows = abi.Rows(B, s, S)
        shard = _frame(bhrt_lib, k, rows=rows)
        image_rows = [r for b in range(s, (H + B - 1) // B, S) for r in range(b * B, min((b + 1) * B, H))]
        for f in FRAME_FIELDS:
            tail = built[f].shape[1:]
            built[f].reshape((H, W) + tail)[image_rows] = shard[f].reshape((len(image_rows), W) + tail)
    _same(built, whole, FRAME_FIELDS, "2 shards")


def test_claim_order_changes_nothing(bhrt_lib, smooth):
    import torch
    a = _frame(bhrt_lib, 0)
    order = torch.tensor(np.random.default_rng(5).permutation(W * H).astype(np.int32), device="cuda")
    torch.cuda.synchronize()
    bhrt_lib.set_claim_order(order.data_ptr(), W * H)
    try:
        b = _frame(bhrt_lib, 0)
    finally:
        bhrt_lib.set_claim_order(None, 0)
    _same(a, b, FRAME_FIELDS, "claim order")


def test_without_the_flag_a_bound_sky_changes_nothing(bhrt_lib):
    for k in (0, 2):
        bhrt_lib.set_sky(None)
        bare = _frame(bhrt_lib, k, flags_extra=0)
        sky = bhrt_lib.sky_create(sr.smooth_map())
        try:
            bhrt_lib.set_sky(sky)
            bound = _frame(bhrt_lib, k, flags_extra=0)
        finally:
            bhrt_lib.sky_destroy(sky)
        _same(bare, bound, FRAME_FIELDS, _fixture(k)[8])


def test_the_flag_without_a_sky_is_refused_and_writes_nothing(bhrt_lib):
    import torch
    bhrt_lib.set_sky(None)
    bh, dk, cfg, cam, method, flags = _fixture(0)[:6]
    t = _tensors(W * H, FRAME_FIELDS)
    torch.cuda.synchronize()
    rc = bhrt_lib.load().bhrt_render_frame_device(bh, dk, cfg, cam, W, H, None, method,
                                                  flags | SKY, bhrt_lib.soa_from_tensors(t), None)
    torch.cuda.synchronize()
    assert rc == -1 and "no sky map is bound" in bhrt_lib.last_error()
    for v in t.values():
        assert bool((v == 7).all())
    with pytest.raises(bhrt_lib.BhrtError, match="no sky map is bound"):
        bhrt_lib.render_frame(bh, dk, cfg, cam, W, H, method, flags | SKY)


def test_host_frame_equals_device_frame(bhrt_lib, smooth, monkeypatch):
    monkeypatch.setenv("BHRT_MAX_DEVICES", "1")   # (a map serves one device: no multi-GPU split)
    bh, dk, cfg, cam, method, flags = _fixture(1)[:6]
    host = bhrt_lib.render_frame(bh, dk, cfg, cam, W, H, method, flags | SKY, fields=FRAME_FIELDS)
    _same(host, _frame(bhrt_lib, 1), FRAME_FIELDS, "host form")


# 5. composition ---------------------------------------------------------------------------------
GRID = abi.JITTER_REGULAR_GRID
SS_FIELDS = ("result",) + RGB + ("rgba32f", "rgba8")


def _ss(lib, k, ss, as_=None, adaptive=False):
    import torch
    bh, dk, cfg, cam, method, flags = _fixture(k)[:6]
    t = _tensors(W * H, SS_FIELDS)
    torch.cuda.synchronize()
    if adaptive:
        lib.render_frame_adaptive_device(bh, dk, cfg, cam, W, H, None, method, flags | SKY, ss, as_,
                                         lib.soa_from_tensors(t), None, None)
    else:
        lib.render_frame_ss_device(bh, dk, cfg, cam, W, H, None, method, flags | SKY, ss, as_,
                                   lib.soa_from_tensors(t), None)
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in t.items()}


@pytest.mark.parametrize("k", [0, 1])
def test_supersampled_and_adaptive_frames_compose(bhrt_lib, smooth, k):
    """The comparisons of test_gpu_supersample.py (the ss frame against the in-order mean of its
    single-offset frames: classes exact, colours at 1e-5, the measured deviation printed -- the
    sample rays and the camera rays are two compilations of one set-up) and test_gpu_adaptive.py
    (a negative threshold makes every pixel an edge pixel: the ss frame of max_samples, bit for
    bit)."""
    spp = 4
    ss = abi.SupersamplingParams(spp, GRID, 1.0)
    full = abi.AdaptiveSamplingParams(1, spp, spp, 0.0, 0.0)   # (the frame of spp samples)
    offsets = bhrt_lib.sample_offsets(ss, full)
    assert len(offsets) == spp
    planes = [_frame(bhrt_lib, k, offset=off) for off in offsets]
    got = _ss(bhrt_lib, k, ss, full)
    want = {"result": planes[0]["result"]}
    for f in RGB:
        acc = np.zeros(W * H)
        for p in planes:
            acc = acc + p[f]
        want[f] = acc / spp
    worst = compare(got, want, 1e-5, False, "ss with the flag", fields=("result",) + RGB)
    exact = all(np.array_equal(got[f], want[f], equal_nan=True) for f in RGB)
    print(f"scene {k}: ss frame vs the mean of its {spp} sky frames: bit-identical {exact}, max rel "
          f"deviation {worst:.2e}")
    assert not np.array_equal(got["rgb_r"], _ss_plain(bhrt_lib, k, ss)["rgb_r"])
    ad = _ss(bhrt_lib, k, ss, abi.AdaptiveSamplingParams(1, 1, spp, 0.0, -1.0), adaptive=True)
    _same(ad, got, SS_FIELDS, "adaptive, negative threshold")


def _ss_plain(lib, k, ss):
    import torch
    bh, dk, cfg, cam, method, flags = _fixture(k)[:6]
    t = _tensors(W * H, SS_FIELDS)
    torch.cuda.synchronize()
    lib.render_frame_ss_device(bh, dk, cfg, cam, W, H, None, method, flags, ss,
                               abi.AdaptiveSamplingParams(1, 4, 4, 0.0, 0.0),
                               lib.soa_from_tensors(t), None)
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in t.items()}


def test_one_accumulation_step_is_the_blend_of_the_sky_frame(bhrt_lib, smooth):
    """Step 1 of an accumulator: the single-offset sky frame's rgba32f through temporal_rule's
    blend, bit for bit (what test_own_frames_bit_for_bit_against_the_rule checks of every step)."""
    import torch
    import temporal_rule as tr
    k = 1
    bh, dk, cfg, cam, method, flags = _fixture(k)[:6]
    ss = abi.SupersamplingParams(4, GRID, 1.0)
    off = bhrt_lib.sample_offsets(ss)[0]
    frame = _frame(bhrt_lib, k, offset=off)["rgba32f"][:, :3]
    acc = bhrt_lib.accum_create(W, H, None, None)
    try:
        t = {"rgb": torch.full((W * H, 3), 7, dtype=torch.float32, device="cuda")}
        torch.cuda.synchronize()
        bhrt_lib.accum_frame_device(acc, bh, dk, cfg, cam, method, flags | SKY, ss,
                                    bhrt_lib.accum_out(t), None)
        torch.cuda.synchronize()
        got = t["rgb"].cpu().numpy()
    finally:
        bhrt_lib.accum_destroy(acc)
    rule = tr.Accumulator(W, H)
    rule.step(frame, cycle=4)
    assert np.array_equal(got.view(np.uint32), rule.acc.view(np.uint32))


def test_sky_demo_writes_a_picture(bhrt_lib, tmp_path):
    """examples/sky_demo.c end to end: a 160x90 PPM whose sky pixels are the star map, not the
    gradient, and the class counts of a C4 frame on stderr."""
    import subprocess
    from test_sky_cpu import build_sky_demo
    r = subprocess.run([build_sky_demo(tmp_path)], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    head = b"P6\n160 90\n255\n"
    assert r.stdout.startswith(head) and len(r.stdout) == len(head) + 160 * 90 * 3
    err = r.stderr.decode()
    assert "disk" in err and "max distance (sky lookup of the exit chord)" in err, err
    px = np.frombuffer(r.stdout[len(head):], dtype=np.uint8).reshape(90, 160, 3)
    assert (px[0] < 80).mean() > 0.8      # the top row is dark sky (the gradient would be bright)
    assert px.max() > 150                 # and the disk (or a star) is bright
