"""Adaptive supersampled camera frames (bhrt_render_frame_adaptive_device /
bhrt_render_frame_adaptive): min_samples per pixel, max_samples at the pixels the edge rule marks.
The rule is stated in include/bhrt_api.h; tests/adaptive_rule.py restates it in numpy and holds
the case table, on which test_adaptive_cpu.py::test_cases_are_decisive shows that no pixel's
decision is within the colour contract's error of its threshold -- so no pixel is excused here.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import compare
from bhrt import abi, configs
import adaptive_rule as ar
from adaptive_rule import RGB, RTOL

pytestmark = pytest.mark.gpu
FIELDS = ("result",) + RGB + ("rgba32f", "rgba8")
ALL = FIELDS + ("samples",)


def _tensors(n, fields, fill=7):
    import torch
    dt = {"result": torch.int32, "samples": torch.int32, "steps": torch.int32,
          "rgba32f": torch.float32, "rgba8": torch.uint8}
    return {f: torch.full((n, 4) if f in abi.DISPLAY_FIELDS else (n,), fill,
                          dtype=dt.get(f, torch.float64), device="cuda") for f in fields}


def _soa(lib, t):
    return lib.soa_from_tensors({f: v for f, v in t.items() if f != "samples"})


def _adaptive(lib, case, threshold=None, rows=None, fields=ALL, stream=None, as_=None):
    """One adaptive device frame of a case (a shard with rows): (numpy arrays, info)."""
    import torch
    bh, dk, cfg, method, flags = ar.scene(case.name)
    ss, a = ar.params(case, threshold)
    n = case.W * (case.H if rows is None else lib.shard_rows(case.H, rows))
    t = _tensors(n, fields)
    torch.cuda.synchronize()
    info = lib.render_frame_adaptive_device(bh, dk, cfg, configs.camera("B"), case.W, case.H, rows,
                                            method, flags, ss, as_ or a, _soa(lib, t),
                                            t["samples"].data_ptr() if "samples" in t else None,
                                            stream)
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in t.items()}, info


def _ss(lib, case, samples):
    """bhrt_render_frame_ss_device of the case's scene with `samples` samples per pixel (the
    first `samples` offsets of the case's jitter)."""
    import torch
    bh, dk, cfg, method, flags = ar.scene(case.name)
    ss, _ = ar.params(case)
    t = _tensors(case.W * case.H, FIELDS)
    torch.cuda.synchronize()
    lib.render_frame_ss_device(bh, dk, cfg, configs.camera("B"), case.W, case.H, None, method,
                               flags, ss, abi.AdaptiveSamplingParams(1, samples, samples, 0.0, 0.0),
                               lib.soa_from_tensors(t), None)
    torch.cuda.synchronize()
    return {f: v.cpu().numpy() for f, v in t.items()}


def _same(a, b, fields, what=""):
    for f in fields:
        assert np.array_equal(a[f], b[f], equal_nan=True), (what, f)


def _conversions(got):
    assert np.array_equal(got["rgba8"], abi.rgba8_from_rgb(*(got[f] for f in RGB)))
    rgb32 = np.stack([got[f] for f in RGB], axis=1).astype(np.float32)
    assert np.array_equal(got["rgba32f"][:, :3], rgb32, equal_nan=True)
    assert (got["rgba32f"][:, 3] == 1.0).all()


# 1. against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("case", ar.CASES, ids=ar.CASE_IDS)
def test_frame_vs_oracle(bhrt_lib, oracle, case):
    want, margin_min = ar.oracle_frame(oracle, case)
    got, info = _adaptive(bhrt_lib, case)
    edges = int((want["samples"] == case.M).sum())
    assert edges == case.edges
    bad = np.nonzero(got["samples"] != want["samples"])[0]
    assert bad.size == 0, (bad[:10], got["samples"][bad[:10]], want["g"][bad[:10]])
    worst = compare(got, want, RTOL, False, f"{case}", fields=("result",) + RGB)
    print(f"{case.name} {case.W}x{case.H} {case.B}->{case.M} thr {case.threshold}: oracle min "
          f"margin {margin_min:.2e}, edge pixels {edges}, NaN pixels "
          f"{int(np.isnan(want['rgb_r']).sum())}, max rel err {worst:.2e}")
    _conversions(got)
    n = case.W * case.H
    assert info == {"pixels": n, "edge_pixels": edges, "halo_pixels": 0,
                    "sample_rays": n * case.B + edges * (case.M - case.B)}


# 2. bit for bit against the supersampled frame ----------------------------------------------
@pytest.mark.parametrize("case", [ar.CASES[0], ar.CASES[5]], ids=["C2-40x24", "C4-48x27"])
def test_bit_for_bit_against_the_supersampled_frames(bhrt_lib, case):
    full, few = _ss(bhrt_lib, case, case.M), _ss(bhrt_lib, case, case.B)
    assert any(not np.array_equal(full[f], few[f], equal_nan=True) for f in RGB)
    n = case.W * case.H
    # a negative threshold: every pixel an edge, the frame of M samples
    got, info = _adaptive(bhrt_lib, case, threshold=-1.0)
    assert (got["samples"] == case.M).all() and info["edge_pixels"] == n
    _same(got, full, FIELDS, "threshold -1")
    # +inf and NaN: no edge, the frame of B samples in one launch
    for thr in (np.inf, np.nan):
        bhrt_lib.stats(reset=True)
        got, info = _adaptive(bhrt_lib, case, threshold=thr)
        st = bhrt_lib.stats(reset=True)
        assert (got["samples"] == case.B).all() and info["edge_pixels"] == 0
        assert st["launches"] == 1 and st["rays"] == n * case.B, st
        _same(got, few, FIELDS, f"threshold {thr}")
    # the case's own threshold: each pixel is the frame's of its own sample count
    got, info = _adaptive(bhrt_lib, case)
    edge = got["samples"] == case.M
    assert ((got["samples"] == case.B) | edge).all() and 0 < edge.sum() < n
    assert info["edge_pixels"] == edge.sum() == case.edges
    for f in FIELDS:
        e = edge[:, None] if got[f].ndim == 2 else edge
        assert np.array_equal(got[f], np.where(e, full[f], few[f]), equal_nan=True), f


def test_min_equals_max_is_that_frame_in_one_launch(bhrt_lib):
    case = ar.CASES[0]
    a = abi.AdaptiveSamplingParams(1, 3, 3, 0.0, 0.1)
    bhrt_lib.stats(reset=True)
    got, info = _adaptive(bhrt_lib, case, as_=a)
    st = bhrt_lib.stats(reset=True)
    assert (got["samples"] == 3).all() and st["launches"] == 1
    assert info["sample_rays"] == st["rays"] == case.W * case.H * 3 and info["edge_pixels"] > 0
    _same(got, _ss(bhrt_lib, case, 3), FIELDS)


# 3. shards ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,row_block,shards",
                         [(c, rb, s) for c, lst in ar.SHARD_CASES for rb, s, _ in lst],
                         ids=[f"{c.name}-{c.W}x{c.H}-block{rb}-of{s}"
                              for c, lst in ar.SHARD_CASES for rb, s, _ in lst])
def test_shards_reassemble_to_the_frame(bhrt_lib, case, row_block, shards):
    whole, winfo = _adaptive(bhrt_lib, case)
    built = {f: np.full_like(whole[f], 9) for f in ALL}
    edges = 0
    for k in range(shards):
        rows = abi.Rows(row_block, k, shards)
        image_rows = ar.shard_image_rows(case.H, row_block, k, shards)
        shard, info = _adaptive(bhrt_lib, case, rows=rows)
        assert info["pixels"] == len(image_rows) * case.W and info["halo_pixels"] > 0
        # (ext rows: the shard's own and every image row next to one of them)
        near = {y + d for y in image_rows for d in (-1, 0, 1) if 0 <= y + d < case.H}
        assert info["halo_pixels"] == (len(near) - len(image_rows)) * case.W
        assert info["sample_rays"] == (len(near) * case.W * case.B +
                                       info["edge_pixels"] * (case.M - case.B))
        edges += info["edge_pixels"]
        for r, y in enumerate(image_rows):
            for f in ALL:
                built[f][y * case.W:(y + 1) * case.W] = shard[f][r * case.W:(r + 1) * case.W]
    assert edges == winfo["edge_pixels"] == case.edges
    _same(built, whole, ALL)


# 4. determinism and streams -------------------------------------------------------------------
def test_same_frame_twice_and_on_any_stream(bhrt_lib):
    import torch
    case = ar.CASES[0]
    a, ia = _adaptive(bhrt_lib, case)
    b, ib = _adaptive(bhrt_lib, case)
    _same(a, b, ALL, "twice")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c, ic = _adaptive(bhrt_lib, case, stream=s.cuda_stream)
    _same(a, c, ALL, "torch stream")
    assert ia == ib == ic
    rows = abi.Rows(3, 1, 2)
    with torch.cuda.stream(s):
        d, _ = _adaptive(bhrt_lib, case, rows=rows, stream=s.cuda_stream)
    e, _ = _adaptive(bhrt_lib, case, rows=rows)
    _same(d, e, ALL, "shard on a torch stream")


def test_null_stream_orders_after_default_stream_fills(bhrt_lib):
    """Outputs poison-filled on the default stream behind a busy kernel, no sync before the
    NULL-stream call, read back on the default stream: the frame, not the fill."""
    import torch
    assert torch.cuda.current_stream().cuda_stream == 0
    case = ar.CASES[0]
    want, _ = _adaptive(bhrt_lib, case)
    bh, dk, cfg, method, flags = ar.scene(case.name)
    ss, a = ar.params(case)
    t = _tensors(case.W * case.H, ALL, fill=0)
    torch.cuda.synchronize()  # (allocation done; everything below stays queued)
    sleep = getattr(torch.cuda, "_sleep", None)
    if sleep is not None:
        sleep(20_000_000)
    else:
        m = torch.ones(2048, 2048, device="cuda")
        for _ in range(8):
            m = m @ m * 1e-3
    for v in t.values():
        v.fill_(3)
    bhrt_lib.render_frame_adaptive_device(bh, dk, cfg, configs.camera("B"), case.W, case.H, None,
                                          method, flags, ss, a, _soa(bhrt_lib, t),
                                          t["samples"].data_ptr(), None)
    got = {f: v.cpu().numpy() for f, v in t.items()}
    _same(got, want, ALL)


# 5. host form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fields", [("rgba8",), FIELDS])
def test_host_frame_equals_device_frame(bhrt_lib, fields):
    case = ar.CASES[0]
    bh, dk, cfg, method, flags = ar.scene(case.name)
    ss, a = ar.params(case)
    host = bhrt_lib.render_frame_adaptive(bh, dk, cfg, configs.camera("B"), case.W, case.H, method,
                                          flags, ss, a, fields=fields)
    dev, info = _adaptive(bhrt_lib, case, fields=fields + ("samples",))
    assert tuple(host) == tuple(fields) + ("samples", "info")
    _same(host, dev, fields + ("samples",))
    assert host["info"] == info and info["edge_pixels"] == case.edges


# 6. statistics --------------------------------------------------------------------------------
def test_stats_count_both_launches(bhrt_lib):
    case = ar.CASES[8]   # C5 32x18, 1 -> 3
    bhrt_lib.stats(reset=True)
    _, info = _adaptive(bhrt_lib, case)
    st = bhrt_lib.stats(reset=True)
    n, E = case.W * case.H, case.edges
    assert info["edge_pixels"] == E
    assert st["rays"] == n * case.B + E * (case.M - case.B) == info["sample_rays"], st
    assert st["launches"] == 2, st
    rows = abi.Rows(1, 0, 2)   # 9 own rows, 9 halo rows
    _, info = _adaptive(bhrt_lib, case, rows=rows)
    st = bhrt_lib.stats(reset=True)
    owned, halo = 9 * case.W, 9 * case.W
    assert (info["pixels"], info["halo_pixels"]) == (owned, halo)
    assert st["rays"] == (owned + halo) * case.B + info["edge_pixels"] * (case.M - case.B), st
    assert st["launches"] == 2 and info["edge_pixels"] > 0, st


# 7. the separate colour pass ------------------------------------------------------------------
def test_separate_colour_pass_gives_the_same_frame(bhrt_lib, monkeypatch):
    case = ar.CASES[0]
    fused, _ = _adaptive(bhrt_lib, case)
    sharded, _ = _adaptive(bhrt_lib, case, rows=abi.Rows(3, 0, 2))
    monkeypatch.setenv("BHRT_FUSE_COLOUR", "0")
    separate, _ = _adaptive(bhrt_lib, case)
    _same(separate, fused, ALL)
    separate, _ = _adaptive(bhrt_lib, case, rows=abi.Rows(3, 0, 2))
    _same(separate, sharded, ALL, "shard")


# 8. refusals ----------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["as NULL", "adaptive off", "B = 0", "M < B", "M = 65", "steps",
                                  "random", "use_offset", "rgb_r alone"])
def test_bad_arguments_are_refused_and_write_nothing(bhrt_lib, what):
    import torch
    L = bhrt_lib.load()
    W, H = 16, 8
    bh, dk, cfg, method, flags = ar.scene("C2")
    cam = configs.camera("B")
    ss = abi.SupersamplingParams(4, ar.GRID, 1.0)
    a = abi.AdaptiveSamplingParams(1, 1, 4, 0.0, 0.1)
    fields = FIELDS
    if what == "as NULL":
        a = None
    elif what == "adaptive off":
        a = abi.AdaptiveSamplingParams(0, 1, 4, 0.0, 0.1)
    elif what == "B = 0":
        a = abi.AdaptiveSamplingParams(1, 0, 4, 0.0, 0.1)
    elif what == "M < B":
        a = abi.AdaptiveSamplingParams(1, 3, 2, 0.0, 0.1)
    elif what == "M = 65":
        a = abi.AdaptiveSamplingParams(1, 1, 65, 0.0, 0.1)
    elif what == "steps":
        fields = FIELDS + ("steps",)
    elif what == "random":
        ss = abi.SupersamplingParams(4, abi.JITTER_RANDOM, 1.0)
    elif what == "use_offset":
        cam.use_offset, cam.offset_x, cam.offset_y = 1, 0.25, 0.25
    elif what == "rgb_r alone":
        fields = ("result", "rgb_r")
    t = _tensors(W * H, fields + ("samples",))
    host, host_soa = abi.alloc_soa(W * H, fields)
    host_samples = np.full(W * H, 7, dtype=np.int32)
    for v in host.values():
        v[...] = 7
    torch.cuda.synchronize()
    soa = _soa(bhrt_lib, t)
    pa = C.byref(a) if a is not None else None
    info = abi.AdaptiveInfo(7, 7, 7, 7)
    assert L.bhrt_render_frame_adaptive_device(C.byref(bh), C.byref(dk), C.byref(cfg),
                                               C.byref(cam), W, H, None, method, flags,
                                               C.byref(ss), pa, C.byref(soa),
                                               t["samples"].data_ptr(), C.byref(info), None) == -1
    assert bhrt_lib.last_error()
    assert L.bhrt_render_frame_adaptive(C.byref(bh), C.byref(dk), C.byref(cfg), C.byref(cam), W, H,
                                        method, flags, C.byref(ss), pa, C.byref(host_soa),
                                        host_samples.ctypes.data, C.byref(info)) == -1
    assert bhrt_lib.last_error()
    torch.cuda.synchronize()
    for f in fields + ("samples",):
        assert (t[f].cpu().numpy() == 7).all(), f
    for f in fields:
        assert (host[f] == 7).all(), f
    assert (host_samples == 7).all() and info.pixels == 7 and info.edge_pixels == 7
