"""Adaptive supersampled frames (bhrt_render_frame_adaptive_device): the rule of
include/bhrt_api.h in numpy, the oracle's reference frames and the case table, shared by
test_adaptive_cpu.py and test_gpu_adaptive.py.

All frames use camera B and the whole image. Reference for a case: the oracle's M frames at the
offsets orc_jittered_offset(s, spp, method, strength), s = 0..M-1 (as test_gpu_supersample.py
builds its own), put through rule_frame below.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from conftest import KNIFE_EDGE
from bhrt import abi, configs

RTOL = 1e-5
THREADS = 16
GRID, HALTON = abi.JITTER_REGULAR_GRID, abi.JITTER_HALTON
RGB = ("rgb_r", "rgb_g", "rgb_b")

Case = namedtuple("Case", "name W H jm spp strength B M threshold edges")
# scene, W x H, jitter, spp, strength | B -> M | threshold | edge pixels on the oracle. The two
# sky-only scenes (C1, C5) have their threshold in the middle of the widest gap of the oracle's
# sorted edge values.
CASES = [
    Case("C2", 40, 24, GRID, 4, 1.0, 1, 4, 0.1, 134),
    Case("C2", 40, 24, GRID, 4, 1.0, 2, 4, 0.02, 520),
    Case("C2", 23, 7, HALTON, 5, 0.5, 2, 5, 0.05, 41),
    Case("C2", 40, 40, GRID, 4, 1.0, 1, 4, 0.1, 195),
    Case("C3", 32, 18, HALTON, 4, 1.0, 1, 4, 0.1, 136),
    Case("C4", 48, 27, GRID, 5, 1.0, 1, 5, 0.1, 219),
    Case("kerr099", 64, 36, GRID, 4, 1.0, 1, 4, 0.1, 217),   # 16 NaN base pixels
    Case("C1", 16, 16, GRID, 2, 1.0, 1, 2, 0.004134, 242),
    Case("C5", 32, 18, HALTON, 3, 0.75, 1, 3, 0.006673, 48),
]
CASE_IDS = [f"{c.name}-{c.W}x{c.H}-{c.B}to{c.M}-thr{c.threshold}" for c in CASES]
# (case, [(row_block, shards, pixels whose decision needs another shard's row)])
SHARD_CASES = [
    (CASES[7], [(3, 2, 18), (1, 2, 96)]),
    (CASES[8], [(1, 2, 48), (2, 3, 8)]),
    (CASES[3], [(8, 3, 0)]),      # shards of 16, 16 and 8 rows: the uneven indexing
]


def scene(name):
    """(bh, dk, cfg, method, flags)"""
    if name == "kerr099":  # the disk down to the ISCO of a = 0.99: hits at r_xy < 2 are NaN
        bh = abi.black_hole(1.0, 0.99)
        return (bh, abi.disk(bh.isco_radius, 20.0, 1.0, 1.0), abi.sim_config(0.1, 100.0, 1000, 1e-6),
                abi.INTEGRATOR_RK4, abi.BHRT_FLAG_DOPPLER)
    c = configs.CONFIGS[name]
    return c.scene() + (c.method, c.flags)


def params(case, threshold=None):
    """(SupersamplingParams, AdaptiveSamplingParams) of a case."""
    thr = case.threshold if threshold is None else threshold
    return (abi.SupersamplingParams(case.spp, case.jm, case.strength),
            abi.AdaptiveSamplingParams(1, case.B, case.M, 0.0, thr))


# ---- the rule ----
def base_colour(planes, B):
    """Step 1: ((0.0 + c_0) + ... + c_{B-1}) / B per channel; planes[s][f] are [H*W] arrays."""
    out = {}
    for f in RGB:
        acc = np.zeros_like(planes[0][f])
        for s in range(B):
            acc = acc + planes[s][f]
        out[f] = acc / B
    return out


def edge_value(base, W, H, row_block=None):
    """Step 2: g(p) over the 4-neighbours inside the image, [H*W]. With row_block, vertical
    neighbours in another row block are ignored (what a shard without a halo would compute)."""
    b = np.stack([base[f].reshape(H, W) for f in RGB], axis=0)
    g = np.zeros((H, W))

    def take(dst, src, same_block=None):
        with np.errstate(invalid="ignore"):
            d = np.abs(b[(slice(None),) + dst] - b[(slice(None),) + src])
            d = ((d[0] + d[1]) + d[2]) / 3.0
            raise_it = d > g[dst]          # (False for a NaN d)
            if same_block is not None:
                raise_it &= same_block
            g[dst] = np.where(raise_it, d, g[dst])

    every = slice(None)
    take((every, slice(1, None)), (every, slice(None, -1)))    # left neighbour
    take((every, slice(None, -1)), (every, slice(1, None)))    # right
    rows = np.arange(H)
    up = dn = None
    if row_block is not None:
        up = (rows[1:] // row_block == rows[:-1] // row_block)[:, None]
        dn = up
    take((slice(1, None), every), (slice(None, -1), every), up)     # the row above
    take((slice(None, -1), every), (slice(1, None), every), dn)     # the row below
    return g.reshape(-1)


def sample_counts(g, threshold, B, M):
    """Steps 3 and 4: trace_pixel's count with edge_factor = g > threshold ? 1.0 : 0.0."""
    with np.errstate(invalid="ignore"):
        factor = np.where(g > threshold, 1.0, 0.0)
    more = np.minimum(B + ((M - B) * factor).astype(np.int64), M)
    return np.where(factor > 0.5, more, B).astype(np.int32)


def rule_frame(planes, W, H, B, M, threshold):
    """The whole rule on M sample planes (dicts of result and RGB, [H*W]): result, RGB, samples
    and the edge values g."""
    g = edge_value(base_colour(planes, B), W, H)
    S = sample_counts(g, threshold, B, M)
    out = {"result": planes[0]["result"], "samples": S, "g": g}
    for f in RGB:
        acc = np.zeros(W * H)
        for s in range(M):                      # step 5: the running sum continued
            acc = np.where(s < S, acc + planes[s][f], acc)
        out[f] = acc / S
    return out


def shard_image_rows(H, row_block, shard, shards):
    """The image rows of a shard, in the shard's own row order."""
    return [y for y in range(H) if (y // row_block) % shards == shard]


# ---- the oracle's frames ----
def orc_offsets(oracle, ss, count):
    fn = oracle.lib.orc_jittered_offset
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    fn.restype = None
    out = []
    for s in range(count):
        ox, oy = C.c_double(0.5), C.c_double(0.5)
        if ss.samples_per_pixel > 1:
            fn(s, ss.samples_per_pixel, ss.jitter_method, ss.jitter_strength, C.byref(ox),
               C.byref(oy))
        out.append((ox.value, oy.value))
    return out


_cache = {}


def oracle_planes(oracle, case):
    """The oracle's M sample frames of a case and the smallest knife-edge margin of their rays;
    computed once per (scene, image, jitter), never modified."""
    key = (case.name, case.W, case.H, case.jm, case.spp, case.strength, case.M)
    if key not in _cache:
        bh, dk, cfg, method, flags = scene(case.name)
        ss = abi.SupersamplingParams(case.spp, case.jm, case.strength)
        planes, margin_min = [], np.inf
        for ox, oy in orc_offsets(oracle, ss, case.M):
            cam = configs.camera("B")
            cam.use_offset, cam.offset_x, cam.offset_y = 1, ox, oy
            plane, margin = oracle.render_frame_margin(bh, dk, cfg, cam, case.W, case.H, method,
                                                       flags, threads=THREADS)
            margin_min = min(margin_min, float(np.nanmin(margin)))
            keep = {f: plane[f].copy() for f in ("result",) + RGB}
            for v in keep.values():
                v.setflags(write=False)
            planes.append(keep)
        _cache[key] = (planes, margin_min)
    return _cache[key]


def oracle_frame(oracle, case, threshold=None):
    """rule_frame of the oracle's planes for a case (the reference frame), and the margin."""
    planes, margin_min = oracle_planes(oracle, case)
    assert margin_min >= KNIFE_EDGE, (case, margin_min)
    thr = case.threshold if threshold is None else threshold
    return rule_frame(planes, case.W, case.H, case.B, case.M, thr), margin_min
