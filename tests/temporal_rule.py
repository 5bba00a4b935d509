"""Temporal accumulation (bhrt_accum_*): the rule of include/bhrt_api.h in numpy float32, the case
table and the oracle's frames at each frame's offset, shared by test_temporal_cpu.py and
test_gpu_temporal.py.

All arithmetic below is float32 array arithmetic, one rounding per operation (numpy does not
contract). The gamma reference is float32(np.power(float64(c'), float64(float32(1) / float32(2.2))))
-- the float64 power, never numpy's float32 one, which may be a vector routine.

All cases use camera B and whole images. Frame k of a case is the plain frame at sample
k % cycle of the case's sample set (orc_jittered_offset, as adaptive_rule.py builds its planes).
"""
from collections import namedtuple

import numpy as np

from conftest import KNIFE_EDGE
from bhrt import abi, configs
import adaptive_rule as ar

F = np.float32
RGB = ar.RGB
GRID, HALTON = ar.GRID, ar.HALTON
REFERENCE, MEAN = abi.BHRT_ACCUM_REFERENCE, abi.BHRT_ACCUM_MEAN
GAMMA = np.float64(F(1) / F(2.2))
# OpenCL's 16-ulp bound for single-precision pow, the loosest a device powf can be, on a byte scale
POW_WIDTH = 255.0 * 16.0 * 2.0 ** -24
EXEMPT_SHARE = 0.002

Params = namedtuple("Params", "schedule blend_factor max_frames edge_threshold edge_decay")
DEFAULTS = Params(REFERENCE, F(0.1), 32, F(0.1), F(0.2))


def params(schedule=REFERENCE, blend_factor=0.1, max_frames=32, edge_threshold=0.1, edge_decay=0.2):
    return Params(schedule, F(blend_factor), int(max_frames), F(edge_threshold), F(edge_decay))


def abi_params(p):
    return abi.AccumParams(p.schedule, float(p.blend_factor), p.max_frames,
                           float(p.edge_threshold), float(p.edge_decay))


def alpha(p, frame_count):
    """Step 2."""
    if p.schedule == MEAN:
        return F(1) / F(frame_count + 1)
    if frame_count == 0:
        return F(1)
    if frame_count < 5:
        return F(0.5)
    return F(p.blend_factor)


def display(acc):
    """Step 6: (rgba8 [n][4], exempt [n][3]) -- exempt marks the channel values where a power
    within POW_WIDTH / 255 of ours may land on the other side of a byte boundary."""
    with np.errstate(invalid="ignore"):
        m = np.where(acc < F(1), acc, F(1))          # std::min(1.0f, c): NaN -> 1
        k = np.where(F(0) < m, m, F(0))              # std::max(0.0f, m): -0 -> 0
    g = np.power(k.astype(np.float64), GAMMA).astype(np.float32)
    v = g * F(255)
    out = np.full((acc.shape[0], 4), 255, dtype=np.uint8)
    out[:, :3] = v.astype(np.int32).astype(np.uint8)
    v64 = g.astype(np.float64) * 255.0
    exempt = (k > 0) & (k < 1) & (np.abs(v64 - np.rint(v64)) <= POW_WIDTH)
    return out, exempt


class Accumulator:
    """The state and one step of the rule for a W x H image (whole) or n pixels of a shard."""

    def __init__(self, W, H, p=DEFAULTS, n=None):
        self.W, self.H, self.p = W, H, p
        self.whole = n is None
        self.n = W * H if n is None else n
        self.acc = np.zeros((self.n, 3), dtype=np.float32)
        self.edge = np.zeros(self.n, dtype=np.float32)
        self.frame_count = self.jitter_index = self.frames_total = 0
        self.reset_pending = True

    def reset(self):
        self.reset_pending = True

    def next_alpha(self):
        return alpha(self.p, 0 if self.reset_pending else self.frame_count)

    def step(self, f, cycle=1):
        """Steps 1 to 6 with the new frame f [n][3] float32; returns (rgba8, exempt)."""
        f = np.asarray(f, dtype=np.float32).reshape(self.n, 3)
        if self.reset_pending:
            self.acc = np.zeros_like(self.acc)
            self.frame_count = 0
            self.reset_pending = False
        a = alpha(self.p, self.frame_count)
        w = F(1) - a
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            self.acc = self.acc * w + f * a
        assert self.acc.dtype == np.float32
        self.frame_count = min(self.frame_count + 1, self.p.max_frames)
        self.jitter_index = (self.jitter_index + 1) % cycle
        self.frames_total += 1
        if self.whole and self.W >= 3 and self.H >= 3:
            self._edges()
        return display(self.acc)

    def _edges(self):
        A = self.acc.reshape(self.H, self.W, 3)
        c = A[1:-1, 1:-1]
        g = np.zeros(c.shape[:2], dtype=np.float32)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            for nb in (A[:-2, 1:-1], A[2:, 1:-1], A[1:-1, :-2], A[1:-1, 2:]):  # up down left right
                d = np.abs(c - nb)
                s = ((F(0) + d[..., 0]) + d[..., 1]) + d[..., 2]
                s = s / F(3)
                g = np.where(s > g, s, g)                   # (False for a NaN d)
            E = self.edge.reshape(self.H, self.W).copy()
            dec = E[1:-1, 1:-1] - self.p.edge_decay
            E[1:-1, 1:-1] = np.where(g > self.p.edge_threshold, F(1),
                                     np.where(F(0) < dec, dec, F(0)))
        assert E.dtype == np.float32
        self.edge = E.reshape(-1)


# ---- the case table ----
Case = namedtuple("Case", "name W H jm spp frames threshold")
CASES = [
    Case("C2", 40, 24, HALTON, 8, 8, 0.1),      # covers alpha 1, 0.5 x4, 0.1 x3
    Case("C2", 23, 7, GRID, 4, 6, 0.1),
    Case("C3", 32, 18, HALTON, 4, 7, 0.1),
    Case("C4", 48, 27, GRID, 4, 8, 0.1),
    Case("kerr099", 64, 36, GRID, 4, 6, 0.1),   # the NaN pixels stay NaN and read 255
    Case("C1", 16, 16, GRID, 4, 6, 0.004),
    Case("C5", 32, 18, HALTON, 3, 6, 0.006),
]
CASE_IDS = [f"{c.name}-{c.W}x{c.H}-{'halton' if c.jm == HALTON else 'grid'}{c.spp}-{c.frames}f"
            for c in CASES]
# (case, rows {row_block, s, num_shards})
SHARD_CASES = [(Case("C2", 40, 40, GRID, 4, 6, 0.1), 8, 3),     # rows 16 / 16 / 8
               (Case("C1", 16, 16, GRID, 4, 6, 0.004), 3, 2)]


def case_params(case, schedule=REFERENCE):
    return params(schedule=schedule, edge_threshold=case.threshold)


def case_ss(case):
    return abi.SupersamplingParams(case.spp, case.jm, 1.0)


scene = ar.scene


# ---- the oracle's frames ----
_cache = {}


def oracle_frames(oracle, case):
    """The oracle's plain frames at the case's sample offsets, one per sample of the cycle, as
    float64 [n][3], and the smallest knife-edge margin of their rays; computed once per case,
    never modified. Frame k of the case is element k % cycle."""
    key = (case.name, case.W, case.H, case.jm, case.spp)
    if key not in _cache:
        bh, dk, cfg, method, flags = scene(case.name)
        frames, margin_min = [], np.inf
        for ox, oy in ar.orc_offsets(oracle, case_ss(case), case.spp):
            cam = configs.camera("B")
            cam.use_offset, cam.offset_x, cam.offset_y = 1, ox, oy
            plane, margin = oracle.render_frame_margin(bh, dk, cfg, cam, case.W, case.H, method,
                                                       flags, threads=ar.THREADS)
            margin_min = min(margin_min, float(np.nanmin(margin)))
            rgb = np.stack([plane[f] for f in RGB], axis=1).copy()
            rgb.setflags(write=False)
            frames.append(rgb)
        _cache[key] = (frames, margin_min)
    return _cache[key]


def oracle_run(oracle, case, schedule=REFERENCE):
    """The rule over the oracle's frames: per frame (acc, edge, rgba8, exempt), and the margin."""
    frames, margin_min = oracle_frames(oracle, case)
    assert margin_min >= KNIFE_EDGE, (case, margin_min)
    A = Accumulator(case.W, case.H, case_params(case, schedule))
    steps = []
    for k in range(case.frames):
        with np.errstate(invalid="ignore"):
            f = frames[k % case.spp].astype(np.float32)
        rgba8, exempt = A.step(f, case.spp)
        steps.append((A.acc.copy(), A.edge.copy(), rgba8, exempt))
    return steps, margin_min
