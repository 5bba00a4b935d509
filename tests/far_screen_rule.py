"""The trace loop's disk screen (bhrt_trace_core.h disk_cand) as a rule on float64 operands, in
exact arithmetic: every product and FMA is the correctly rounded value of its exact result,
float(Fraction) -- here through integers, which is the same number (test_far_screen_cpu.py checks
the two against each other).

  screen_full   the one-mask screen: S = fma(sx, sx, RN(sy sy)) against both scaled thresholds,
                the sign test, and the unscreened pass of |den| >= 2^100;
  far_x, far_y  the far tests: RN(sx sx) > RN(out_sq d2) (RN(sy sy) > ...) and |den| < 2^100;
  screen        far_x, then far_y, then screen_full: what disk_cand computes;
  reference_decision  check_disk_intersection in the reference's expression order, numpy.

An operand set is (px, py, dx, dy, num, den, in_sq, out_sq): den and num are formed before the
screen and are inputs here. The sign of a zero is not kept (no comparison of the screen reads it).
"""
import math
from fractions import Fraction

import numpy as np

BIG = 2.0 ** 100
TINY = 2.0 ** -1000


def _split(x):
    m, e = math.frexp(x)
    return int(math.ldexp(m, 53)), e - 53


def _rn(n, e):
    """RN(n 2^e) for integers n, e: int / int and float(int) round to nearest, ties to even."""
    try:
        return n / (1 << -e) if e < 0 else float(n << e)
    except OverflowError:
        return math.inf if n > 0 else -math.inf


def fma(a, b, c):
    """RN(a b + c), one rounding. A non-finite operand gives what IEEE arithmetic gives."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        if math.isfinite(a) and math.isfinite(b):
            return c  # (a b is finite however large: no overflow before the sum)
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))
    (ma, ea), (mb, eb), (mc, ec) = _split(a), _split(b), _split(c)
    e = min(ea + eb, ec)
    return _rn(((ma * mb) << (ea + eb - e)) + (mc << (ec - e)), e)


def mul(a, b):
    return fma(a, b, 0.0)


def fma_fraction(a, b, c):
    """The same by float(Fraction), finite operands only."""
    try:
        return float(Fraction(a) * Fraction(b) + Fraction(c))
    except OverflowError:
        return math.inf if Fraction(a) * Fraction(b) + Fraction(c) > 0 else -math.inf


def terms(px, py, dx, dy, num, den, in_sq, out_sq):
    d2 = mul(den, den)
    sx = fma(dx, num, mul(px, den))
    sy = fma(dy, num, mul(py, den))
    return dict(d2=d2, sx=sx, sy=sy, sxx=mul(sx, sx), syy=mul(sy, sy), out=mul(out_sq, d2),
                inn=mul(in_sq, d2), sg=mul(den, fma(TINY, den, num)), small=abs(den) < BIG)


def decisions(*ops):
    """(far_x, far_y, screen_full) of one operand set"""
    t = terms(*ops)
    S = fma(t["sx"], t["sx"], t["syy"])
    full = (not (t["sg"] < 0.0) and S >= t["inn"] and S <= t["out"]) or not t["small"]
    return t["sxx"] > t["out"] and t["small"], t["syy"] > t["out"] and t["small"], full


def screen_full(*ops):
    return decisions(*ops)[2]


def far_x(*ops):
    return decisions(*ops)[0]


def far_y(*ops):
    return decisions(*ops)[1]


def screen(*ops):
    fx, fy, full = decisions(*ops)
    return False if fx or fy else full


# ---- the reference's decision and its thresholds -------------------------------------------

def sqrt_lower_bound(inner):
    """min {s : RN(sqrt(s)) >= inner} (scene.c)"""
    if np.isnan(inner):
        return np.nan
    if inner <= 0.0:
        return -np.inf
    s = np.float64(inner) * np.float64(inner)
    while s > 0.0 and np.sqrt(np.nextafter(s, 0.0)) >= inner:
        s = np.nextafter(s, 0.0)
    while np.sqrt(s) < inner:
        s = np.nextafter(s, np.inf)
    return float(s)


def sqrt_upper_bound(outer):
    """max {s : RN(sqrt(s)) <= outer} (scene.c)"""
    if np.isnan(outer):
        return np.nan
    if outer < 0.0:
        return -np.inf
    if np.isinf(outer):
        return np.inf
    s = np.float64(outer) * np.float64(outer)
    while np.sqrt(s) > outer:
        s = np.nextafter(s, 0.0)
    while not np.isinf(s) and np.sqrt(np.nextafter(s, np.inf)) <= outer:
        s = np.nextafter(s, np.inf)
    return float(s)


def reference_decision(p, d, n, inner, outer):
    """check_disk_intersection (raytracer.c:159-196) in numpy float64, the reference's
    expression order, nothing fused: IEEE quotient, |den| < 1e-10, t < 0, r in range.
    Returns (decision, r, den, num)."""
    with np.errstate(all="ignore"):
        den = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
        num = -((p[:, 0] * n[:, 0] + p[:, 1] * n[:, 1]) + p[:, 2] * n[:, 2])
        ok = ~(np.abs(den) < 1e-10)
        t = num / den
        ok &= ~(t < 0.0)
        qx = p[:, 0] + d[:, 0] * t
        qy = p[:, 1] + d[:, 1] * t
        r = np.sqrt(qx * qx + qy * qy)
        ok &= (r >= inner) & (r <= outer)
    return ok, r, den, num


# ---- the frames of tests/test_gpu_far_screen.py --------------------------------------------

W, H = 64, 36
SCENES = ("C2", "C4")
RADII = (7.0, 13.0)  # both rims inside every camera's picture
# name -> (position, up): looking at the origin. B and A are configs.CAMERAS'; "x" is B turned
# onto the +x axis (the second try, on y, decides 5 % of the tile-evaluations there,
# profiles/farscreen/screen_replay.txt), "diag" off both axes, A on the polar axis.
VIEWS = {"B": None, "A": None, "x": ((29.544, 0.0, 5.209), (0.0, 0.0, 1.0)),
         "diag": ((20.0, 20.0, 10.0), (0.0, 0.0, 1.0))}


def view(name):
    from bhrt import abi, configs
    if VIEWS[name] is None:
        return configs.camera(name)
    pos, up = VIEWS[name]
    return abi.Camera(abi.v3(*pos), abi.v3(*(-v for v in pos)), abi.v3(*up), 60.0)


def frame_scene(cname):
    """The configuration's scene with the disk's rims at RADII."""
    from bhrt import abi, configs
    c = configs.CONFIGS[cname]
    bh, _, cfg = c.scene()
    return c, bh, abi.disk(RADII[0], RADII[1], 1.0, 1.0), cfg
