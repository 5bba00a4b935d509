"""The far tests of the disk screen (bhrt_trace_core.h disk_cand) never reject a lane the one-mask screen
passes: the implication "far test true => screen false", checked by brute force on the exact rule
of tests/far_screen_rule.py (correctly rounded products and FMAs), and the frames of
tests/test_gpu_far_screen.py checked on the CPU, compiled reference against the oracle port.

The proof: RN(sy sy) >= 0, so sx sx + RN(sy sy) >= sx sx exactly; rounding is
monotone, so S = fma(sx, sx, RN(sy sy)) >= RN(sx sx) or S is NaN; either way S <= T is false
whenever RN(sx sx) > T. The same for sy: S >= RN(sy sy). With |den| < 2^100 required, the
unscreened pass does not apply."""
import math
import random

import numpy as np
import pytest

import far_screen_rule as rule
from conftest import full_frame_report, sky_pinned

IN_SQ, OUT_SQ = rule.sqrt_lower_bound(6.0), rule.sqrt_upper_bound(20.0)


def ulps(x, k):
    for _ in range(abs(k)):
        x = float(np.nextafter(x, math.inf if k > 0 else -math.inf))
    return x


def random_sets(count, seed=11):
    """Segments as the trace loop meets them: the previous point n 3..300 from the origin, the
    point p one step from it, a unit direction; den and num in the reference's order."""
    rng = np.random.default_rng(seed)

    def unit(k):
        v = rng.normal(size=(k, 3))
        return v / np.sqrt((v * v).sum(axis=1))[:, None]
    n = unit(count) * 10.0 ** rng.uniform(0.5, 2.5, size=(count, 1))
    p = n + 0.1 * unit(count)
    d = unit(count)
    _, _, den, num = rule.reference_decision(p, d, n, 6.0, 20.0)
    return [(p[i, 0], p[i, 1], d[i, 0], d[i, 1], num[i], den[i], IN_SQ, OUT_SQ)
            for i in range(count)]


def threshold_sets(count, seed=12):
    """sx sx (then sy sy) within a few ulp of out_sq d2, on both sides: the direction has no x
    (y) part, so sx = RN(px den), and px is stepped by -3..3 ulp around sqrt(out_sq) and
    around the two neighbours of that root whose squares straddle the threshold."""
    rnd = random.Random(seed)
    sets = []
    root = math.sqrt(OUT_SQ)
    while len(sets) < count:
        den = rnd.choice((1.0, -1.0)) * 2.0 ** rnd.randint(-40, 40) * rnd.uniform(1.0, 2.0)
        num = rnd.uniform(-50.0, 50.0)
        other = rnd.choice((0.0, rnd.uniform(-25.0, 25.0), rnd.uniform(-1.0, 1.0)))
        dother = rnd.uniform(-1.0, 1.0)
        for k in range(-3, 4):
            v = ulps(root, k) * rnd.choice((1.0, -1.0))
            sets.append((v, other, 0.0, dother, num, den, IN_SQ, OUT_SQ))   # x at the rim
            sets.append((other, v, dother, 0.0, num, den, IN_SQ, OUT_SQ))   # y at the rim
    return sets


def special_sets():
    """sy = 0; subnormal and huge den, |den| at and above 2^100; NaN and Inf in each operand."""
    nan, inf = math.nan, math.inf
    dens = [5e-324, 2.0 ** -1060, 2.0 ** -1022, 1e-10, 0.125, 3.0, 2.0 ** 99,
            ulps(2.0 ** 100, -1), 2.0 ** 100, ulps(2.0 ** 100, 1), 2.0 ** 101, 2.0 ** 300,
            2.0 ** 511, 2.0 ** 512, 2.0 ** 600, 1e308, inf]
    dens = [s * v for v in dens for s in (1.0, -1.0)] + [0.0, nan]
    nums = [0.0, 1.0, -1.0, 2.0 ** -1060, -2.0 ** -1060, 1e300, -1e300, nan, inf, -inf]
    points = [(8.0, 0.0, 0.0, 0.0), (0.0, 8.0, 0.0, 0.0), (300.0, 0.0, 0.0, 0.0),
              (0.0, 300.0, 0.0, 0.0), (300.0, 300.0, 0.3, 0.2), (8.0, 0.0, 0.3, 0.0),
              (1e200, 0.0, 0.0, 0.0), (0.0, 1e200, 0.0, 0.0), (1e-200, 1e-200, 1.0, 1.0),
              (nan, 8.0, 0.0, 0.0), (8.0, nan, 0.0, 0.0), (8.0, 1.0, nan, 0.0),
              (8.0, 1.0, 0.0, nan), (inf, 8.0, 0.0, 0.0), (8.0, -inf, 0.0, 0.0),
              (8.0, 1.0, inf, 0.0), (8.0, 1.0, 0.0, -inf), (inf, inf, inf, inf)]
    sets = [(px, py, dx, dy, num, den, IN_SQ, OUT_SQ)
            for den in dens for num in nums for (px, py, dx, dy) in points]
    for thr in ((nan, OUT_SQ), (IN_SQ, nan), (-inf, inf), (IN_SQ, inf), (0.0, 0.0),
                (1e-300, 1e-290), (1e300, 1e305)):
        for den in (0.125, -3.0, 2.0 ** -600, 2.0 ** 99, 2.0 ** 100):
            for (px, py, dx, dy) in points:
                sets.append((px, py, dx, dy, 1.0, den) + thr)
    return sets


def test_integer_fma_is_float_of_fraction():
    """rule.fma (exact integers, rounded once by int / int) = float(Fraction(a) Fraction(b) +
    Fraction(c)) on random and crafted finite operands: cancellation, subnormal and overflowing
    results, ties."""
    rnd = random.Random(5)
    cases = [(1.0 + 2.0 ** -52, 1.0 + 2.0 ** -52, -1.0), (2.0 ** -600, 2.0 ** -600, 0.0),
             (2.0 ** 600, 2.0 ** 600, 0.0), (-2.0 ** 600, 2.0 ** 600, 0.0), (3.0, 5e-324, 5e-324),
             (2.0 ** -1000, 2.0 ** 99, -1.0), (0.1, 10.0, -1.0), (0.0, 5.0, 0.0),
             (1.0 + 2.0 ** -52, 0.5, 2.0 ** -54), (1e308, 10.0, -1e308)]
    for _ in range(3000):
        e = [rnd.randint(-300, 300) for _ in range(3)]
        cases.append(tuple(rnd.uniform(-2.0, 2.0) * 2.0 ** k for k in e))
        a, b = rnd.uniform(-9.0, 9.0), rnd.uniform(-9.0, 9.0)
        cases.append((a, b, -a * b))  # the FMA's own rounding error
    for a, b, c in cases:
        assert rule.fma(a, b, c) == rule.fma_fraction(a, b, c), (a, b, c)


def test_far_test_true_implies_screen_false():
    """On >= 1e5 operand sets: a set the far test on x or on y rejects is one the one-mask screen
    rejects, so far_x, far_y, screen_full in sequence decide what screen_full alone decides."""
    groups = {"random": random_sets(68000), "threshold": threshold_sets(28000),
              "special": special_sets()}
    total = sum(len(g) for g in groups.values())
    assert total >= 100000, total
    seen = {g: [0, 0, 0, 0] for g in groups}  # far_x, far_y only, full rejects, full passes
    for g, sets in groups.items():
        for ops in sets:
            fx, fy, full = rule.decisions(*ops)
            assert not ((fx or fy) and full), (g, ops, fx, fy, full)
            seen[g][0 if fx else 1 if fy else 2 if not full else 3] += 1
    for ops in groups["special"][::7]:
        assert rule.screen(*ops) == rule.screen_full(*ops), ops
    print(total, "sets:", seen)
    for g in groups:  # every route decides in every group
        assert min(seen[g]) > 0, (g, seen[g])
    # the threshold sets do lie on both sides of the far test, through each component
    assert min(seen["threshold"][:2]) > 2000 and sum(seen["threshold"][2:]) > 2000
    # |den| at and above 2^100 passes unscreened however far the point lies
    assert rule.decisions(300.0, 0.0, 0.0, 0.0, 1.0, 2.0 ** 100, IN_SQ, OUT_SQ) == (False, False, True)
    assert rule.decisions(300.0, 0.0, 0.0, 0.0, 1.0, ulps(2.0 ** 100, -1), IN_SQ, OUT_SQ)[0]


@pytest.mark.parametrize("cname", rule.SCENES)
def test_frames_need_no_exemption_for_the_reference(oracle, cname):
    """The 64 x 36 frames of test_gpu_far_screen.py (four views, rims at RADII): the compiled
    reference and the oracle port agree on every ray, so the GPU test needs no knife-edge
    exemption; both classes are in every picture."""
    import oracle as orc
    from bhrt import abi
    ref = orc.reference()
    c, bh, dk, cfg = rule.frame_scene(cname)
    for name in rule.VIEWS:
        cam = rule.view(name)
        want, margin = oracle.render_frame_margin(bh, dk, cfg, cam, rule.W, rule.H, c.method,
                                                  c.flags, threads=16)
        got = ref.render_frame(bh, dk, cfg, cam, rule.W, rule.H, c.method, c.flags, threads=16)
        rep = full_frame_report(got, want, margin, sky_pinned(c.method))
        assert rep["mismatched_rays"] == 0, (cname, name, rep)
        disk = want["result"] == abi.RAY_DISK
        print(cname, name, "disk rays", int(disk.sum()), "min margin", rep["min_margin"])
        assert disk.sum() >= 40 and (~disk).sum() >= 40, (cname, name, int(disk.sum()))
