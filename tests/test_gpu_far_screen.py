"""The disk screen with its far tests first (bhrt_trace_core.h disk_cand): a segment whose candidate
point lies beyond the outer rim in x alone, or in y alone, is rejected before the rest of the
screen is formed. The decision must stay the reference's:

  * the decision itself (bhrt_check_disk_hit) on operands that each of the four routes decides
    -- x rejects, y rejects, the full screen rejects, the full screen passes -- on candidate
    points within 4 ulp of either rim along the x axis, the y axis and the diagonal, and on special
    values, against the reference's literal rule in numpy (tests/far_screen_rule.py);
  * 64 x 36 frames of the C2 and C4 scenes from four views, every ray against the oracle, no
    knife-edge exemption (tests/test_far_screen_cpu.py checks the frames on the CPU);
  * one k_paths batch whose hit records are the trace launch's.
"""
import ctypes as C
import math

import numpy as np
import pytest

import far_screen_rule as rule
from conftest import full_frame_report, sky_pinned
from bhrt import abi, configs

pytestmark = pytest.mark.gpu

INNER, OUTER = 8.5, 10.0  # 8.5^2 and 10^2 lie in [64, 128): one ulp of s is 2^-46 at both rims
Z = (0.0, 0.0, 1.0)       # the plane "normal": den = dz and num = -pz exactly, fused or not


def gpu_decision(bhrt_lib, p, d, n, inner, outer):
    import torch
    L = bhrt_lib.load()
    L.bhrt_check_disk_hit.restype = C.c_int
    L.bhrt_check_disk_hit.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_double, C.c_double,
                                                         C.c_void_p, C.c_void_p]
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()
           for a in (p, d, n)]
    out = torch.full((len(p),), -1, dtype=torch.int32, device="cuda")
    assert L.bhrt_check_disk_hit(*(t.data_ptr() for t in dev), len(p),
                                 rule.sqrt_lower_bound(inner), rule.sqrt_upper_bound(outer),
                                 out.data_ptr(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(bool)


def ulps(x, k):
    for _ in range(abs(k)):
        x = float(np.nextafter(x, math.inf if k > 0 else 0.0))
    return x


def s_forms_agree(qx, qy, in_sq, out_sq):
    """s = qx^2 + qy^2 decides the same against both thresholds however it is contracted: the
    reference's two products and a sum, or an FMA over either rounded square."""
    forms = (rule.mul(qx, qx) + rule.mul(qy, qy), rule.fma(qx, qx, rule.mul(qy, qy)),
             rule.fma(qy, qy, rule.mul(qx, qx)))
    return len({(s >= in_sq, s <= out_sq) for s in forms}) == 1


def route_operands():
    """A direction along z and a power-of-two den: the candidate point is p's (x, y) whatever t
    is, and the screen's products are exact scalings. Points far out in x, far out in y, in the
    hole, in the ring; each with t >= 0 and t < 0."""
    P, D = [], []
    xy = [(200.0, 0.0), (-200.0, 5.0), (10.5, 0.0), (1e150, 9.0),           # x rejects
          (0.0, 200.0), (9.0, -200.0), (0.0, 10.5), (-9.5, 1e150),          # y rejects
          (2.0, 1.0), (0.0, 0.0), (8.0, 8.0), (-7.5, 7.5), (6.0, -6.0),     # the full screen rejects
          (9.0, 0.0), (0.0, -9.5), (6.5, 6.5), (-6.2, 6.2), (8.5, 0.0)]     # ... passes (t >= 0)
    for x, y in xy:
        for den in (0.125, -0.125, 2.0, -2.0 ** -10, 2.0 ** 99, -2.0 ** 99, 2.0 ** 100, 2.0 ** 300):
            for pz in (-1.0, 1.0, 0.0):
                P.append((x, y, pz))
                D.append((0.0, 0.0, den))
    return np.array(P), np.array(D), np.tile(Z, (len(P), 1))


def rim_operands():
    """Candidate points within 4 ulp of a rim in |q_xy|, along the x axis (qx = the radius -4..4
    ulp, qy = m 2^-23: an exact square, a whole number of ulps of s), the y axis, and the
    diagonal (qx, qy = the radius / sqrt 2, each -4..4 ulp); only points whose s decides alike
    in every contraction (s_forms_agree), so the reference's unfused s, the screen's S and
    disk_decide's s cannot differ. Returns p, d, n and the axis of each case."""
    in_sq, out_sq = rule.sqrt_lower_bound(INNER), rule.sqrt_upper_bound(OUTER)
    pts = []
    for radius in (INNER, OUTER):
        for k in range(-4, 5):
            a = ulps(radius, k)
            for m in range(0, 5):
                pts.append(("x", a, m * 2.0 ** -23))
                pts.append(("x", -a, m * 2.0 ** -23))
                pts.append(("y", m * 2.0 ** -23, a))
                pts.append(("y", -m * 2.0 ** -23, -a))
            h = float(np.float64(radius) / np.sqrt(np.float64(2.0)))
            for j in range(-4, 5):
                pts.append(("diag", ulps(h, k), ulps(h, j)))
                pts.append(("diag", -ulps(h, k), ulps(h, j)))
    P, D, axis = [], [], []
    for ax, qx, qy in pts:
        if not s_forms_agree(qx, qy, in_sq, out_sq):
            continue
        for den in (0.125, -0.125, 2.0, 2.0 ** -10):
            P.append((qx, qy, -1.0 if den > 0 else 1.0))
            D.append((0.0, 0.0, den))
            axis.append(ax)
    return np.array(P), np.array(D), np.tile(Z, (len(P), 1)), np.array(axis)


def special_operands():
    """den around 1e-10 and 1e150, subnormal, at and above 2^100, zeros, NaN, Inf; num zeros,
    +-2^-1060, NaN, Inf, +-1; the point in the ring, far out in x, far out in y, NaN and Inf
    in a component; a direction along z and two oblique ones (a NaN or Inf part included)."""
    nan, inf = np.nan, np.inf
    dens = []
    for v in (1e-10, 1e150, 2.0 ** 100):
        for w in (np.nextafter(v, 0.0), v, np.nextafter(v, inf)):
            dens += [w, -w]
    dens += [0.0, -0.0, nan, inf, -inf, 0.125, -0.125, 5e-324, -2.0 ** -1060, 2.0 ** -1022,
             2.0 ** 101, 2.0 ** 300, 2.0 ** 600, -2.0 ** 600]
    nums = [0.0, -0.0, 2.0 ** -1060, -2.0 ** -1060, nan, inf, 1.0, -1.0, 2.0 ** -950]
    points = [(9.0, 0.0), (0.0, 9.0), (300.0, 0.0), (0.0, -300.0), (300.0, 300.0), (nan, 9.0),
              (9.0, nan), (inf, 0.0), (0.0, -inf)]
    dirs = [(0.0, 0.0), (0.3, 0.2), (1e-12, 0.0), (nan, 0.0), (0.0, inf)]
    P, D = [], []
    for den in dens:
        for num in nums:
            for x, y in points:
                for dx, dy in dirs:
                    P.append((x, y, -num))
                    D.append((dx, dy, den))
    return np.array(P), np.array(D), np.tile(Z, (len(P), 1))


def random_operands(count=2048, seed=3):
    """Oblique segments 3..300 from the origin, clear of both rims (the screen's S carries other
    roundings than the reference's s: within a few ulp of a rim they may differ)."""
    rng = np.random.default_rng(seed)

    def unit(k):
        v = rng.normal(size=(k, 3))
        return v / np.sqrt((v * v).sum(axis=1))[:, None]
    n = unit(count) * 10.0 ** rng.uniform(0.5, 2.5, size=(count, 1))
    p = n + 0.1 * unit(count)
    d = unit(count)
    _, r, _, _ = rule.reference_decision(p, d, n, INNER, OUTER)
    clear = (np.abs(r - INNER) > 1e-9) & (np.abs(r - OUTER) > 1e-9)
    return p[clear], d[clear], n[clear]


def test_disk_decision_by_every_route(bhrt_lib):
    """A few thousand cases in one launch; every decision equals the reference's."""
    groups = {"routes": route_operands(), "rims": rim_operands()[:3],
              "special": special_operands(), "random": random_operands()}
    p, d, n = (np.concatenate([g[i] for g in groups.values()]) for i in range(3))
    want, r, den, num = rule.reference_decision(p, d, n, INNER, OUTER)
    got = gpu_decision(bhrt_lib, p, d, n, INNER, OUTER)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(p[i].tolist(), d[i].tolist(), n[i].tolist(), bool(want[i]))
                           for i in bad[:8]]
    # each of the four routes decides some of the cases (the rule on the reference's den, num)
    in_sq, out_sq = rule.sqrt_lower_bound(INNER), rule.sqrt_upper_bound(OUTER)
    routes = [0, 0, 0, 0]
    for i in range(len(p)):
        fx, fy, full = rule.decisions(p[i, 0], p[i, 1], d[i, 0], d[i, 1], num[i], den[i], in_sq,
                                      out_sq)
        routes[0 if fx else 1 if fy else 2 if not full else 3] += 1
    print(len(p), "cases; x rejects, y rejects, screen rejects, screen passes:", routes,
          "hits", int(want.sum()))
    assert min(routes) >= 100, routes
    assert want.sum() >= 100

    # the rim cases lie on both sides of both rims along each axis, within 4 ulp, and both
    # decisions occur there
    rp, rd, rn, axis = rim_operands()
    rwant, rr, _, _ = rule.reference_decision(rp, rd, rn, INNER, OUTER)
    for ax in ("x", "y", "diag"):
        for rim in (INNER, OUTER):
            near = (axis == ax) & (np.abs(rr - rim) <= 4 * np.spacing(rim))
            assert (rr[near] < rim).any() and (rr[near] > rim).any() and (rr[near] == rim).any(), (ax, rim)
            assert rwant[near].any() and (~rwant[near]).any(), (ax, rim)
            assert near.sum() >= 36, (ax, rim, int(near.sum()))


@pytest.fixture(scope="module")
def oracle_frames(oracle):
    cache = {}

    def get(cname, name):
        if (cname, name) not in cache:
            c, bh, dk, cfg = rule.frame_scene(cname)
            cache[cname, name] = oracle.render_frame_margin(
                bh, dk, cfg, rule.view(name), rule.W, rule.H, c.method, c.flags, threads=16)
        return cache[cname, name]
    return get


@pytest.mark.parametrize("name", list(rule.VIEWS))
@pytest.mark.parametrize("cname", rule.SCENES)
def test_frames_every_ray_vs_oracle(bhrt_lib, oracle_frames, cname, name):
    """64 x 36 frames of the C2 and C4 scenes (rims at 7 and 13, in the picture) from camera B, a
    camera on the +x axis, a diagonal one and A on the polar axis: class and steps equal the
    oracle's, floats within 1e-5, on every ray -- no knife-edge ray is left out."""
    c, bh, dk, cfg = rule.frame_scene(cname)
    got = bhrt_lib.render_frame(bh, dk, cfg, rule.view(name), rule.W, rule.H, c.method, c.flags)
    want, margin = oracle_frames(cname, name)
    rep = full_frame_report(got, want, margin, sky_pinned(c.method))
    print(cname, name, {k: rep[k] for k in ("mismatched_rays", "knife_edge_rays")},
          "disk rays", int((want["result"] == abi.RAY_DISK).sum()))
    assert rep["mismatched_rays"] == 0, (cname, name, rep)


def test_paths_hit_records_equal_the_trace_launch(bhrt_lib):
    """One k_paths batch of 64 rays (an 8 x 8 crop of C2's camera-B frame across column 1248,
    where the disk test stops hitting on the first segments): the hit records are
    bhrt_trace_rays_device's for the same rays, bit for bit."""
    from test_gpu_paths import _trace_rays_device, run_device
    c = configs.CONFIGS["C2"]
    bh, dk, cfg = c.scene()
    rays = configs.camera_rays(configs.camera("B"), c.width, c.height).reshape(c.height, c.width)
    rays = np.ascontiguousarray(rays[500:508, 1244:1252]).reshape(-1)
    want = _trace_rays_device(bhrt_lib, rays, bh, dk, cfg, c.method)
    assert len({int(v) for v in want["result"]}) > 1, want["result"]
    got = run_device(bhrt_lib, rays, bh, dk, cfg, c.method, 1001, 1)
    for f in abi.PATH_HIT_FIELDS:
        assert np.array_equal(got[f], want[f], equal_nan=f not in ("result", "steps")), f
