"""The tail of the trace loop's iteration (bhrt_trace_core.h): the disk decision without a quotient
(disk_cand / disk_decide) and the one-correction square root of the segment length (seg_len).

  * frames whose disk rims cross many pixels, every ray against the oracle;
  * the decision itself on crafted operands (bhrt_check_disk_hit) against the reference's
    expression order in numpy;
  * seg_len's root (bhrt_check_seg_len) against numpy.sqrt.

Measured figures are in profiles/looptail/test_figures.txt.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import full_frame_report, sky_pinned
from bhrt import abi, configs

W, H = 128, 72
# (inner, outer): a wide ring, a narrow one, and a ring 1e-9 wide (inner = outer - 1e-9); with
# camera B every rim crosses several hundred of the 128 x 72 pixels
RADII = [(7.0, 13.0), (10.0, 10.5), (12.0 - 1e-9, 12.0)]
SCENES = ["C2", "C4", "C5"]
# knife-edge exemptions (conftest.full_frame_report: a mismatch on a ray whose oracle margin is
# below KNIFE_EDGE) the parent commit needed on these nine frames, measured on an MI355X: 0 each
PARENT_KNIFE_EDGE_MISMATCHES = 0


def _scene(cname, radii):
    """The configuration's scene with the disk's radii moved (C5, which has no disk, gets one)."""
    c = configs.CONFIGS[cname]
    bh, _, cfg = c.scene()
    return c, bh, abi.disk(radii[0], radii[1], 1.0, 1.0), cfg


@pytest.fixture(scope="module")
def oracle_frames(oracle):
    """The oracle's frame and knife-edge margins of every (scene, radii), computed once."""
    cache = {}

    def get(cname, radii):
        if (cname, radii) not in cache:
            c, bh, dk, cfg = _scene(cname, radii)
            cache[cname, radii] = oracle.render_frame_margin(
                bh, dk, cfg, configs.camera("B"), W, H, c.method, c.flags, threads=16)
        return cache[cname, radii]
    return get


@pytest.mark.parametrize("cname", SCENES)
def test_rim_frames_need_no_exemption_for_the_reference(oracle_frames, cname):
    """CPU: on the chosen radii the oracle and the compiled reference agree on every ray (so no
    knife-edge exemption is needed for the reference itself), and both rims are in the frame."""
    import oracle as orc
    ref = orc.reference()
    for radii in RADII:
        c, bh, dk, cfg = _scene(cname, radii)
        want, margin = oracle_frames(cname, radii)
        got = ref.render_frame(bh, dk, cfg, configs.camera("B"), W, H, c.method, c.flags,
                               threads=16)
        rep = full_frame_report(got, want, margin, sky_pinned(c.method))
        assert rep["mismatched_rays"] == 0, (cname, radii, rep)
        disk = want["result"] == abi.RAY_DISK
        if radii[1] - radii[0] > 1e-6:
            assert disk.sum() > 100 and (~disk).sum() > 100, (cname, radii, int(disk.sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("cname", SCENES)
def test_rim_frames_every_ray_vs_oracle(bhrt_lib, oracle_frames, cname):
    """128 x 72 camera-B frames of the C2, C4 and C5 scenes with the disk's rims moved into the
    picture (RADII): result and steps equal the oracle's on every ray, hit point, distance and
    colour within 1e-5; knife-edge exemptions at most the parent commit's on the same frames.
    Measured: parent 0 / 0 / 0, this kernel 0 / 0 / 0 mismatching rays (C2 / C4 / C5, three
    radius pairs each)."""
    for radii in RADII:
        c, bh, dk, cfg = _scene(cname, radii)
        got = bhrt_lib.render_frame(bh, dk, cfg, configs.camera("B"), W, H, c.method, c.flags)
        want, margin = oracle_frames(cname, radii)
        rep = full_frame_report(got, want, margin, sky_pinned(c.method))
        print(cname, radii, {k: rep[k] for k in ("mismatched_rays", "knife_edge_rays",
                                                 "mismatches_on_knife_edge", "unexplained")},
              "disk rays", int((want["result"] == abi.RAY_DISK).sum()))
        assert rep["unexplained"] == 0, (cname, radii, rep)
        assert rep["mismatches_on_knife_edge"] <= PARENT_KNIFE_EDGE_MISMATCHES, (cname, radii, rep)


# ---- the decision on crafted operands ---------------------------------------------------

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
    """check_disk_intersection (raytracer.c:159-196) in numpy float64, in the reference's
    expression order, nothing fused. Returns (decision, r)."""
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
    return ok, r


def gpu_decision(bhrt_lib, p, d, n, inner, outer):
    import torch
    L = bhrt_lib.load()
    L.bhrt_check_disk_hit.restype = C.c_int
    L.bhrt_check_disk_hit.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_double, C.c_double,
                                                         C.c_void_p, C.c_void_p]
    dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).ravel()).cuda()
           for a in (p, d, n)]
    cnt = len(p)
    out = torch.full((cnt,), -1, dtype=torch.int32, device="cuda")
    assert L.bhrt_check_disk_hit(*(t.data_ptr() for t in dev), cnt, sqrt_lower_bound(inner),
                                 sqrt_upper_bound(outer), out.data_ptr(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(bool)


INNER, OUTER = 6.0, 10.0


def special_operands():
    """Plane normal (0, 0, 1), so den = dz and num = -pz exactly whether or not the products are
    fused. den: around 1e-10 (the parallel test) and 1e150, zeros, NaN, Inf; num: zeros,
    +-2^-1060 (a quotient that underflows to +-0 for a large den), NaN, +-1. The candidate
    point is p's (8, 0) for a direction along z, and moves with t for an oblique one."""
    e, b = 1e-10, 1e150
    dens = []
    for v in (e, b):
        for w in (np.nextafter(v, 0.0), v, np.nextafter(v, np.inf)):
            dens += [w, -w]
    dens += [0.0, -0.0, np.nan, np.inf, -np.inf, 0.125, -0.125, 2.0 ** 100, -2.0 ** 100,
             2.0 ** 300, 2.0 ** 600, -2.0 ** 600]
    nums = [0.0, -0.0, 2.0 ** -1060, -2.0 ** -1060, np.nan, 1.0, -1.0, 2.0 ** -950, -2.0 ** -950]
    P, D, N = [], [], []
    for den in dens:
        for num in nums:
            for dxy in ((0.0, 0.0), (0.3, 0.2), (1e-12, 0.0)):
                P.append((8.0, 0.0, -num))
                D.append((dxy[0], dxy[1], den))
                N.append((0.0, 0.0, 1.0))
    return np.array(P), np.array(D), np.array(N)


def rim_operands(dens=(0.125, -0.125, 2.0, 2.0 ** -10)):
    """Candidate points whose s = qx^2 + qy^2 lies exactly on a threshold and one ulp either
    side: direction along z (q = p's x, y whatever t is), qy = the radius +- k ulp and qx =
    m 2^-23, whose square m^2 2^-46 is exact and a whole number of ulps of s in [64, 128), so
    fused and unfused sums agree. For a den that is a power of two the screen's products
    are exact scalings, so the decision is the reference's on the threshold itself."""
    P, D, N = [], [], []
    for radius in (INNER + 2.5, OUTER):  # 8.5^2 and 10^2 lie in [64, 128)
        for k in range(-4, 5):
            qy = radius
            for _ in range(abs(k)):
                qy = np.nextafter(qy, np.inf if k > 0 else 0.0)
            for m in range(0, 7):
                for den in dens:
                    P.append((m * 2.0 ** -23, qy, -1.0 if den > 0 else 1.0))
                    D.append((0.0, 0.0, den))
                    N.append((0.0, 0.0, 1.0))
    return np.array(P), np.array(D), np.array(N)


@pytest.mark.gpu
def test_disk_decision_on_special_operands(bhrt_lib):
    """The trace loop's disk decision equals the reference's on every special operand: den at
    +-1e-10 and +-1e150 and one ulp either side, +-0, NaN, Inf; num +-0, +-2^-1060, NaN; s
    exactly on disk_in_sq / disk_out_sq and one ulp on either side."""
    p, d, n = special_operands()
    want, _ = reference_decision(p, d, n, INNER, OUTER)
    got = gpu_decision(bhrt_lib, p, d, n, INNER, OUTER)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(p[i].tolist(), d[i].tolist(), bool(want[i])) for i in bad[:8]]
    assert want.any() and (~want).any()
    # t = -0.0 (num = +0, or an underflowed quotient) is accepted by the reference
    assert want[(p[:, 2] == 2.0 ** -1060) & (d[:, 2] == 1e150) & (d[:, 0] == 0.0)].all()

    inner, outer = INNER + 2.5, OUTER
    p, d, n = rim_operands()
    want, r = reference_decision(p, d, n, inner, outer)
    got = gpu_decision(bhrt_lib, p, d, n, inner, outer)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(p[i].tolist(), d[i].tolist(), bool(want[i])) for i in bad[:8]]
    s = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]
    for thr in (sqrt_lower_bound(inner), sqrt_upper_bound(outer)):
        for v in (np.nextafter(thr, 0.0), thr, np.nextafter(thr, np.inf)):
            assert (s == v).any(), (thr, v)  # the crafted set does land on it

    # the same points with a den whose products round (3, 1e-3): the screen may reject a point
    # on or one ulp inside a threshold, never accept one the reference rejects
    p, d, n = rim_operands((3.0, -3.0, 1e-3))
    want, r = reference_decision(p, d, n, inner, outer)
    got = gpu_decision(bhrt_lib, p, d, n, inner, outer)
    print("rim points, rounding den:", int((got != want).sum()), "of", len(p), "differ")
    assert not (got & ~want).any()
    assert not ((got != want) & ~near_rim(r, inner, outer)).any()


RANDOM_SEED = 7


def random_operands(seed=RANDOM_SEED, count=4096):
    """In-range triples: the previous path point n within 3..25 of the origin, the current point
    p one step (0.1) from it, a unit direction d."""
    rng = np.random.default_rng(seed)

    def unit(k):
        v = rng.normal(size=(k, 3))
        return v / np.sqrt((v * v).sum(axis=1))[:, None]
    n = unit(count) * rng.uniform(3.0, 25.0, size=(count, 1))
    p = n + 0.1 * unit(count)
    return p, unit(count), n


def near_rim(r, inner, outer, ulps=4):
    return (np.abs(r - inner) <= ulps * np.spacing(inner)) | \
           (np.abs(r - outer) <= ulps * np.spacing(outer))


def test_random_operands_are_clear_of_the_rims():
    """CPU: with RANDOM_SEED no random triple's r lies within 4 ulp of a radius (the reference
    against itself then has nothing to exempt), and both decisions occur."""
    p, d, n = random_operands()
    want, r = reference_decision(p, d, n, INNER, OUTER)
    assert near_rim(r, INNER, OUTER).sum() == 0
    assert want.sum() > 200 and (~want).sum() > 200


@pytest.mark.gpu
def test_disk_decision_on_random_operands(bhrt_lib):
    """4096 random in-range triples: the decision may differ from the reference's only where
    the reference's r is within 4 ulp of a radius, and such triples are < 1 % of the set
    (measured: 0 differences, 0 near a rim)."""
    p, d, n = random_operands()
    want, r = reference_decision(p, d, n, INNER, OUTER)
    got = gpu_decision(bhrt_lib, p, d, n, INNER, OUTER)
    near = near_rim(r, INNER, OUTER)
    diff = got != want
    print("random triples:", int(diff.sum()), "differ,", int(near.sum()), "within 4 ulp of a rim,",
          int(want.sum()), "hits")
    assert not (diff & ~near).any(), np.nonzero(diff & ~near)[0][:10]
    assert near.sum() < 0.01 * len(p)


# ---- seg_len's square root ---------------------------------------------------------------

@pytest.mark.gpu
def test_seg_len_root_within_one_ulp(bhrt_lib):
    """seg_len's root (rsq, Goldschmidt, ONE residual correction) on 1e5 arguments log-uniform in
    [2^-700, 2^600] and around the 2^-767 fallback boundary: <= 1 ulp from numpy.sqrt
    everywhere, bit-identical on >= 95 % (measured: see profiles/looptail/test_figures.txt)."""
    import torch
    L = bhrt_lib.load()
    L.bhrt_check_seg_len.restype = C.c_int
    L.bhrt_check_seg_len.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    rng = np.random.default_rng(3)
    x = 2.0 ** rng.uniform(-700.0, 600.0, size=100000)
    lim = 2.0 ** -767
    edge = [lim, np.nextafter(lim, 0.0), np.nextafter(lim, 1.0), 2.0 ** -768, 2.0 ** -766,
            2.0 ** -1022, 5e-324, 0.0, 1.0, 2.0, 4.0, 2.0 ** -700, 2.0 ** 600]
    x = np.concatenate([x, np.array(edge)])
    dx = torch.from_numpy(x).cuda()
    out = torch.full_like(dx, -1.0)
    assert L.bhrt_check_seg_len(dx.data_ptr(), len(x), out.data_ptr(),
                                C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    got, want = out.cpu().numpy(), np.sqrt(x)
    ulps = np.abs(got.view(np.int64) - want.view(np.int64))  # (all values >= 0: ordered as ints)
    same = float((ulps == 0).mean())
    print(f"seg_len root: max {int(ulps.max())} ulp, bit-identical {100.0 * same:.3f} %")
    assert ulps.max() <= 1, (x[ulps > 1][:5], got[ulps > 1][:5])
    assert (ulps[x < lim] == 0).all()  # the fallback's lanes
    assert same >= 0.95
