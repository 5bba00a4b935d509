"""Narrow-first shifts at far-anchor sites of the RK4 a = 0 iteration (bhrt_trace_core.h
BHRT_NARROW_SITES): stage 2's and stage 4's theta and the advance of state[3] take
shift_chain<2>'s two coefficients on |delta| <= 1/64 first, and a lane beyond the bound redoes
the shift with shift_or_eval.

  * the two-coefficient shift on given operands (bhrt_check_shift_chain, site 0 -- the very
    function the sites now call): its polynomials seen through operands that expose them,
    against long-double sin / cos; outside the bound, and for NaN, Inf and a near 0, the bits of
    shift_or_eval;
  * ten 64 x 36 frames against the oracle with NO ray left out: class and steps equal on every
    ray, floats within the parity tests' tolerance;
  * the same frame through the camera kernel and as a ray array. The two set-ups round a ray's
    initial velocities one ulp apart (two compilations of the same normalisation, DESIGN.md
    section 11; so on the parent too), so bit identity between them is not there to be had:
    classes and steps are equal and floats within 1e-9, as tests/test_gpu_stage_pairs.py holds
    the same pair. That a ray's bits depend on its operands alone is checked where the operands
    ARE the same: the ray array traced whole and in part, with other wave-mates.

Bounds of the operand test. tools/shift_poly_fit.py 0.015625 prints the truncation error of the
two-coefficient polynomials on |delta| <= 1/64 in exact arithmetic: FIT_SIN = 1.19e-18 for
sin(delta), FIT_COS = 1.69e-21 for cos(delta) - 1. A double cannot hold either value that well,
so the device's results carry their own roundings on top, each bounded here from the format:
  sd  = fma(z delta, p, delta) is rounded once, <= ulp(sd) / 2 <= 2^-53 |delta|; its inner term
        (z delta) p, of magnitude <= |delta|^3 / 6 <= 4.1e-5 |delta|, carries three roundings,
        <= 3 * 2^-53 * 4.1e-5 |delta|; together <= 2^-53 |delta| (1 + 1.3e-4);
  cm1 = z * fma(z, q, -1/2), three roundings on a value of magnitude <= delta^2 / 2:
        <= 3 * 2^-53 * delta^2 / 2.
The check kernel hands out sin and cos of x, not sd and cm1; from the anchor a = 0 with s0 = 0,
c0 = 1 its closing FMAs give s = sd exactly and c = RN(1 + cm1), a value in (1/2, 1] whose last
rounding is <= 2^-54; from s0 = 1, c0 = 0 they give s = RN(1 + cm1) and c = -sd. The long-double
reference (64-bit mantissa) is within 2^-63 of the true values' magnitude. Measured figures:
profiles/nursery/test_figures.txt.
"""
import numpy as np
import pytest

from conftest import compare, sky_pinned
from bhrt import abi, configs
from test_gpu_parity import RTOL
from test_gpu_shift_chain import _check_site, _rows, _same_bits, _shift_chain, special_operands

T = 1.0 / 64.0
FIT_SIN, FIT_COS = 1.19e-18, 1.69e-21  # tools/shift_poly_fit.py 0.015625, two coefficients
U = 2.0 ** -53
W, H = 64, 36
# tests/test_gpu_shift_chain.py's cameras, as values: position (looking at the origin, up +z), fov.
# Every camera some 30 away has lanes beyond 1/64 at the far-anchor sites in its rays' first
# iterations ("polar" and "rims" are checked below); "horizon", whose steps are tiny, has none.
CAMS = {"rims": ((3.1, -29.2, 5.3), 60.0), "far": ((5.1, -33.0, 7.7), 50.0),
        "horizon": ((0.2925, -2.0268, 0.4179), 90.0),
        "polar": ((1.4508, -2.3212, 28.8705), 50.0),
        "chain": ((5.1042, -33.0313, 7.7051), 100.0)}
FRAMES = [(c, cam) for c in ("C2", "C1") for cam in CAMS]


def _camera(name):
    p, fov = CAMS[name]
    return abi.Camera(abi.v3(*p), abi.v3(*[-x for x in p]), abi.v3(0.0, 0.0, 1.0), fov)


def _eps(seed=41, count=4096):
    """delta over [-1/64, 1/64]: half uniform, half log-uniform down to 1e-12 / 64, and the
    bound itself with either sign."""
    rng = np.random.default_rng(seed)
    e = rng.uniform(-T, T, count)
    e[1::2] = T * 10.0 ** rng.uniform(-12.0, 0.0, count // 2) * rng.choice([-1.0, 1.0], count // 2)
    return np.concatenate([e, [T, -T]])


@pytest.mark.gpu
def test_two_coefficient_polynomials_within_the_fit(bhrt_lib):
    """sin(delta) and 1 + (cos(delta) - 1) as the narrow form computes them, exposed by the
    anchors (0; 0, 1) and (0; 1, 0), within the fit's figures plus the roundings a double adds."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "long double is not wider than double here"
    e = _eps()
    n = len(e)
    zero = np.zeros(n)
    ops = np.concatenate([np.stack([zero, zero, zero + 1.0, e], axis=1),    # s = sd, c = RN(1 + cm1)
                          np.stack([zero, zero + 1.0, zero, e], axis=1)])   # s = RN(1 + cm1), c = -sd
    out = _shift_chain(bhrt_lib, ops, 0)
    assert (out[:, 4] == 1.0).all()  # every |delta| <= 1/64 keeps the narrow form
    el = e.astype(np.longdouble)
    sin_t, cos_t = np.sin(el), np.cos(el)
    ref = 2.0 ** -63
    bound_s = FIT_SIN + U * np.abs(e) * (1.0 + 1.3e-4) + ref * np.abs(e)
    bound_c = FIT_COS + 3.0 * U * e * e / 2.0 + 2.0 ** -54 + ref
    err_s = np.maximum(np.abs(out[:n, 0].astype(np.longdouble) - sin_t),
                       np.abs(-out[n:, 1].astype(np.longdouble) - sin_t)).astype(np.float64)
    err_c = np.maximum(np.abs(out[:n, 1].astype(np.longdouble) - cos_t),
                       np.abs(out[n:, 0].astype(np.longdouble) - cos_t)).astype(np.float64)
    # sd beside the fit's figure alone, with the final rounding of sd taken off: the distance of
    # the true sine from the double nearest to it is what no double result can avoid
    nearest = np.abs(sin_t.astype(np.float64).astype(np.longdouble) - sin_t).astype(np.float64)
    print(f"narrow shift on {n} deltas in [-1/64, 1/64]: worst |sd - sin| {err_s.max():.4e} "
          f"(bound at that delta {bound_s[err_s.argmax()]:.4e}; fit {FIT_SIN:.3e}); worst excess "
          f"over the nearest double {np.max(err_s - nearest):.4e}; worst |RN(1 + cm1) - cos| "
          f"{err_c.max():.4e} (bound {bound_c[err_c.argmax()]:.4e}; fit {FIT_COS:.3e})")
    assert (err_s <= bound_s).all(), (float(e[np.argmax(err_s - bound_s)]), float(err_s.max()))
    assert (err_c <= bound_c).all(), (float(e[np.argmax(err_c - bound_c)]), float(err_c.max()))
    # both anchors expose the same sd and the same 1 + cm1
    assert _same_bits(out[:n, 0], -out[n:, 1]) and _same_bits(out[:n, 1], out[n:, 0])


@pytest.mark.gpu
def test_beyond_the_bound_is_shift_or_eval(bhrt_lib):
    """Operands straddling 1/64 (the bound and one ulp either side), beyond it up to the wide
    and the direct forms' ranges, NaN and Inf in x, and a near 0 where x - a is inexact: the
    narrow flag is |x - a| <= 1/64 as the double subtraction gives it, and a lane without it has
    shift_or_eval's bits."""
    rng = np.random.default_rng(43)
    count = 2048
    a = 10.0 ** rng.uniform(np.log10(0.03), 4.0, count) * rng.choice([-1.0, 1.0], count)
    # |eps| log-uniform from just inside the bound to 4: shift_or_eval's own three ranges
    eps = 10.0 ** rng.uniform(np.log10(T * 0.9), np.log10(4.0), count) * rng.choice([-1.0, 1.0], count)
    near0 = _rows(10.0 ** rng.uniform(-30.0, -3.0, 256) * rng.choice([-1.0, 1.0], 256),
                  rng.uniform(-2.0 * T, 2.0 * T, 256))
    spc, built = special_operands(0)
    assert np.array_equal(spc[:len(built), 3] - spc[:len(built), 0], built)
    ops = np.concatenate([_rows(a, a + eps), near0, spc])
    out = _shift_chain(bhrt_lib, ops, 0)
    fast = out[:, 4] == 1.0
    assert fast.sum() > 100 and (~fast).sum() > 1000
    bad = ~np.isfinite(ops[:, 3])
    assert bad.sum() == 4 and not fast[bad].any() and np.isnan(out[bad][:, :4]).all()
    err_narrow, err_wide = _check_site(ops, out, 0, "straddling 1/64")
    print(f"straddling operands: {int(fast.sum())} narrow, {int((~fast).sum())} redone with "
          f"shift_or_eval's bits; worst abs error narrow {err_narrow:.4e}, shift_or_eval on the "
          f"same operands {err_wide:.4e}")


# ---- frames ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_frames(oracle):
    cache = {}

    def get(cname, camname):
        if (cname, camname) not in cache:
            c = configs.CONFIGS[cname]
            bh, dk, cfg = c.scene()
            cache[cname, camname] = oracle.render_frame(bh, dk, cfg, _camera(camname), W, H,
                                                        c.method, c.flags)
        return cache[cname, camname]
    return get


def test_two_cameras_have_lanes_beyond_the_bound(oracle):
    """CPU: the replay (tools/shift_deltas.py) of the "polar" and "rims" 64 x 36 C2 frames has
    lanes beyond 1/64 at a far-anchor site, so the redo runs inside those frames; "horizon" has
    none, so that frame runs the narrow form alone."""
    import os
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shift_deltas
    for camname in ("polar", "rims", "horizon"):
        ages = shift_deltas.replay(_camera(camname), W, H, oracle)["ages"]
        over = sum(int(ages[s].sum()) for s in shift_deltas.AGE_SITES)
        print(camname, "lane-site cases beyond 1/64:", over)
        assert (over > 0) == (camname != "horizon")


@pytest.mark.gpu
@pytest.mark.parametrize("cname,camname", FRAMES)
def test_small_frames_vs_oracle_every_ray(bhrt_lib, oracle_frames, cname, camname):
    """Class and steps equal the oracle's on every ray of the frame, none left out; the float
    fields within the parity tests' tolerance."""
    c = configs.CONFIGS[cname]
    bh, dk, cfg = c.scene()
    want = oracle_frames(cname, camname)
    got = bhrt_lib.render_frame(bh, dk, cfg, _camera(camname), W, H, c.method, c.flags)
    for f in ("result", "steps"):
        print(cname, camname, f, "mismatches over all", W * H, "rays:",
              int((got[f] != want[f]).sum()))
    worst = compare(got, want, RTOL, sky_pinned(c.method), f"{cname} camera {camname}")
    print(cname, camname, "max rel err", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("camname", ["rims", "polar"])
def test_camera_path_and_ray_array_agree(bhrt_lib, camname):
    """The C2 scene's frame through the camera kernel and through bhrt_trace_rays_device on the
    same rays with the frame's own directions: one origin, so both set a ray up from the shared
    origin block; classes and steps equal, floats within 1e-9 (the two set-ups round a direction
    differently: test_gpu_stage_pairs' bound for the same comparison) -- and the ray array traced
    twice, in two launches of different size, gives the same bits for the rays both hold: a ray's
    rounding does not depend on its wave-mates."""
    c = configs.CONFIGS["C2"]
    bh, dk, cfg = c.scene()
    cam = _camera(camname)
    frame = bhrt_lib.render_frame(bh, dk, cfg, cam, W, H, c.method, c.flags)
    rays = configs.camera_rays(cam, W, H)
    arr = bhrt_lib.trace_rays(rays, bh, dk, cfg, c.method, c.flags)
    for f in ("result", "steps"):
        assert np.array_equal(frame[f], arr[f]), f
    worst = compare(frame, arr, 1e-9, sky_pinned(c.method), f"camera vs rays, {camname}")
    part = bhrt_lib.trace_rays(rays[37:37 + 1000], bh, dk, cfg, c.method, c.flags)
    for f, v in part.items():
        assert _same_bits(np.asarray(v, dtype=np.float64), np.asarray(arr[f][37:1037], dtype=np.float64)), f
    print(camname, "camera path vs ray array: max rel err", worst)
