"""The RK4 a = 0 iteration on two reciprocals (stage pairs (1,2) and (3,4), bhrt_trace_core.h rk4_step)
and its two chained angle shifts (shift_chain): stage 3's theta from stage 2's, and the advance
of state[1] from stage 4's.

  * the chained shifts on crafted operands (bhrt_check_shift_chain) against long-double sin/cos
    and against shift_or_eval on the same operands;
  * 64 x 36 frames of the C2 and C1 scenes from the three cameras of test_gpu_stage_pairs and
    two more, chosen with the replay of tools/shift_deltas.py, whose frames hold the largest
    chained shifts -- some beyond the chained bounds, so the redo of a shift runs inside a frame.

The bound of the operand test: a chained shift differs from shift_or_eval's on the same operands
by the truncation of its shorter polynomials alone -- the argument, the two closing FMAs and
their roundings are the same. On the chained intervals that is at most 1.2e-18 (two coefficients,
|eps| <= 1/64) and 9.8e-19 (one coefficient, |eps| <= 2^-10) by tools/shift_poly_fit.py, and the
Taylor remainders eps^7 / 5040 and eps^5 / 120 + ... bound it by 2^-54. The test holds the chained
form's worst absolute error to shift_or_eval's worst on the same operands plus CHAIN_SLACK =
2^-54; the fit's smaller figure is not used as the bound because the two forms' closing FMAs
round different sums (cm1 and sd differ in their last bits), which moves either worst case by a
fraction of an ulp of 1, 2^-53, in either direction.
Measured figures are in profiles/shiftchain/test_figures.txt.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, compare, sky_pinned
from bhrt import abi, configs
from test_gpu_parity import RTOL, _ulp_stable
from test_gpu_stage_pairs import CAMS as PAIR_CAMS

CHAIN_SLACK = 2.0 ** -54
BOUNDS = {0: 1.0 / 64.0, 1: 2.0 ** -10}  # site -> |x - a| the short polynomials are kept on
W, H = 64, 36
# The three cameras of test_gpu_stage_pairs (rims, far field crossing 15 rs, horizon) and two
# chosen with the replay (tools/shift_deltas.py, profiles/shiftchain/shift_deltas.txt):
#   "polar"  inside 15 rs, looking down the polar axis from just off it: where sin theta is
#            small the |d| <= 10 clamp of the accelerations binds, and the chained shifts are the
#            largest of any camera replayed -- stage 3 from stage 2 reaches h^2 / 4 * 10 = 0.025,
#            beyond 1/64 on 0.5 % of lanes, the advance 0.0075, beyond 2^-10 on 0.3 %: both
#            redos run inside the near-field kernel's frame;
#   "chain"  just beyond 15 rs with a wide field of view: the largest chained advance of the
#            off-axis cameras (0.003), in the far-field kernel, whose stages on the far-field
#            branch leave the anchors where they were.
CAMS = dict(PAIR_CAMS, polar=((1.4508, -2.3212, 28.8705), 50.0),
            chain=((5.1042, -33.0313, 7.7051), 100.0))
FRAMES = [(c, cam) for c in ("C2", "C1") for cam in CAMS]
LEFT_OUT_MAX = 0.01


def _camera(name):
    p, fov = CAMS[name]
    return abi.Camera(abi.v3(*p), abi.v3(*[-x for x in p]), abi.v3(0.0, 0.0, 1.0), fov)


# ---- the chained shifts on given operands ------------------------------------------------

def _shift_chain(bhrt_lib, ops, site):
    import torch
    L = bhrt_lib.load()
    L.bhrt_check_shift_chain.restype = C.c_int
    L.bhrt_check_shift_chain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    d_in = torch.from_numpy(np.ascontiguousarray(ops, dtype=np.float64).ravel()).cuda()
    out = torch.full((len(ops), 5), -7.0, dtype=torch.float64, device="cuda")
    assert L.bhrt_check_shift_chain(d_in.data_ptr(), len(ops), int(site), out.data_ptr(),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _rows(a, x):
    """Operand rows (a, s0, c0, x): s0, c0 the long-double sin a, cos a rounded to double."""
    a = np.asarray(a, dtype=np.float64)
    al = a.astype(np.longdouble)
    return np.stack([a, np.sin(al).astype(np.float64), np.cos(al).astype(np.float64),
                     np.asarray(x, dtype=np.float64)], axis=1)


def random_operands(site, seed=23, count=4096):
    """a log-uniform in [0.03, 1e4] with either sign; x = a + eps, eps over the full fast range
    of the site: half the cases uniform in [-T, T], half log-uniform down to 1e-12 T."""
    rng = np.random.default_rng(seed + site)
    T = BOUNDS[site]
    a = 10.0 ** rng.uniform(np.log10(0.03), 4.0, count) * rng.choice([-1.0, 1.0], count)
    eps = rng.uniform(-T, T, count)
    eps[1::2] = T * 10.0 ** rng.uniform(-12.0, 0.0, count // 2) * rng.choice([-1.0, 1.0],
                                                                             count // 2)
    return _rows(a, a + eps)


def special_operands(site):
    """eps exactly at the bound and one ulp either side of it (from a = -T/2, where x and
    x - a are exact), eps = +-0 and subnormal, a near 0 where x - a is inexact, and NaN, +-Inf
    in x. Returns the rows and, for the first six, the eps they were built for."""
    T = BOUNDS[site]
    a, x, eps = [], [], []
    for e in (T, np.nextafter(T, 0.0), np.nextafter(T, 1.0)):
        for sgn in (1.0, -1.0):
            a.append(-0.5 * T * sgn)
            x.append(-0.5 * T * sgn + sgn * e)
            eps.append(sgn * e)
    a += [1.0, -3.5, 0.0, 0.0, 0.0, 0.0, 0.0, 1e-20, -3e-17, 2.0 ** -1060, 1.0, 1.0, 1.0, 250.0]
    x += [1.0, -3.5, 0.0, -0.0, 5e-324, -1e-310, 2.0 ** -1022, 0.5 * T, 0.25 * T, 0.75 * T,
          np.nan, np.inf, -np.inf, np.nan]
    return _rows(a, x), np.array(eps)


def _same_bits(p, q):
    """Equal bit for bit; a NaN equals any NaN (payloads are not compared)."""
    p, q = np.asarray(p), np.asarray(q)
    nan = np.isnan(p) & np.isnan(q)
    return bool((nan | (p.view(np.uint64) == q.view(np.uint64))).all())


def _check_site(ops, out, site, what):
    """fast is |x - a| <= T as the double subtraction gives it (NaN: not fast); beyond the bound
    the chained pair equals shift_or_eval's bit for bit; within it both are compared with the
    long-double sin x, cos x. Returns (worst chained error, worst shift_or_eval error)."""
    T = BOUNDS[site]
    with np.errstate(invalid="ignore"):
        want_fast = np.abs(ops[:, 3] - ops[:, 0]) <= T
    fast = out[:, 4] == 1.0
    assert np.array_equal(fast, want_fast), (what, np.nonzero(fast != want_fast)[0][:10])
    assert _same_bits(out[~fast, 0], out[~fast, 2]) and _same_bits(out[~fast, 1], out[~fast, 3]), what
    xl = ops[fast, 3].astype(np.longdouble)
    truth = (np.sin(xl), np.cos(xl))
    err_chain = max(float(np.abs(out[fast, k].astype(np.longdouble) - truth[k]).max())
                    for k in (0, 1))
    err_today = max(float(np.abs(out[fast, 2 + k].astype(np.longdouble) - truth[k]).max())
                    for k in (0, 1))
    return err_chain, err_today


@pytest.mark.gpu
@pytest.mark.parametrize("site", [0, 1])
def test_chained_shift_on_operands(bhrt_lib, site):
    """4096 random operands over the site's fast range and the special ones: the fast-path flag
    is the stated comparison, a lane beyond the bound (or with NaN / Inf in x) gets
    shift_or_eval's bits, and the chained form's worst absolute error against long-double
    sin / cos is within CHAIN_SLACK of shift_or_eval's worst on the same operands."""
    rnd = random_operands(site)
    spc, eps = special_operands(site)
    # the crafted cases are what they say: x - a is the eps they were built for, exactly
    assert np.array_equal(spc[:len(eps), 3] - spc[:len(eps), 0], eps)
    ops = np.concatenate([rnd, spc])
    out = _shift_chain(bhrt_lib, ops, site)
    n = len(rnd)
    assert (out[:n, 4] == 1.0).all()  # every random operand is on the fast path
    sp_fast = out[n:, 4] == 1.0
    assert sp_fast.any() and (~sp_fast).any()
    # NaN and Inf in x give what shift_or_eval gives: NaN sin and cos
    bad = ~np.isfinite(spc[:, 3])
    assert bad.sum() == 4 and not sp_fast[bad].any()
    assert np.isnan(out[n:][bad][:, :4]).all()
    err_chain, err_today = _check_site(ops, out, site, f"site {site}")
    print(f"chained shift site {site} (|eps| <= {BOUNDS[site]:g}), {len(ops)} operands: worst "
          f"abs error chained {err_chain:.4e}, shift_or_eval {err_today:.4e}, difference "
          f"{err_chain - err_today:+.3e} (allowed {CHAIN_SLACK:.3e})")
    assert err_chain <= err_today + CHAIN_SLACK, (site, err_chain, err_today)


@pytest.mark.gpu
def test_other_site_is_refused(bhrt_lib):
    """bhrt_check_shift_chain knows sites 0 and 1; any other is an error, nothing is launched."""
    ops = random_operands(0, count=8)
    import torch
    L = bhrt_lib.load()
    L.bhrt_check_shift_chain.restype = C.c_int
    L.bhrt_check_shift_chain.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    d_in = torch.from_numpy(ops.ravel()).cuda()
    out = torch.full((8, 5), -7.0, dtype=torch.float64, device="cuda")
    assert L.bhrt_check_shift_chain(d_in.data_ptr(), 8, 2, out.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()


# ---- small frames against the oracle -----------------------------------------------------

@pytest.fixture(scope="module")
def frames(oracle):
    """The oracle's frame of every (scene, camera) and the rays it keeps (_ulp_stable on the
    frame's rays as a ray array), computed once."""
    cache = {}

    def get(cname, camname):
        if (cname, camname) not in cache:
            c = configs.CONFIGS[cname]
            bh, dk, cfg = c.scene()
            cam = _camera(camname)
            want = oracle.render_frame(bh, dk, cfg, cam, W, H, c.method, c.flags)
            keep = _ulp_stable(oracle, configs.camera_rays(cam, W, H), bh, dk, cfg)
            cache[cname, camname] = (want, keep)
        return cache[cname, camname]
    return get


@pytest.mark.parametrize("cname,camname", FRAMES)
def test_frames_hold_what_they_are_for(frames, cname, camname):
    """CPU: the oracle alone leaves out at most 1 % of each frame (_ulp_stable)."""
    want, keep = frames(cname, camname)
    assert (~keep).mean() <= LEFT_OUT_MAX, (cname, camname, int((~keep).sum()))
    if cname == "C2" and camname in PAIR_CAMS:
        res = want["result"]
        assert (res == abi.RAY_DISK).sum() > 100 and (res != abi.RAY_DISK).sum() > 100


def test_replay_cameras_run_the_fallbacks(oracle):
    """CPU: the replay of the two added cameras' 64 x 36 C2 frames. "polar" has lanes beyond
    both chained bounds (stage 3 from stage 2 beyond 1/64, the advance of state[1] from stage 4
    beyond 2^-10) and the largest chained shifts replayed, above camera B's 0.0086 and 0.00078 of
    a 480 x 270 frame; "chain" has lanes whose advance is beyond 2^-10 and none beyond 1/64. So
    the redo of either chained shift (shift_or_eval from the same anchor) runs inside these
    frames, in the near-field and in the far-field kernel."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import shift_deltas
    j10, j64 = shift_deltas.TS.index(1 / 1024), shift_deltas.TS.index(1 / 64)
    seen = {}
    for camname in ("polar", "chain"):
        res = shift_deltas.replay(_camera(camname), W, H, oracle)
        adv, st3 = res["adv_y1_from4"], res["stage3_from2"]
        seen[camname] = (adv, st3)
        print(f"{camname} camera replay: {res['lane_evals']} lane-iterations; advance from stage 4 "
              f"max {adv['max']:.3e}, {int(adv['lane_over'][j10])} lanes beyond 2^-10; stage 3 from "
              f"stage 2 max {st3['max']:.3e}, {int(st3['lane_over'][j64])} lanes beyond 1/64")
    adv, st3 = seen["polar"]
    assert st3["lane_over"][j64] > 0 and adv["lane_over"][j10] > 0
    assert st3["max"] > 0.0087 and adv["max"] > 0.003
    assert st3["max"] <= 0.025 * (1 + 1e-9)  # h / 2 * h / 2 * 10: the clamp's bound at h = 0.1
    adv, st3 = seen["chain"]
    assert adv["lane_over"][j10] > 0 and adv["lane_over"][j64] == 0 and st3["lane_over"][j64] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("cname,camname", FRAMES)
def test_small_frames_vs_oracle(bhrt_lib, frames, cname, camname):
    """result and steps equal the oracle's for every kept ray, hit fields within the parity
    tests' tolerance; the rays left out are _ulp_stable's, at most 1 %."""
    c = configs.CONFIGS[cname]
    bh, dk, cfg = c.scene()
    want, keep = frames(cname, camname)
    assert (~keep).mean() <= LEFT_OUT_MAX
    got = bhrt_lib.render_frame(bh, dk, cfg, _camera(camname), W, H, c.method, c.flags)
    every = sum(int((got[f] != want[f]).sum()) for f in ("result", "steps"))
    print(cname, camname, "left out", int((~keep).sum()), "of", W * H,
          "; class/steps mismatches over ALL rays:", every)
    worst = compare({f: v[keep] for f, v in got.items()}, {f: v[keep] for f, v in want.items()},
                    RTOL, sky_pinned(c.method), f"{cname} camera {camname}")
    print(cname, camname, "max rel err", worst)
