"""The reciprocal that RK4's a = 0 stages 2 and 3 share (bhrt_trace_core.h pair_rcp, rk4_step) and
the exact trims beside it (the -2 folded into the reciprocal, the trip's exits as masks).

  * the shared reciprocal on crafted operands (bhrt_check_pair_rcp) against exact quotients;
  * 64 x 36 frames of the C2 and C1 scenes from cameras that put the horizon, the disk's rims
    and the far-field threshold in the picture, every ray against the oracle;
  * the same rays through bhrt_trace_rays_device, the single-ray call and k_paths (bit for
    bit), the camera-frame kernel against the ray array, and rays forced through the redo pass.

The bound: a member's yr = RN(st RN(x_b W)), W = RN(1 / RN(x_a x_b)), x_a = RN(rc st). x_b's own
rounding cancels (it is a factor of P and of x_b W alike), so yr carries five roundings against
1 / rc: x_a, P, W, x_b W and the last product. Each is at most 2^-53 relative; the reciprocal's
(v_rcp_f64 and one cubic step) is taken as at most one ulp, 2^-52. That is 6 * 2^-53 relative,
and 2^-53 |v| <= ulp(v): at most ULP_BOUND = 6 ulp of the exact quotient, for ys alike.
Measured figures are in profiles/stagepairs/test_figures.txt.
"""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from conftest import compare, sky_pinned
from bhrt import abi, configs
from test_gpu_parity import RTOL, _ulp_stable

ULP_BOUND = 6
RS = 2.0  # the C1 / C2 black hole's Schwarzschild radius (M = 1)
W, H = 64, 36
# Cameras looking at the origin, up +z, off every axis (on an axis a one-ulp move of the origin
# turns phi by a right angle and _ulp_stable leaves the whole frame out):
#   "rims"    just inside 15 rs: the near-field kernel; both disk rims cross the picture, and rays
#             that miss run to the step budget;
#   "far"     beyond 15 rs: the far-field kernel, whose rays cross the threshold in flight (a ray
#             takes both branches) and end on the distance limit;
#   "horizon" inside 1.05 rs: every ray is at the horizon after its first step, and with a disk
#             some of those first segments cross it (the disk exit goes first).
# In this integrator no ray that starts outside 1.05 rs reaches it within the step budget: the
# step size there is 1e-4.
CAMS = {"rims": ((3.1, -29.2, 5.3), 60.0), "far": ((5.1, -33.0, 7.7), 50.0),
        "horizon": ((0.2925, -2.0268, 0.4179), 90.0)}
FRAMES = [(c, cam) for c in ("C2", "C1") for cam in CAMS]
LEFT_OUT_MAX = 0.01


def _camera(name):
    p, fov = CAMS[name]
    return abi.Camera(abi.v3(*p), abi.v3(*[-x for x in p]), abi.v3(0.0, 0.0, 1.0), fov)


# ---- the shared reciprocal on given operands ---------------------------------------------

def _pair_rcp(bhrt_lib, ops, huge):
    import torch
    L = bhrt_lib.load()
    L.bhrt_check_pair_rcp.restype = C.c_int
    L.bhrt_check_pair_rcp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    d_in = torch.from_numpy(np.ascontiguousarray(ops, dtype=np.float64).ravel()).cuda()
    out = torch.full((len(ops), 5), -7.0, dtype=torch.float64, device="cuda")
    assert L.bhrt_check_pair_rcp(d_in.data_ptr(), len(ops), int(huge), out.data_ptr(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _ulps(got, operand):
    """|got - 1 / operand| in ulps of the exact quotient (of its rounded double)."""
    if not np.isfinite(operand) or operand == 0.0:  # 1 / Inf = 0 exactly; 1 / NaN, 1 / 0: no
        return 0.0 if np.isinf(operand) and got == 0.0 else np.inf  # finite value is right
    exact = 1 / Fraction(float(operand))
    return float(abs(Fraction(float(got)) - exact) / Fraction(float(np.spacing(abs(float(exact))))))


def random_pairs(seed=11, count=4096):
    """(rc_a, st_a, rc_b, st_b) log-uniform over the loop's range: rc in [1.5 rs, 1e6],
    |st| in [0.01, 1], either sign."""
    rng = np.random.default_rng(seed)
    ops = np.empty((count, 4))
    for k in (0, 2):
        ops[:, k] = 10.0 ** rng.uniform(np.log10(1.5 * RS), 6.0, count)
        ops[:, k + 1] = 10.0 ** rng.uniform(-2.0, 0.0, count) * rng.choice([-1.0, 1.0], count)
    return ops


def special_pairs():
    """One member out of range (the other a plain operand), both orders: sin theta = +-0,
    +-0.01 and one ulp either side of it, subnormals, NaN, +-Inf; and rc at 1e150 and one ulp
    either side of it (the redo pass's test), alone and in both members."""
    lim = 0.01
    sts = [0.0, -0.0, lim, -lim, np.nextafter(lim, 0.0), np.nextafter(lim, 1.0),
           -np.nextafter(lim, 0.0), -np.nextafter(lim, 1.0), 5e-324, -5e-324, 1e-310, 2.0 ** -1022,
           np.nan, np.inf, -np.inf]
    plain = [(3.0, 1.0), (7.25, -0.3), (1.0e6, 0.010000001), (40.0, 0.7071067811865476)]
    big = 1.0e150
    ops = []
    for st in sts:
        for rc_p, st_p in plain:
            ops.append((9.5, st, rc_p, st_p))
            ops.append((rc_p, st_p, 9.5, st))
    for rc in (np.nextafter(big, 0.0), big, np.nextafter(big, np.inf)):
        for rc_p, st_p in plain:
            ops.append((rc, -0.5, rc_p, st_p))
            ops.append((rc_p, st_p, rc, 1.0))
        ops.append((rc, 1.0, rc, -1.0))
    return np.array(ops)


def _expected_ok(ops, huge):
    ok = (np.abs(ops[:, 1]) >= 0.01) & (np.abs(ops[:, 3]) >= 0.01)
    if huge:
        ok &= (ops[:, 0] < 1.0e150) & (ops[:, 2] < 1.0e150)
    return ok


def _in_range(ops, huge):
    """Both members' operands are what a stage can hand the pair in range: 0.01 <= |sin theta|
    <= 1 and, in the redo pass's form, rc < 1e150."""
    st = np.abs(ops[:, [1, 3]])
    good = ((st >= 0.01) & (st <= 1.0)).all(axis=1)
    if huge:
        good &= (ops[:, 0] < 1.0e150) & (ops[:, 2] < 1.0e150)
    return good


def _check_pairs(ops, out, huge, what):
    """The range test is the one stated. A pair with both members in range passes it and all four
    quotients are within ULP_BOUND of the exact ones. Any other pair leaves each member a value
    that is within the bound or not finite (NaN here also stands for "not used": where the test
    fails both stages take the literal form) -- never a finite wrong value."""
    ok = out[:, 4] == 1.0
    assert np.array_equal(ok, _expected_ok(ops, huge)), (what, np.nonzero(ok != _expected_ok(ops, huge))[0])
    good = _in_range(ops, huge)
    assert ok[good].all(), what
    used = np.where(ok[:, None], out[:, :4], np.nan)
    worst = 0.0
    for i in range(len(ops)):
        for k in range(4):
            if not np.isfinite(used[i, k]):
                assert not good[i], (what, ops[i].tolist(), k)
                continue
            err = _ulps(used[i, k], ops[i, k])
            assert err <= ULP_BOUND, (what, ops[i].tolist(), k, float(used[i, k]), err)
            worst = max(worst, err)
    return worst


@pytest.mark.gpu
def test_shared_reciprocal_on_random_operands(bhrt_lib):
    """4096 log-uniform pairs over the loop's range: every pair passes the range test and
    1 / rc, 1 / sin theta of both members are within ULP_BOUND ulp of the exact quotients
    (measured worst: 2.9 ulp, in the hot form and in the redo pass's)."""
    ops = random_pairs()
    for huge in (0, 1):
        out = _pair_rcp(bhrt_lib, ops, huge)
        assert (out[:, 4] == 1.0).all()
        worst = _check_pairs(ops, out, huge, f"random huge={huge}")
        print(f"shared reciprocal, 4096 random pairs, huge={huge}: worst {worst:.3f} ulp")


@pytest.mark.gpu
def test_shared_reciprocal_on_special_operands(bhrt_lib):
    """A member whose sin theta is +-0, below 0.01, subnormal, NaN or Inf, or whose rc is at
    1e150 in the redo pass's form, fails the range test for BOTH members (neither stage uses a
    quotient of the pair); at and above the limits both members are within the bound."""
    ops = special_pairs()
    for huge in (0, 1):
        out = _pair_rcp(bhrt_lib, ops, huge)
        worst = _check_pairs(ops, out, huge, f"special huge={huge}")
        ok = out[:, 4] == 1.0
        assert ok.any() and (~ok).any()
        print(f"shared reciprocal, {len(ops)} special pairs, huge={huge}: {int(ok.sum())} in "
              f"range, worst {worst:.3f} ulp")
    # rc = 1e150 in both members passes without the redo pass's test: P = 1e300 is finite
    both = (ops[:, 0] >= 1.0e150) & (ops[:, 2] >= 1.0e150)
    assert both.any() and (_pair_rcp(bhrt_lib, ops[both], 0)[:, 4] == 1.0).all()


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
    """CPU: the oracle alone leaves out at most 1 % of each frame (_ulp_stable), and the
    cameras show what CAMS says."""
    want, keep = frames(cname, camname)
    assert (~keep).mean() <= LEFT_OUT_MAX, (cname, camname, int((~keep).sum()))
    res = want["result"]
    r0 = float(np.linalg.norm(CAMS[camname][0]))
    if cname == "C2":
        assert (res == abi.RAY_DISK).sum() > 100 and (res != abi.RAY_DISK).sum() > 100
    if camname == "horizon":
        assert r0 < 1.05 * RS and (res == abi.RAY_HORIZON).sum() > 100
    elif camname == "far":
        assert r0 > 15.0 * RS and (res == abi.RAY_MAX_DISTANCE).sum() > 100
        assert want["steps"].max() > 300  # (t passes 15 rs, the far-field test's operand)
    else:
        assert 14.0 * RS < r0 < 15.0 * RS and (res == abi.RAY_MAX_STEPS).sum() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("cname,camname", FRAMES)
def test_small_frames_vs_oracle(bhrt_lib, frames, cname, camname):
    """result and steps equal the oracle's for every kept ray, hit fields within the parity
    tests' tolerance; the rays left out are _ulp_stable's, at most 1 % (measured: none left out,
    no class or step differs on any ray of the six frames, largest relative error 4.1e-12)."""
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


# ---- the same bits on every path ---------------------------------------------------------

def _rays256():
    """256 camera-B rays of C2's frame: 8 rows of 32 across the crop of test_gpu_paths (rays
    that hit the disk after a step or two beside rays that run to the step budget)."""
    c = configs.CONFIGS["C2"]
    rays = configs.camera_rays(configs.camera("B"), c.width, c.height).reshape(c.height, c.width)
    return np.ascontiguousarray(rays[500:508, 1232:1264]).reshape(-1)


@pytest.mark.gpu
def test_same_bits_on_every_path(bhrt_lib, monkeypatch):
    """256 rays of the C2 scene: bhrt_trace_rays_device, the hit fields of k_paths and the
    single-ray call agree bit for bit (the single-ray kernel sets a ray up on the device, so the
    array is traced with the per-ray set-up too); the last point of k_paths is the hit position
    to the last bits (profiles/paths/hits_bits.txt: <= 1.8e-15 relative before this change)."""
    from test_gpu_paths import _trace_rays_device, run_device
    c = configs.CONFIGS["C2"]
    bh, dk, cfg = c.scene()
    rays = _rays256()
    trace = _trace_rays_device(bhrt_lib, rays, bh, dk, cfg, c.method)
    assert len(set(trace["result"].tolist())) >= 2
    P = cfg.max_integration_steps + 1
    paths = run_device(bhrt_lib, rays, bh, dk, cfg, c.method, P, 1)
    for f in abi.PATH_HIT_FIELDS:
        assert np.array_equal(paths[f], trace[f], equal_nan=f not in ("result", "steps")), f
    last = paths["xyz"][np.arange(len(rays)), paths["count"] - 1]
    hit = np.stack([trace["hit_x"], trace["hit_y"], trace["hit_z"]], axis=1)
    has = ~np.isnan(hit).any(axis=1)
    rel = np.abs(last[has] - hit[has]) / np.maximum(np.abs(hit[has]), 1e-300)
    print("k_paths last point vs hit position: max rel", float(rel.max()),
          "differing rays", int((rel > 0).any(axis=1).sum()))
    assert float(rel.max()) <= 1e-14

    monkeypatch.setenv("BHRT_SHARED_ORIGIN", "0")
    arr = bhrt_lib.trace_rays(rays, bh, dk, cfg, c.method, c.flags)
    L = bhrt_lib.load()
    for i in range(0, len(rays), 5):
        o, d = rays["origin"][i], rays["direction"][i]
        hitrec = abi.RayTraceHit()
        res = L.trace_ray(C.byref(abi.Ray(abi.v3(*o), abi.v3(*d))), C.byref(bh), C.byref(dk),
                          C.byref(cfg), C.byref(hitrec))
        assert (res, hitrec.steps) == (arr["result"][i], arr["steps"][i]), i
        one = np.array([hitrec.hit_position.x, hitrec.hit_position.y, hitrec.hit_position.z,
                        hitrec.distance])
        many = np.array([arr["hit_x"][i], arr["hit_y"][i], arr["hit_z"][i], arr["distance"][i]])
        assert np.array_equal(one, many, equal_nan=True), (i, one, many)


@pytest.mark.gpu
def test_frame_kernel_equals_ray_array(bhrt_lib):
    """The camera-frame kernel against bhrt_trace_rays on the same frame's rays: classes and
    steps equal, floats within 1e-9 (the two set-ups round a direction differently:
    test_shared_origin_ray_arrays_vs_oracle's bound), C2's scene from every camera of CAMS."""
    c = configs.CONFIGS["C2"]
    bh, dk, cfg = c.scene()
    for camname in CAMS:
        cam = _camera(camname)
        frame = bhrt_lib.render_frame(bh, dk, cfg, cam, 32, 8, c.method, c.flags)
        arr = bhrt_lib.trace_rays(configs.camera_rays(cam, 32, 8), bh, dk, cfg, c.method, c.flags)
        for f in ("result", "steps"):
            assert np.array_equal(frame[f], arr[f]), (camname, f)
        for f in ("hit_x", "hit_y", "hit_z", "distance"):
            a, b = frame[f], arr[f]
            assert np.array_equal(np.isnan(a), np.isnan(b)), (camname, f)
            ok = ~np.isnan(a)
            rel = np.abs(a[ok] - b[ok]) / np.maximum(np.abs(b[ok]), 1e-300)
            assert rel.size == 0 or float(rel.max()) <= 1e-9, (camname, f, float(rel.max()))


@pytest.mark.gpu
def test_rays_through_the_redo_pass(bhrt_lib, oracle):
    """The pair in the redo pass's instantiation (its rc < 1e150 test, the library sincos): a
    frame whose every ray is handed over (the unprovable far-field bound of
    test_unbounded_far_field_launch_takes_the_redo_path: M = 1e-3 seen from camera B), and rays
    evicted for a large sincos argument (test_large_argument_rays_take_the_redo_path's groups at
    |origin| 2e6 and just outside the horizon, its _ulp_stable rays), against the oracle."""
    cam = configs.camera("B")
    dk = abi.disk(0.006, 0.04, 1.0, 1.0)
    cfg = abi.sim_config(0.1, 100.0, 300, 1e-6)
    bh = abi.black_hole(1.0e-3, 0.0)
    bhrt_lib.stats(reset=True)
    got = bhrt_lib.render_frame(bh, dk, cfg, cam, 40, 24, abi.INTEGRATOR_RK4, 0)
    st = bhrt_lib.stats(reset=True)
    assert st["rays_redone"] == 40 * 24, st
    want = oracle.render_frame(bh, dk, cfg, cam, 40, 24, abi.INTEGRATOR_RK4, 0)
    compare(got, want, RTOL, False, "redo-pass frame")

    rng = np.random.default_rng(7)
    n = 192
    rays = np.zeros(n, dtype=abi.RAY_DTYPE)
    radius = np.concatenate([np.full(64, 2.0e6), 2.0 + 10.0 ** rng.uniform(-8.0, -7.0, 128)])
    u = rng.normal(size=(n, 3))
    rays["origin"] = u / np.linalg.norm(u, axis=1)[:, None] * radius[:, None]
    d = rng.normal(size=(n, 3))
    rays["direction"] = d / np.linalg.norm(d, axis=1)[:, None]
    bh = abi.black_hole(1.0, 0.0)
    cfg = abi.sim_config(time_step=0.1, max_dist=1.0e8, max_steps=120)
    dk = abi.disk(6.0, 20.0, 1.0, 1.0)
    sel = rays[_ulp_stable(oracle, rays, bh, dk, cfg)]
    assert len(sel) >= 32
    bhrt_lib.stats(reset=True)
    got = bhrt_lib.trace_rays(sel, bh, dk, cfg)
    st = bhrt_lib.stats(reset=True)
    compare(got, oracle.trace_rays(sel, bh, dk, cfg), RTOL, False, "large-argument rays")
    assert st["rays_redone"] > 0, st
