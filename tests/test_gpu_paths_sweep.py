"""The path kernels (paths.hip k_paths / k_path) on the scene sweep (tests/sweep_scenes.py):
the 181 edge rays of rays_rk4_disk.npz in one bhrt_trace_paths_device call per scene -- two full
waves and a ragged one of 53 lanes, path lengths from 2 points to the step budget inside every
wave -- with the scene's disk and with disk = NULL, against the oracle's paths
(test_paths_cpu.oracle_paths) under test_gpu_paths.check_paths' rules, and the drop-in
integrate_photon_path on six rays of every scene.

Tolerances are the project's contract: counts, classes and steps exact, every stored component
and hit float rtol 1e-5 with atol 1e-9, NaN and +-inf at the same places. Rays of index >= 21
match without exception; a hand-written ray may differ only where the oracle's margin for that
disk argument is below KNIFE_EDGE (test_paths_sweep_cpu.test_path_sweep_inputs_are_decisive caps
how many there are). PATHS_SWEEP_ERR / SWEEP_KNIFE lines are information, never a bound
(profiles/paths_sweep/test_figures.txt).
"""
import time

import numpy as np
import pytest

import paths_sweep_rule as rule
import sweep_scenes as sw
from conftest import KNIFE_EDGE
from bhrt import abi
from test_gpu_paths import (ATOL, BIG, RTOL, SENT, SENT32, SENTI, _trace_rays_device, check_hits,
                            check_paths, run_device)
from test_paths_cpu import TRACE_FIELDS, oracle_paths, stored_points
from test_scene_sweep import HAND_RAYS

pytestmark = pytest.mark.gpu

CASES = [(name, arg) for name in sw.SCENES for arg in ("disk", "null")
         if arg == "null" or sw.SCENES[name][7] is not None]
IDS = [f"{n}-{a}" for n, a in CASES]
STORE_SCENES = ("m24_rkf", "m05_kerr_rkf", "retro_rk4", "dt7_kerr_rkf", "dtneg_rk4", "dt0_rk4",
                "tol_lo_s", "tol_0_kerr", "disk_thin_ring", "leapfrog", "m40")
STORE_CASES = [c for c in CASES if c[0] in STORE_SCENES]
DROPIN_RAYS = (21, 50, 90, 130, 170, 180)
HIT_FLOATS = ("hit_x", "hit_y", "hit_z", "distance", "time_dilation")

_cache = {}


def _scene(name, arg):
    bh, dk, cfg, method, _, _ = sw.scene(name)
    return bh, (dk if arg == "disk" else None), cfg, method


def _oracle(oracle, name, arg):
    """The oracle's paths, trace and margins of the edge rays for one scene and disk argument;
    computed once, never modified."""
    if (name, arg) not in _cache:
        bh, dk, cfg, method = _scene(name, arg)
        rays = rule.edge_rays()
        trace, margin = oracle.trace_rays_margin(rays, bh, dk, cfg, method, 0, fields=TRACE_FIELDS)
        _cache[name, arg] = (oracle_paths(oracle, rays, bh, dk, cfg, method), trace, margin)
    return _cache[name, arg]


def _pairs(cfg):
    longer = cfg.max_integration_steps + 5
    return ((1, longer), (3, longer), (8, 7), (1, 2), (BIG, longer))


def _one(got, i):
    return {f: v[i:i + 1] for f, v in got.items()}


def _path_fault(got, i, q, every, P, what):
    """check_paths' rules on ray i, with the NaN, +inf and -inf patterns compared explicitly:
    None, or what is wrong."""
    want = stored_points(q, every, P)
    try:
        a = got["xyz"][i, :len(want)]
        for pattern in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(pattern(a), pattern(want)), (what, i, pattern.__name__)
        check_paths(_one(got, i), [q], every, P, what=f"{what} [ray {i}], its slice")
    except AssertionError as e:
        return str(e)
    return None


def _hit_fault(got, trace, i, what):
    try:
        for f in HIT_FLOATS:
            for pattern in (np.isnan, np.isposinf, np.isneginf):
                assert pattern(got[f][i]) == pattern(trace[f][i]), (what, i, f, pattern.__name__)
        check_hits(_one(got, i), _one(trace, i), what=f"{what} ray {i}")
    except AssertionError as e:
        return str(e)
    return None


def _errors(got, paths, skip):
    """The measured error of an untruncated every = 1 run over the rays not in `skip`: the worst
    relative error of a component of magnitude >= 1e-4, the worst absolute difference of a
    smaller one, and the worst |got - want|_inf / |want|_2 of a point."""
    rel = small = norm = 0.0
    for i, q in enumerate(paths):
        if i in skip:
            continue
        a, b = got["xyz"][i, :len(q)], q
        ok = np.isfinite(a) & np.isfinite(b)
        diff, scale = np.abs(a - b), np.maximum(np.abs(a), np.abs(b))
        big = ok & (scale >= 1e-4)
        if big.any():
            rel = max(rel, float((diff[big] / scale[big]).max()))
        if (ok & ~big).any():
            small = max(small, float(diff[ok & ~big].max()))
        rows = ok.all(axis=1) & (np.linalg.norm(np.where(ok, b, 0.0), axis=1) > 0.0)
        if rows.any():
            norm = max(norm, float((diff[rows].max(axis=1) / np.linalg.norm(b[rows], axis=1)).max()))
    return rel, small, norm


@pytest.mark.parametrize("name,arg", CASES, ids=IDS)
def test_sweep_paths_vs_oracle(bhrt_lib, oracle, name, arg):
    """bhrt_trace_paths_device into sentinel-filled arrays at five (every, max_positions) pairs,
    and the hits of the same calls: bhrt_trace_rays_device's bits, the oracle's trace within the
    contract."""
    t0 = time.perf_counter()
    bh, dk, cfg, method = _scene(name, arg)
    rays = rule.edge_rays()
    paths, trace, margin = _oracle(oracle, name, arg)
    t_oracle = time.perf_counter() - t0
    knife = [i for i in range(HAND_RAYS) if margin[i] < KNIFE_EDGE]
    own = _trace_rays_device(bhrt_lib, rays, bh, dk, cfg, method)
    differ, faults = set(), []
    for k, (every, P) in enumerate(_pairs(cfg)):
        what = f"{name} {arg} every {every} P {P}"
        got = run_device(bhrt_lib, rays, bh, dk, cfg, method, P, every)
        for i in range(len(rays)):
            bad = _path_fault(got, i, paths[i], every, P, what)
            if not bad and k == 0:  # (the later calls' hits are these bits: `own`, below)
                bad = _hit_fault(got, trace, i, what)
            if bad:
                differ.add(i)
                if i >= HAND_RAYS or i not in knife:
                    faults.append(bad)
        for f in abi.PATH_HIT_FIELDS:  # the trace kernel's own bits (flags 0)
            assert np.array_equal(got[f], own[f], equal_nan=f not in ("result", "steps")), (what, f)
        if k == 0:
            rel, small, norm = _errors(got, paths, differ)
    wall = time.perf_counter() - t0
    print(f"PATHS_SWEEP_ERR {name} {arg} rel {rel:.3e} abs_below_1e-4 {small:.3e} "
          f"norm_rel {norm:.3e} min_margin {float(np.nanmin(margin)):.3e} "
          f"wall_s {wall:.2f} (oracle {t_oracle:.2f})")
    print(f"SWEEP_KNIFE paths {name} {arg} knife-edge {knife} differ {sorted(differ)}")
    assert not faults, (len(faults), faults[:3])


@pytest.mark.parametrize("name,arg", CASES, ids=IDS)
def test_sweep_paths_counters(bhrt_lib, name, arg):
    """Without hits the call is one launch of n rays; an RK4 ray adds its R.k at termination,
    which is count - 1 where nothing is decimated or truncated. bhrt_get_stats returns 0
    (bhrt.lib.stats raises otherwise)."""
    bh, dk, cfg, method = _scene(name, arg)
    rays = rule.edge_rays()
    bhrt_lib.stats(reset=True)
    got = run_device(bhrt_lib, rays, bh, dk, cfg, method, cfg.max_integration_steps + 5, 1,
                     hits=False)
    st = bhrt_lib.stats(reset=True)
    assert st["rays"] == len(rays) and st["launches"] == 1, st
    if method == abi.INTEGRATOR_RK4:
        assert st["iterations"] == int((got["count"].astype(np.int64) - 1).sum()), st
    for f in abi.PATH_HIT_FIELDS:
        assert (got[f] == SENTI).all(), (f, "written though hits was NULL")


@pytest.mark.parametrize("name,arg", STORE_CASES, ids=[f"{n}-{a}" for n, a in STORE_CASES])
def test_sweep_store_forms_agree(bhrt_lib, monkeypatch, name, arg):
    """BHRT_PATHS_STORE=direct and =staged write the same bytes into every output."""
    bh, dk, cfg, method = _scene(name, arg)
    rays = rule.edge_rays()
    for every, P in ((1, cfg.max_integration_steps + 5), (8, 7), (3, 9)):
        out = {}
        for form in ("direct", "staged"):
            monkeypatch.setenv("BHRT_PATHS_STORE", form)
            out[form] = run_device(bhrt_lib, rays, bh, dk, cfg, method, P, every)
        for f in out["direct"]:
            assert out["direct"][f].tobytes() == out["staged"][f].tobytes(), (name, arg, every, P, f)


@pytest.mark.parametrize("name", list(sw.SCENES))
def test_sweep_single_ray_call(bhrt_lib, oracle, name):
    """integrate_photon_path through libbhrt on six rays: the points and count of the ray's row
    of the disk = NULL batched call bit for bit; return value, hit class and hit steps the
    oracle's; hit floats within the contract; and the reference's truncation at
    max_positions = 3 (count stops at 3, nothing written beyond, result and hit as before)."""
    bh, _, cfg, method = _scene(name, "null")
    rays = rule.edge_rays()
    P = cfg.max_integration_steps + 1
    fn, orc_fn = bhrt_lib.load().integrate_photon_path, oracle.lib.orc_integrate_photon_path
    batch = run_device(bhrt_lib, rays, bh, None, cfg, method, P, 1, hits=False)
    for i in DROPIN_RAYS:
        buf, m, res, hit = rule.integrate(fn, rays[i], bh, cfg, method, P, fill=SENT, room=2)
        wbuf, wm, wres, whit = rule.integrate(orc_fn, rays[i], bh, cfg, method, P)
        assert m == batch["count"][i], (name, i, m, batch["count"][i])
        assert buf[:m].tobytes() == batch["xyz"][i, :m].tobytes(), (name, i)
        assert (buf[m:] == SENT).all(), (name, i)
        assert (res, m, hit.result, hit.steps) == (wres, wm, whit.result, whit.steps), (name, i)
        h = lambda x: np.array([x.hit_position.x, x.hit_position.y, x.hit_position.z, x.distance,
                                x.time_dilation])
        for pattern in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(pattern(h(hit)), pattern(h(whit))), (name, i, pattern.__name__)
        np.testing.assert_allclose(h(hit), h(whit), rtol=RTOL, atol=ATOL, err_msg=f"{name} ray {i}")
        cut, cm, cres, chit = rule.integrate(fn, rays[i], bh, cfg, method, 3, fill=SENT, room=2)
        _, om, ores, ohit = rule.integrate(orc_fn, rays[i], bh, cfg, method, 3)
        assert cm == om == min(m, 3), (name, i, cm, om, m)
        assert cut[:cm].tobytes() == buf[:cm].tobytes() and (cut[cm:] == SENT).all(), (name, i)
        assert (cres, chit.result, chit.steps) == (ores, ohit.result, ohit.steps) \
            == (res, hit.result, hit.steps), (name, i)
        assert h(chit).tobytes() == h(hit).tobytes(), (name, i)


def _same(a, b, what):
    """The contract on arrays that hold NaN and infinities: the same places, then 1e-5 / 1e-9."""
    assert a.shape == b.shape, (what, a.shape, b.shape)
    for pattern in (np.isnan, np.isposinf, np.isneginf):
        assert np.array_equal(pattern(a), pattern(b)), (what, pattern.__name__)
    ok = np.isfinite(b)
    np.testing.assert_allclose(a[ok], b[ok], rtol=RTOL, atol=ATOL, err_msg=what)


@pytest.mark.parametrize("name", list(rule.REPAIRED_SCENES))
def test_duplicate_segment_hit_behind_the_stuck_point(bhrt_lib, oracle, monkeypatch, name):
    """k_paths' R.k - k_before == 2: a stuck ray whose segment 1 cannot hit and whose duplicate
    segment 2 does (paths_sweep_rule.REPAIRED_SCENES: non-finite origins, repaired by the first
    iteration; test_paths_sweep_cpu.test_repaired_origin_rays pins the oracle to the compiled
    reference and shows that none of these rays is knife-edge). The stored path is the
    non-finite origin, the stuck point and the hit point; in both store forms, decimated and
    truncated; with the hits of the same call."""
    bh, dk, cfg, method = rule.repaired_scene(name)
    rays = rule.repaired_rays()
    want = oracle_paths(oracle, rays, bh, dk, cfg, method)
    trace = oracle.trace_rays(rays, bh, dk, cfg, method, 0, fields=TRACE_FIELDS)
    behind = (trace["result"] == abi.RAY_DISK) & (trace["steps"] == 2)
    assert behind.sum() >= 10 and all(len(want[i]) == 3 for i in np.nonzero(behind)[0])
    # The hits are the trace kernel's (paths.c). Where the origin's round trip is infinite in
    # every component the first segment is infinitely long and the reference ends the ray there
    # as MAX_DISTANCE; k_path and k_paths do (seg_len<WIDE>), the trace kernel's hot RKF45
    # instantiations do not (their one-correction root gives NaN for +Inf, so the ray runs on to
    # DISK or MAX_STEPS): a known deviation of bhrt_trace_rays on infinite origins, outside the
    # path kernels. Those 12 rays' hits are judged against the oracle with LEAPFROG only.
    endless = np.array([np.isinf(q[0]).all() for q in want])
    assert endless.sum() == 12 and not (endless & behind).any()
    judged = np.ones(len(rays), dtype=bool) if method == sw.LEAPFROG else ~endless
    own = _trace_rays_device(bhrt_lib, rays, bh, dk, cfg, method)
    longer = cfg.max_integration_steps + 5
    for every, P in ((1, longer), (2, longer), (3, longer), (1, 2), (8, 7), (BIG, longer)):
        out = {}
        for form in ("direct", "staged"):
            monkeypatch.setenv("BHRT_PATHS_STORE", form)
            out[form] = got = run_device(bhrt_lib, rays, bh, dk, cfg, method, P, every)
            what = f"{name} {form} every {every} P {P}"
            for i in range(len(rays)):
                q = stored_points(want[i], every, P)
                assert got["count"][i] == len(q), (what, i, int(got["count"][i]), len(q))
                _same(got["xyz"][i, :len(q)], q, f"{what} ray {i}")
                assert np.array_equal(got["xyz32"][i, :len(q)], np.float32(got["xyz"][i, :len(q)]),
                                      equal_nan=True), (what, i)
                assert (got["xyz"][i, len(q):] == SENT).all(), (what, i, "xyz tail written")
                assert (got["xyz32"][i, len(q):] == SENT32).all(), (what, i)
            for f in ("result", "steps"):
                assert np.array_equal(got[f][judged], trace[f][judged]), (what, f)
            for f in HIT_FLOATS:
                _same(got[f][judged], trace[f][judged], f"{what} {f}")
            for f in abi.PATH_HIT_FIELDS:  # what the API promises of the hits, for every ray
                assert np.array_equal(got[f], own[f], equal_nan=f not in ("result", "steps")), (what, f)
        for f in out["direct"]:
            assert out["direct"][f].tobytes() == out["staged"][f].tobytes(), (name, every, P, f)
    # k_path on an origin of each kind: the row of the disk = NULL batched call, the oracle's
    # class, count and steps (ray 30's first segment is infinitely long: MAX_DISTANCE at once)
    monkeypatch.delenv("BHRT_PATHS_STORE")
    cap = cfg.max_integration_steps + 1
    null = run_device(bhrt_lib, rays, bh, None, cfg, method, cap, 1, hits=False)
    fn, orc_fn = bhrt_lib.load().integrate_photon_path, oracle.lib.orc_integrate_photon_path
    for i in (0, 12, 24, 30, 36, 42):
        buf, m, res, hit = rule.integrate(fn, rays[i], bh, cfg, method, cap)
        _, wm, wres, whit = rule.integrate(orc_fn, rays[i], bh, cfg, method, cap)
        assert (res, m, hit.result, hit.steps) == (wres, wm, whit.result, whit.steps), (name, i)
        assert m == null["count"][i], (name, i)
        assert np.array_equal(buf[:m], null["xyz"][i, :m], equal_nan=True), (name, i)
