"""Adaptive physical geodesics (bhrt_kerr_rk45_*) without a GPU: the symbols, the header's rule,
the numpy rule (kerr_rk45_rule.py) against the fixed-step rule's classes, against itself at a
tolerance of 1e-13, against the analytic critical impact parameters and its own condition, and
the host code on simulated devices under ASan+UBSan (a stand-alone program; nothing is loaded
into Python under a sanitizer). The rule is stated in include/bhrt_api.h."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from bhrt import abi, lib
from host_sources import hip_sources, host_core, host_feature
import kerr_rule as kr
import kerr_rk45_rule as k5

CSRC = os.path.join(ROOT, "raytracing-engine-in-c_amd", "csrc")
FAKE = os.path.join(ROOT, "tests", "fakehip")
ENTRIES = ("bhrt_kerr_rk45_frame_device", "bhrt_kerr_rk45_frame", "bhrt_kerr_rk45_rays_device",
           "bhrt_kerr_rk45_rays")
WRAPPERS = ("kerr_rk45_frame_device", "kerr_rk45_frame", "kerr_rk45_rays_device", "kerr_rk45_rays")
FRAMES = [(spin, disk, W, H) for spin, disk in kr.SCENES for W, H in kr.FRAME_SIZES]
FRAME_IDS = [f"spin{spin}-{W}x{H}" for spin, _, W, H in FRAMES]
DELTA = 1e-3
# the largest component difference of the disk points against the rule at tolerance 1e-13:
# measured 4.4e-6 .. 5.8e-6 at 1e-8 and 2.6e-4 .. 6.4e-4 at 1e-6; the bounds are 3x the worst
DISK_POINT_BOUND = {1e-8: 2e-5, 1e-6: 2e-3}


def test_symbols_prototypes_and_the_diag_struct():
    L = lib.load()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in lib._PROTOS, name
    for name in WRAPPERS:
        assert callable(getattr(lib, name)), name
    assert C.sizeof(abi.KerrRk45Diag) == 24
    assert (abi.KerrRk45Diag.h_residual.offset, abi.KerrRk45Diag.lz_drift.offset,
            abi.KerrRk45Diag.rejected.offset) == (0, 8, 16)
    assert C.sizeof(abi.KerrDiag) == 16     # (the fixed-step calls keep theirs)
    # argument for argument the fixed-step calls' prototypes, with the wider diag struct
    for name in ENTRIES:
        res, args = lib._PROTOS[name]
        res4, args4 = lib._PROTOS[name.replace("_rk45", "")]
        assert res is res4 and len(args) == len(args4), name
        for a, b in zip(args, args4):
            assert a is b or (a._type_, b._type_) == (abi.KerrRk45Diag, abi.KerrDiag), name
    header = open(os.path.join(ROOT, "include", "bhrt_api.h")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
    assert re.search(r"double\* h_residual;\s*double\* lz_drift;\s*int\* rejected;\s*"
                     r"\} bhrt_kerr_rk45_diag;", header)
    # its section follows "Physical geodesics" and precedes the recorded paths
    at = [header.index(s) for s in ("/* ---- Physical geodesics:", "bhrt_kerr_ray_init(",
                                    "/* ---- Physical geodesics, adaptive steps:",
                                    "bhrt_kerr_rk45_rays(", "/* ---- Physical photon paths:")]
    assert at == sorted(at), at


def test_header_states_the_rule():
    header = " ".join(open(os.path.join(ROOT, "include", "bhrt_api.h")).read().split())
    header = header.replace(" * ", " ")   # (comment continuation marks)
    section = header[header.index("Physical geodesics, adaptive steps:"):
                     header.index("} bhrt_kerr_rk45_diag;")]
    for phrase in ("THE ADAPTIVE RULE", "tests/kerr_rk45_rule.py", "Dormand-Prince 5(4)",
                   "standard 7-stage tableau with FSAL", "5th-order solution",
                   "e = h sum_j (b5_j - b4_j) k_j", "a rejected attempt keeps its k1",
                   "h_try = min(h, r / 2)", "the first h is time_step",
                   "sc_c = tol (1 + max(|y_c|, |ynew_c|))", "err = max_c |e_c| / sc_c",
                   "fac = min(5, max(0.2, 0.9 err^(-1/5)))", "a non-finite fac is 0.2",
                   "h = h_try fac", "Accepted iff err <= 1", "steps is the number of attempts",
                   "in this order", "a non-finite ynew or err: RAY_ERROR", "only test 6 runs",
                   "cubic Hermite polynomial", "h_try k1_z and h_try k7_z",
                   "theta = z_old / (z_old - z_new)", "four Newton iterations",
                   "hit = (q_x, q_y, 0)", "distance += theta seg", "r_new <= r+: RAY_HORIZON",
                   "attempts >= max_integration_steps: RAY_MAX_STEPS", "EXIT TANGENT",
                   "unit Hermite derivative of position at theta", "accepted points only",
                   "BEFORE ANY HIP CALL", "finite and within [1e-12, 1e-2]",
                   "iterations counts attempts", "bhrt_kerr_paths* stays RK4"):
        assert phrase in section, phrase


def test_host_core_does_not_name_the_launcher():
    for f in host_core():
        assert "bhrt_launch_kerr" not in open(f).read(), f
    mine = os.path.join(CSRC, "kerr_rk45.c")
    assert mine in host_feature() and mine not in host_core()
    # the file names its own launcher and no other; the launcher is defined in exactly one unit
    text = open(mine).read()
    assert set(re.findall(r"\bbhrt_launch_\w+", text)) == {"bhrt_launch_kerr_rk45"}
    defined = [p for p in hip_sources()
               if re.search(r'extern "C" int bhrt_launch_kerr_rk45\(', open(p).read())]
    assert [os.path.basename(p) for p in defined] == ["kerr.hip"], defined
    assert "bhrt_launch_kerr_rk45(" in open(os.path.join(CSRC, "bhrt_kernel.h")).read()
    for other in host_feature():
        if other != mine:
            assert "bhrt_launch_kerr_rk45" not in open(other).read(), other
    # it shares kerr.c's checks through bhrt_host.h instead of restating them
    for shared in ("bhrt_kerr_scene(", "bhrt_kerr_out_bad(", "bhrt_kerr_observer(",
                   "bhrt_kerr_rays_check(", "bhrt_ctx_launch_fn("):
        assert shared in text, shared
    assert "hipHostRegister" not in text and "hipHostMalloc" not in text


def test_tableau_is_dormand_princes():
    """Row sums are the nodes, both weight sets sum to 1 and meet the order conditions up to
    sum b c^3 = 1/4 (5th) -- the embedded set's c^4 condition fails, as a 4th-order set's must."""
    rows = ((), k5.A2, k5.A3, k5.A4, k5.A5, k5.A6, k5.B5)
    c = np.array([sum(r) for r in rows])
    assert np.allclose(c, [0, 1 / 5, 3 / 10, 4 / 5, 8 / 9, 1, 1], atol=1e-15)
    b5 = np.array(k5.B5 + (0.0,))
    b4 = b5 - np.array(k5.EC)
    for b in (b5, b4):
        for p in range(4):
            assert abs(b @ c ** p - 1.0 / (p + 1)) < 1e-15, (p, b @ c ** p)
    assert abs(b5 @ c ** 4 - 0.2) < 1e-15 and abs(b4 @ c ** 4 - 0.2) > 1e-4
    assert abs(sum(k5.EC)) < 1e-16


@pytest.mark.parametrize("frame", FRAMES, ids=FRAME_IDS)
def test_rule_frames_against_rk4_and_against_itself(frame):
    """Per frame, at tolerance 1e-6 and 1e-8: every ray's class is the fixed-step rule's; the
    disk points are within the bounds above of the rule's own at tolerance 1e-13; and at 1e-8
    the frame's attempts are at most a quarter of the fixed-step rule's steps (measured 0.18)."""
    base = kr.frame_rule(*frame)
    ref = k5.frame_rule(*frame, k5.REF_TOL, max_steps=k5.REF_STEPS)
    assert np.array_equal(ref["result"], base["result"])
    for tol in k5.TOLS:
        got = k5.frame_rule(*frame, tol)
        differ = int((got["result"] != base["result"]).sum())
        disk = got["result"] == kr.DISK
        err = float(np.abs(got["hit"][disk] - ref["hit"][disk]).max())
        ratio = got["steps"].sum() / base["steps"].sum()
        print(f"{frame} tol {tol:g}: {int(got['steps'].sum())} attempts ({int(got['rejected'].sum())} "
              f"rejected, longest {int(got['steps'].max())}) of {int(base['steps'].sum())} RK4 steps "
              f"= {ratio:.3f}; classes differ on {differ}; disk points off by {err:.2e}; H residual "
              f"{got['h_residual'].max():.2e}, L_z drift {got['lz_drift'].max():.2e}")
        assert differ == 0
        assert disk.sum() > 100 and err <= DISK_POINT_BOUND[tol], (tol, err)
        assert (got["rejected"] <= got["steps"]).all() and got["rejected"].sum() > 0
        if tol == 1e-8:
            assert ratio <= 0.25, ratio
            assert got["h_residual"].max() < base["h_residual"].max()


@pytest.mark.parametrize("spin", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("tol", k5.TOLS)
def test_rule_fans_capture_and_escape_at_the_analytic_edge(spin, tol):
    """kerr_rule.fan from (20, 0, 0), both sides: rays with |b| below (1 - 1e-3) of the analytic
    critical value are captured, those above (1 + 1e-3) of it escape; at least 17 on each side of
    every edge."""
    for side in (1, -1):
        tr = k5.fan_trace(spin, side, tol)
        b = tr["b"]
        bc = kr.analytic_b(spin, b[0])
        inside, outside = np.abs(b) < (1.0 - DELTA) * abs(bc), np.abs(b) > (1.0 + DELTA) * abs(bc)
        assert inside.sum() >= 17 and outside.sum() >= 17, (bc, inside.sum(), outside.sum())
        assert (tr["result"][inside] == kr.HORIZON).all(), (side, b[inside], tr["result"][inside])
        assert (tr["result"][outside] == kr.MAX_DISTANCE).all(), (side, tr["result"][outside])


@pytest.mark.parametrize("tol", k5.TOLS)
def test_rule_knife_edge_set_of_the_six_frames(tol):
    """At most 1% of a frame's rays change class, attempts or rejected count under a +-1e-7
    direction perturbation (the set the GPU comparison leaves out; wider than the fixed-step
    rule's 1e-9 probe because rounding enters err relative to the tolerance). Measured: 0 on all
    twelve frame x tolerance cases, at 1e-9 and at 1e-7."""
    for frame in FRAMES:
        k = k5.knife_edge(*frame, tol)
        print(f"{frame} tol {tol:g}: knife-edge {int(k.sum())} of {len(k)}")
        assert k.sum() <= 0.01 * len(k), (frame, int(k.sum()))


def test_rule_edge_cases():
    """max_integration_steps == 0 ends at the origin; an origin without an observer is RAY_ERROR
    with 0 attempts; a budget of attempts counts rejected ones; the disk point lies on the disk
    plane, between the step's ends; a MAX_DISTANCE ray's tangent is xdot at its end point."""
    o = np.array([[0.0, -18.0, 4.0], [1.5, 0.0, 0.0]])
    d = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])
    tr = k5.trace(o, d, 0.9, 1.0, None, 0.25, 60.0, 0, 1e-8)
    assert tr["result"].tolist() == [kr.MAX_STEPS, kr.ERROR] and tr["steps"].tolist() == [0, 0]
    assert np.array_equal(tr["hit"], o) and (tr["distance"] == 0.0).all()
    assert tr["rejected"].tolist() == [0, 0]
    # a first trial step far too long is rejected, and the rejection is an attempt
    tr = k5.trace(o[:1], d[:1], 0.9, 1.0, None, 50.0, 60.0, 1, 1e-8)
    assert tr["result"][0] == kr.MAX_STEPS and tr["steps"][0] == 1 and tr["rejected"][0] == 1
    assert np.array_equal(tr["hit"][0], o[0]) and tr["distance"][0] == 0.0
    # h_try = min(h, r / 2): the same ray's first accepted step is no longer than r / 2
    tr = k5.trace(o[:1], d[:1], 0.9, 1.0, None, 50.0, 1e9, 1, 1e-2)
    assert tr["distance"][0] <= 0.5 * np.linalg.norm(o[0]) * 1.01
    f = k5.frame_rule(0.9, (2.4, 12.0), 48, 27, 1e-8)
    disk, far = f["result"] == kr.DISK, f["result"] == kr.MAX_DISTANCE
    assert (f["hit"][disk, 2] == 0.0).all()
    s2 = f["hit"][disk, 0] ** 2 + f["hit"][disk, 1] ** 2
    assert (s2 >= 2.4 ** 2 + 0.81).all() and (s2 <= 144.0 + 0.81).all()
    # far away xdot is p up to f u l = O(M / r): a nearly unit vector pointing outward
    t = f["chord"][far]
    assert np.all(np.abs(np.linalg.norm(t, axis=1) - 1.0) < 0.1)
    assert np.all((t * f["hit"][far]).sum(axis=1) > 0.0)


def test_refusals_without_a_device():
    """The tolerance's refusal, decided before any HIP call on a machine without a GPU too
    (tests/fakehip/kerr_rk45_driver.c counts the HIP calls: zero), beside a sample of the shared
    ones."""
    L = lib.load()
    n = 48 * 27
    arrays, soa = abi.alloc_soa(n, lib.KERR_FIELDS)
    for a in arrays.values():
        a[...] = 7
    rays = np.zeros(n, dtype=abi.RAY_DTYPE)
    rays["origin"] = (0.0, -18.0, 4.0)
    rays["direction"] = (0.0, 1.0, 0.0)
    cam = kr.camera()

    def calls(bh, dk, cfg):
        yield L.bhrt_kerr_rk45_frame(lib._ptr(bh), lib._ptr(dk), lib._ptr(cfg), lib._ptr(cam), 48,
                                     27, 0, lib._ptr(soa), None)
        yield L.bhrt_kerr_rk45_frame_device(lib._ptr(bh), lib._ptr(dk), lib._ptr(cfg),
                                            lib._ptr(cam), 48, 27, None, 0, lib._ptr(soa), None,
                                            None)
        yield L.bhrt_kerr_rk45_rays(rays.ctypes.data, n, lib._ptr(bh), lib._ptr(dk), lib._ptr(cfg),
                                    0, lib._ptr(soa), None)
        yield L.bhrt_kerr_rk45_rays_device(rays.ctypes.data, n, lib._ptr(bh), lib._ptr(dk),
                                           lib._ptr(cfg), 0, lib._ptr(soa), None, None)

    for tol in (0.0, -1e-8, 9.99e-13, 1.01e-2, 1.0, float("nan"), float("inf")):
        bh, dk, cfg = k5.scene(0.9, (2.4, 12.0), tol)
        for rc in calls(bh, dk, cfg):
            assert rc == -1 and "tolerance" in lib.last_error(), (tol, lib.last_error())
    bh, dk, cfg = k5.scene(0.9, (2.4, 12.0), 1e-8)
    cfg.time_step = 0.0
    for rc in calls(bh, dk, cfg):
        assert rc == -1 and "time_step" in lib.last_error()
    bh, dk, cfg = k5.scene(0.9, (2.4, 12.0), 1e-8)
    bh.spin = 1.0
    for rc in calls(bh, dk, cfg):
        assert rc == -1 and "spin" in lib.last_error()
    for a in arrays.values():
        assert (a == 7).all()
    with pytest.raises(lib.BhrtError, match="tolerance"):
        lib.kerr_rk45_frame(*k5.scene(0.9, (2.4, 12.0), 1e-13), cam, 8, 8)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_kerr_rk45_demo_builds_against_the_drop_in_headers(tmp_path):
    exe = str(tmp_path / "kerr_rk45_demo")
    path = os.path.abspath(lib.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", "kerr_rk45_demo.c"), path,
                    f"-Wl,-rpath,{os.path.dirname(path)}", "-lm", "-o", exe], check=True)
    assert os.path.exists(exe)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_host_code_on_simulated_devices_asan_ubsan(tmp_path):
    """tests/fakehip/kerr_rk45_driver.c: every refusal -- 33 argument sets through all four
    calls, the tolerance's eight among them, and 24 of single calls -- with the HIP calls
    counted (zero), the constants
    and tile counts a launch carries, the tolerance's bounds, shards and offsets, ray arrays, the
    host forms' round trips with the rejected plane, the statistics."""
    exe = str(tmp_path / "kerr_rk45_asan")
    wrapped = ("hipMalloc", "hipFree", "hipMemcpy", "hipMemcpyAsync", "hipSetDevice", "hipGetDevice",
               "hipStreamSynchronize", "hipEventRecord", "hipStreamWaitEvent", "hipHostMalloc")
    cmd = ["gcc", "-fopenmp", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
           "-I", "/opt/rocm/include", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           os.path.join(FAKE, "kerr_rk45_driver.c"), os.path.join(FAKE, "fake_hip.c"),
           os.path.join(CSRC, "kerr_rk45.c"), os.path.join(CSRC, "kerr.c"), *host_core(),
           "-Wl," + ",".join("--wrap=" + w for w in wrapped), "-lpthread", "-lm", "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-6000:]
    env = dict(os.environ, FAKEHIP_DEVICES="2", ASAN_OPTIONS="detect_leaks=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for name in ("HIP_VISIBLE_DEVICES", "BHRT_NULL_STREAM", "BHRT_FUSE_COLOUR", "BHRT_MAX_DEVICES"):
        env.pop(name, None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    m = re.search(r"all checks passed \((\d+) refusals, (\d+) adaptive launches\)", r.stdout)
    assert m, r.stdout[-2000:]
    # 33 x 4 = 132, of which 8 x 4 are the tolerance's; 24 single calls: the observer (12),
    # camera, size, sharding, n, rays and the sky flag (2 each)
    refusals, launches = int(m.group(1)), int(m.group(2))
    assert refusals == EXPECTED_REFUSALS and launches == EXPECTED_LAUNCHES, (refusals, launches)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, \
        r.stderr[-4000:]


EXPECTED_REFUSALS, EXPECTED_LAUNCHES = 156, 11
