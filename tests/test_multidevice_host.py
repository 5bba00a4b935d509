"""libbhrt's host layer on SIMULATED devices, without a GPU (multi-device state).

tests/fakehip/fake_hip.c stands in for the HIP runtime with host memory tagged by device and
synchronous streams, and aborts on a cross-device stream, event, copy or launch buffer, or on
an asynchronous D2H copy into host memory that is not pinned, or on any page-locking of caller
memory (libbhrt registers none).
tests/fakehip/multidev_driver.c stubs the trace launcher (it checks every launch buffer
against the current device and writes an encoding of each ray's image pixel) and drives,
from two host threads at once, frames split over two devices and several chunks (staged,
frames in flight) and ray batches split over the devices,
checking that every value lands at its pixel. Built twice: ASan+UBSan and TSan."""
import glob
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from host_sources import host_core, host_feature

CSRC = os.path.join(ROOT, "raytracing-engine-in-c_amd", "csrc")
FAKE = os.path.join(ROOT, "tests", "fakehip")


def test_every_host_file_is_in_exactly_one_makefile_list():
    """Every csrc/*.c is in HOST_CORE (what the drivers here and in test_sanitizers.py link) or
    in HOST_FEATURE, never both: a new file cannot silently miss the sanitizer builds."""
    listed = sorted(host_core() + host_feature())
    assert len(set(listed)) == len(listed), listed
    assert listed == sorted(glob.glob(os.path.join(CSRC, "*.c")))


def build(tmp_path, name, sanitize, openmp):
    exe = str(tmp_path / name)
    cmd = ["gcc", "-std=gnu11", "-O1", "-g", f"-fsanitize={sanitize}", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", "/opt/rocm/include",
           "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           os.path.join(FAKE, "multidev_driver.c"), os.path.join(FAKE, "fake_hip.c"),
           *host_core(), "-lpthread", "-lm", "-o", exe]
    if openmp:
        cmd.insert(1, "-fopenmp")
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def run(exe, **env):
    e = dict(os.environ, FAKEHIP_DEVICES="2", **env)
    e.pop("HIP_VISIBLE_DEVICES", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    assert "all checks passed" in r.stdout
    return r


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_two_simulated_devices_asan_ubsan(tmp_path):
    exe = build(tmp_path, "multidev_asan", "address,undefined", openmp=True)
    env = {"ASAN_OPTIONS": "detect_leaks=0", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    # the default chunk plan, and trace_rays_batch's weighted plans (BHRT_BATCH_WEIGHTS: small
    # first and last chunks, chunk counts 2..8)
    # (and libbhrt's streams made each way BHRT_STREAM_QUEUE offers)
    for weights, queue in ((None, "0"), ("1,5,5,4,1", "1"), ("3,1", "2"), ("1,2,3,4,5,6,7,8", "0")):
        extra = {"BHRT_STREAM_QUEUE": queue}
        if weights:
            extra["BHRT_BATCH_WEIGHTS"] = weights
        r = run(exe, **env, **extra)
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc")
def test_two_simulated_devices_tsan(tmp_path):
    """Two host threads through the same library: per-thread contexts must not race. Built
    without OpenMP (libgomp is not TSan-instrumented); the host copies then run serially."""
    exe = build(tmp_path, "multidev_tsan", "thread", openmp=False)
    r = run(exe, TSAN_OPTIONS="halt_on_error=1")
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-6000:]
