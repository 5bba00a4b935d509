"""The layout of the device side (csrc/*.hip, bhrt_trace_core.h), as text: the Makefile builds
every .hip file there is, every launcher the host layer calls is defined once, and no unit
carries a copy of a device function the shared headers define."""
import glob
import os
import re
import subprocess

from host_sources import CSRC, hip_sources

CORE, COLOUR = '#include "bhrt_trace_core.h"', '#include "bhrt_colour.h"'
LAUNCHER = r"(bhrt_launch_\w+|bhrt_trace_untested)\("


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _device_defs(text):
    """Names of the device functions and kernels a text defines at file level: `__device__ ...
    name(` / `__global__ ... name(` at the start of a line (bodies and calls are indented), the
    __attributes__ in between, and their arguments, taken out."""
    names = set()
    for m in re.finditer(r"^__(?:device|global)__ ([^\n]*)", text, re.M):
        rest = re.sub(r"__\w+__(?:\(\(?[^()]*\)?\))?", "", m.group(1))
        name = re.search(r"\b(\w+)\(", rest)
        if name:
            names.add(name.group(1))
    return names


def test_makefile_lists_every_hip_file():
    listed = hip_sources()
    assert len(listed) == len(set(listed))
    assert sorted(listed) == sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def test_no_rule_makes_a_hip_source_from_its_object():
    """X.hip compiles to X.hip.o, and make's built-in `%: %.o` would link X.hip from it, over the
    source: the Makefile runs without built-in rules."""
    rules = subprocess.run(["make", "-C", CSRC, "-n", "-p", "print-hip"], capture_output=True,
                           text=True, check=True).stdout
    assert "%.hip.o: %.hip" in rules
    assert not re.search(r"^%: %\.o$", rules, re.M)


def test_every_launcher_is_defined_in_exactly_one_unit():
    declared = set(re.findall(r"^int " + LAUNCHER, _read("bhrt_kernel.h"), re.M))
    assert {"bhrt_launch_trace", "bhrt_launch_paths", "bhrt_launch_ta_blend", "bhrt_launch_kerr",
            "bhrt_launch_particles", "bhrt_trace_untested"} <= declared
    defined = {os.path.basename(p): re.findall(r'^extern "C" int ' + LAUNCHER, open(p).read(), re.M)
               for p in hip_sources()}
    for name in sorted(declared):
        owners = [unit for unit, names in defined.items() for n in names if n == name]
        assert len(owners) == 1, (name, owners)
    # and nothing but the declared ones goes by these names
    assert {n for names in defined.values() for n in names} == declared


def test_no_unit_redefines_a_shared_device_function():
    colour = _device_defs(_read("bhrt_colour.h"))
    core = _device_defs(_read("bhrt_trace_core.h")) | colour
    assert {"rhs", "rk4_step", "rkf45_attempt", "ray_iterate", "store_hit", "wave_sum",
            "sincos_ocml", "camera_dir"} <= core and {"store_colour", "sky_lookup"} <= colour
    users = []
    for path in hip_sources():
        text = open(path).read()
        if CORE in text:
            users.append(os.path.basename(path))
            shared = core
        elif COLOUR in text:
            shared = colour  # (kerr.hip: its own arithmetic under its own names)
        else:
            continue
        again = shared & _device_defs(text)
        assert not again, (path, sorted(again))
    assert sorted(users) == ["checks.hip", "frames.hip", "geodesic.hip", "paths.hip"]
