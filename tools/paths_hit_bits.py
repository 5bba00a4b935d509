"""Where the batched path kernel's integration and the trace kernel's differ in their last bits.

For the rays of tests/golden/path_batch.npz and the C2 camera crop of tests/test_gpu_paths.py:
the last stored point of each ray's full path (bhrt_trace_paths_device, every = 1: k_paths'
own integration, the single-ray kernel's instantiation) against the hit position that
bhrt_trace_rays_device records for the same ray, and, without a disk, against the single-ray
integrate_photon_path's. One line per scene: how many rays differ, the largest relative
difference and the first pair. k_paths equals the single-ray kernel bit for bit; the trace
kernel's multi-iteration trips round a long ray's end differently, which is why
bhrt_trace_paths_device takes its hit records from a trace launch instead of writing them from
its own state (profiles/paths/hits_bits.txt)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402,F401  (puts the package and the oracle on the path)
from bhrt import abi, lib  # noqa: E402
import test_gpu_paths as g  # noqa: E402


def single_ray_ends(L, s):
    out = []
    for ray in s["rays"]:
        hit, num = abi.RayTraceHit(), C.c_int(0)
        o, d = [float(x) for x in ray["origin"]], [float(x) for x in ray["direction"]]
        L.integrate_photon_path(C.byref(abi.Vector4D(0.0, *o)), C.byref(abi.v3(*d)),
                                C.byref(s["bh"]), C.byref(s["cfg"]), s["method"], None, 0,
                                C.byref(num), C.byref(hit))
        out.append([hit.hit_position.x, hit.hit_position.y, hit.hit_position.z])
    return np.array(out)


def report(name, a, b, what):
    ne = (a != b).any(axis=1)
    if not ne.any():
        print(f"{name}: last point == {what}, bit for bit ({len(a)} rays)")
        return
    rel = np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-300)
    i = int(np.nonzero(ne)[0][0])
    print(f"{name}: last point != {what} on {int(ne.sum())} of {len(a)} rays, largest relative "
          f"difference {rel.max():.3g}; first ray {i}: {a[i].tolist()!r} vs {b[i].tolist()!r}")


def main():
    L = lib.load()
    for name in g.NAMES + ["crop"]:
        args = g.crop()[:5] if name == "crop" else g.scene_args(g.scenes()[name])
        P = args[3].max_integration_steps + 1
        got = g.run_device(lib, *args, P, 1)
        last = got["xyz"][np.arange(len(args[0])), got["count"] - 1]
        trace = np.stack([got["hit_x"], got["hit_y"], got["hit_z"]], axis=1)  # the trace launch's
        report(name, last, trace, "bhrt_trace_rays_device's hit position")
        if name != "crop" and args[2] is None:
            report(name, last, single_ray_ends(L, g.scenes()[name]),
                   "integrate_photon_path's hit position")


if __name__ == "__main__":
    main()
