"""Generate tests/golden/sweep_paths_<k>.npz from the COMPILED REFERENCE (oracle/_ref/libref.so).

Run in the build container only (the reference sources are not on the GPU box):

    make -C oracle ref && python tests/golden/gen_sweep_paths.py

For every scene of the sweep (tests/sweep_scenes.py) and each of the 181 edge rays of
rays_rk4_disk.npz the reference's integrate_photon_path(origin with t = 0, direction, the
scene's method, max_positions = max_steps + 1) is run and a digest of its outputs is stored
(tests/paths_sweep_rule.py: return value, count and hit class, four running sums over the
path's points, three points of every fourth ray). The full paths would be 93 MB.

Fixture contents are data only: the reference's outputs, keyed by scene name (the table is the
source of truth for the inputs). tests/golden/paths_repaired_origin.npz holds the full paths and
trace_ray's results of the 48 rays with a non-finite origin in three scenes of
paths_sweep_rule.REPAIRED_SCENES (the duplicate segment that hits behind the first stuck point).
The files' bytes depend on the arrays alone (gen_golden.py save_fixed), so a rerun reproduces
them byte for byte.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from gen_golden import REF, save_fixed  # noqa: E402
import paths_sweep_rule as rule  # noqa: E402
import sweep_scenes as sw  # noqa: E402

FILE_LIMIT, TOTAL_LIMIT = 230_000, 700_000


def main():
    names = list(sw.SCENES)
    REF.quiet(1)
    try:
        for g in range(0, len(names), rule.PATH_GROUP):
            arrays = {}
            for name in names[g:g + rule.PATH_GROUP]:
                for f, v in rule.scene_digest(REF.lib.integrate_photon_path, name).items():
                    arrays[f"{name}.{f}"] = v
            save_fixed(f"sweep_paths_{g // rule.PATH_GROUP}", arrays)
    finally:
        REF.quiet(0)
    arrays = {}  # the rays whose duplicate segment hits at segment 2 (paths_sweep_rule.py)
    for name in rule.REPAIRED_SCENES:
        bh, dk, cfg, method = rule.repaired_scene(name)
        rays = rule.repaired_rays()
        REF.quiet(1)
        try:
            path, res = rule.full_paths(REF.lib.integrate_photon_path, rays, bh, cfg, method)
        finally:
            REF.quiet(0)
        trace = REF.trace_rays(rays, bh, dk, cfg, method, 0, fields=rule.REPAIRED_FIELDS)
        arrays[f"{name}.path"], arrays[f"{name}.res"] = path, res
        for f in rule.REPAIRED_FIELDS:
            arrays[f"{name}.{f}"] = trace[f].astype(np.int32) if f in ("result", "steps") else trace[f]
    save_fixed("paths_repaired_origin", arrays)
    sizes = [os.path.getsize(p) for p in rule.fixture_files()]
    assert max(sizes) < FILE_LIMIT and sum(sizes) < TOTAL_LIMIT, sizes
    print("sweep_paths:", sizes, "bytes, total", sum(sizes), file=sys.stderr)


if __name__ == "__main__":
    main()
