"""The path kernels' inputs on the scene sweep, without a GPU (tests/paths_sweep_rule.py).

The oracle's orc_integrate_photon_path against the compiled reference's recorded digests
(tests/golden/sweep_paths_<k>.npz, gen_sweep_paths.py) on every sweep scene and every edge ray,
and the proof that those rays are decisive for the branches only the path kernels have: the GPU
tests (tests/test_gpu_paths_sweep.py) may excuse a hand-written ray whose oracle margin is below
KNIFE_EDGE and nothing else.

Measured with the oracle on the 41 scenes x 181 rays (3.87 M path points, none non-finite):
knife-edge rays only among the hand-written ones, at most 16 per scene with the scene's disk and
15 with disk = NULL (both in m1e3); 1905 (scene, ray) pairs end on the disk; 1345 full paths hold
a repeated point; 72 disk hits land on a duplicate segment (dt0_rk4 21, tol_lo_s 17, dist_0 9,
disk_thin_ring 1, leapfrog 22, m40 2).
"""
import os

import numpy as np
import pytest

import paths_sweep_rule as rule
import sweep_scenes as sw
from conftest import KNIFE_EDGE, golden
from bhrt import abi
from test_paths_cpu import TRACE_FIELDS, oracle_paths
from test_scene_sweep import HAND_RAYS, REACHABLE_CLASSES, REF_RTOL

KNIFE_CAP = 16  # hand-written rays per scene and disk argument that the GPU tests may excuse
DUPLICATE_HIT_SCENES = ("dt0_rk4", "tol_lo_s", "dist_0", "disk_thin_ring", "leapfrog", "m40")
REPEATED_POINT_SCENES = ("tol_0_kerr", "tol_nan_kerr", "dt0_rk4", "leapfrog")


def test_fixture_files_obey_the_size_caps():
    files = rule.fixture_files()
    sizes = [os.path.getsize(p) for p in files]
    assert len(files) == -(-len(sw.SCENES) // rule.PATH_GROUP), files
    assert max(sizes) < 230_000 and sum(sizes) < 700_000, sizes
    fx = rule.fixtures()
    assert set(fx) == set(sw.SCENES)
    for name, f in fx.items():
        assert f["res"].dtype == np.int32 and f["res"].shape == (181, 4), name
        assert f["sum"].dtype == np.float64 and f["sum"].shape == (181, 4), name
        assert f["pts"].dtype == np.float64 and f["pts"].shape == (46, 3, 3), name


def test_digest_is_the_stated_rule():
    q = np.array([[1.0, -2.0, 3.0], [1e16, 1.0, -1.0], [-1e16, 0.5, 0.25], [4.0, 0.0, -8.0]])
    s, p = rule.digest(q)
    want = [((1.0 + 1e16) + -1e16) + 4.0, ((-2.0 + 1.0) + 0.5) + 0.0, ((3.0 + -1.0) + 0.25) + -8.0,
            ((6.0 + (1e16 + 1.0 + 1.0)) + (1e16 + 0.5 + 0.25)) + 12.0]
    assert s.tolist() == want                       # left to right: x sums to 4, not to 5
    assert p.tolist() == q[[1, 2, 3]].tolist()
    assert rule.pts_indices(1) == [0, 0, 0] and rule.pts_indices(2) == [1, 1, 1]
    assert rule.pts_indices(1001) == [1, 500, 1000]


@pytest.mark.parametrize("name", list(sw.SCENES))
def test_oracle_paths_vs_reference(oracle, name):
    """Every ray of every scene: return value, count, hit class and hit steps exact; the stored
    points rtol 1e-12; each coordinate sum within 1e-12 of the recorded sum of absolutes, that
    sum rtol 1e-12; NaN patterns identical."""
    want = rule.fixtures()[name]
    got = rule.scene_digest(oracle.lib.orc_integrate_photon_path, name)
    assert np.array_equal(got["res"], want["res"]), np.nonzero(got["res"] != want["res"])[0][:10]
    for f in ("sum", "pts"):
        assert np.array_equal(np.isnan(got[f]), np.isnan(want[f])), (name, f)
    ok = ~np.isnan(want["pts"])
    a, b = got["pts"][ok], want["pts"][ok]
    assert (np.abs(a - b) <= REF_RTOL * np.maximum(np.abs(a), np.abs(b))).all(), name
    for i in range(181):
        g, w = got["sum"][i], want["sum"][i]
        if np.isnan(w).any():
            continue
        assert abs(g[3] - w[3]) <= REF_RTOL * max(abs(g[3]), abs(w[3])), (name, i, g[3], w[3])
        assert (np.abs(g[:3] - w[:3]) <= REF_RTOL * w[3]).all(), (name, i, g, w)


def _measure(oracle, name, dk):
    """What one scene holds for one disk argument: the margins, the class that ends each path,
    the path lengths, and which rays' disk hit lands on a duplicate segment."""
    bh, _, cfg, method, _, _ = sw.scene(name)
    rays = rule.edge_rays()
    out, margin = oracle.trace_rays_margin(rays, bh, dk, cfg, method, 0, fields=TRACE_FIELDS)
    paths = oracle_paths(oracle, rays, bh, dk, cfg, method)
    full = paths if dk is None else oracle_paths(oracle, rays, bh, None, cfg, method)
    dup = []
    for i in range(len(rays)):
        h = int(out["steps"][i])
        if dk is not None and out["result"][i] == abi.RAY_DISK and 1 <= h < len(full[i]):
            assert len(paths[i]) == h + 1, (name, i)
            if np.array_equal(full[i][h], full[i][h - 1]):
                dup.append(i)
    # a repeated point: two equal consecutive points in a full path of more than two (a
    # two-point path that ends where it began has no jump for the kept indices to cross)
    repeated = [i for i, q in enumerate(full)
                if len(q) > 2 and (q[1:] == q[:-1]).all(axis=1).any()]
    finite = all(np.isfinite(q).all() for q in paths)
    return dict(margin=margin, result=out["result"], lens=np.array([len(q) for q in paths]),
                dup=dup, repeated=repeated, finite=finite, points=sum(len(q) for q in full))


def test_path_sweep_inputs_are_decisive(oracle):
    """Guards the GPU tests against excusing failures (oracle only), for each scene's disk and
    for disk = NULL: no ray of index >= 21 is knife-edge and at most KNIFE_CAP hand-written ones
    are per scene; every reachable class ends some path; the listed scenes hold a disk hit on a
    duplicate segment and at least 100 rays with a repeated point; every scene but dist_0 holds
    a path of 2 points and one of max_steps + 1."""
    seen = {"disk": set(), "null": set()}
    total = dict(disk_hits=0, repeated=0, dup=0, points=0)
    worst = {"disk": (0, ""), "null": (0, "")}
    for name in sw.SCENES:
        _, dk, cfg, _, _, _ = sw.scene(name)
        for arg in ("disk", "null"):
            if arg == "disk" and dk is None:
                continue
            m = _measure(oracle, name, dk if arg == "disk" else None)
            rest = m["margin"][HAND_RAYS:]
            assert (rest >= KNIFE_EDGE).all(), (name, arg,
                                                HAND_RAYS + np.nonzero(~(rest >= KNIFE_EDGE))[0])
            knife = int((~(m["margin"][:HAND_RAYS] >= KNIFE_EDGE)).sum())  # (a NaN margin counts)
            assert knife <= KNIFE_CAP, (name, arg, knife)
            worst[arg] = max(worst[arg], (knife, name))
            assert m["finite"], (name, arg)
            seen[arg] |= set(np.unique(m["result"]).tolist())
            lens = m["lens"]
            if name == "dist_0":
                assert (lens == 2).all(), (arg, lens)
            else:
                assert lens.min() == 2 and lens.max() == cfg.max_integration_steps + 1, (
                    name, arg, lens.min(), lens.max())
            if arg == "disk":
                total["disk_hits"] += int((m["result"] == abi.RAY_DISK).sum())
                total["dup"] += len(m["dup"])
                if name in DUPLICATE_HIT_SCENES:
                    assert len(m["dup"]) >= 1, name
                if m["dup"]:
                    print(f"PATHS_SWEEP_DUP {name} {len(m['dup'])} rays {m['dup']}")
            else:
                total["repeated"] += len(m["repeated"])
                total["points"] += m["points"]
                if name in REPEATED_POINT_SCENES:
                    assert len(m["repeated"]) >= 100, (name, len(m["repeated"]))
    print(f"PATHS_SWEEP_INPUTS {total} most knife-edge hand rays {worst}")
    assert seen["disk"] == REACHABLE_CLASSES, seen
    assert seen["null"] == REACHABLE_CLASSES - {abi.RAY_DISK}, seen


@pytest.mark.parametrize("name", list(rule.REPAIRED_SCENES))
def test_repaired_origin_rays(oracle, name):
    """The rays with a non-finite origin (paths_sweep_rule.REPAIRED_SCENES): the oracle equals
    the compiled reference (classes, counts and steps exact, floats 1e-12, NaN and infinity at
    the same places), and the rays are decisive for the branch they are there for: none is
    knife-edge, and at least ten hit the disk on segment 2 with q_2 == q_1 finite and q_0 not."""
    bh, dk, cfg, method = rule.repaired_scene(name)
    rays = rule.repaired_rays()
    want = {k.split(".")[1]: v for k, v in golden("paths_repaired_origin").items()
            if k.split(".")[0] == name}
    path, res = rule.full_paths(oracle.lib.orc_integrate_photon_path, rays, bh, cfg, method)
    trace, margin = oracle.trace_rays_margin(rays, bh, dk, cfg, method, 0,
                                             fields=rule.REPAIRED_FIELDS)
    assert np.array_equal(res, want["res"])
    for f in ("result", "steps"):
        assert np.array_equal(trace[f], want[f]), f
    for a, b in [(path, want["path"])] + [(trace[f], want[f]) for f in rule.REPAIRED_FIELDS[2:]]:
        for pattern in (np.isnan, np.isposinf, np.isneginf):
            assert np.array_equal(pattern(a), pattern(b)), pattern.__name__
        ok = np.isfinite(b)
        assert (np.abs(a[ok] - b[ok]) <= REF_RTOL * np.abs(b[ok])).all()
    behind = [i for i in range(len(rays))
              if trace["result"][i] == abi.RAY_DISK and trace["steps"][i] == 2
              and np.isfinite(path[i, 1]).all() and np.array_equal(path[i, 2], path[i, 1])
              and not np.isfinite(path[i, 0]).all()]
    assert len(behind) >= 10, behind
    assert (margin >= KNIFE_EDGE).all(), margin  # no ray at all: the GPU test excuses nothing
    assert (trace["result"] != abi.RAY_DISK).sum() >= 10  # and stuck rays that never hit
