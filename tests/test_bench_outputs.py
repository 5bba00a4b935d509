"""bench.py as a plain run on the GPU: the result line and --dump-outputs.

A plain run (no --full) times its frames and prints one JSON line without the side legs;
--dump-outputs DIR leaves the last timed frame as DIR/<field>.npy in float64 / float32 -- every
ray of a small frame (C1), the same seeded sample of rays for every field of a large one (C2,
whose 2 073 600 rays x 120 B exceed the budget). The timed path is bhrt_render_frame_device, whose
frames equal bhrt_render_frame's bit for bit (test_device_api_on_torch_stream), so the dumped
values must EQUAL a host-API render of the same frame here.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bhrt import abi, configs
from conftest import ROOT

pytestmark = pytest.mark.gpu

FIELDS = abi.SOA_FIELDS + ("rgba8",)
LIMIT_BYTES = 64 << 20  # of .npy files in all


@pytest.mark.parametrize("cname,sampled", [("C1", False), ("C2", True)])
def test_plain_run_dumps_the_last_timed_frame(bhrt_lib, tmp_path, cname, sampled):
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "BHRT_BENCH_DRYRUN")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config",
                        cname, "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["unit"] == "Mrays/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["value"] > 0 and line["ms_per_step"] > 0
    c = configs.CONFIGS[cname]
    n = c.width * c.height
    # value and ms_per_step are the same measurement (each rounded: 3 and 6 decimals)
    assert line["value"] == pytest.approx(n / line["ms_per_step"] / 1e3, rel=1e-3)
    for leg in ("cpu_baseline", "max_rel_dhit", "class_mismatch", "host_path", "display_resident"):
        assert leg not in line, leg  # (the side legs run with --full only)

    names = sorted(os.listdir(out))
    want_names = sorted([f + ".npy" for f in FIELDS] + (["sample_index.npy"] if sampled else []))
    assert names == want_names
    got = {x[:-4]: np.load(out / x, allow_pickle=False) for x in names}
    assert sum(os.path.getsize(out / x) for x in names) <= LIMIT_BYTES
    if sampled:
        idx = got.pop("sample_index")
        assert idx.dtype == np.float64 and np.all(idx == np.floor(idx))
        idx = idx.astype(np.int64)
        assert len(idx) > 100_000 and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < n
    else:
        idx = np.arange(n)
    bh, dk, cfg = c.scene()
    want = bhrt_lib.render_frame(bh, dk, cfg, configs.camera("B"), c.width, c.height, c.method,
                                 c.flags, fields=FIELDS)
    bhrt_lib.stats(reset=True)
    for f in FIELDS:
        a = got[f]
        assert a.dtype == (np.float32 if f == "rgba8" else np.float64), f
        assert a.shape == ((len(idx), 4) if f == "rgba8" else (len(idx),)), (f, a.shape)
        assert np.array_equal(a, want[f][idx].astype(a.dtype), equal_nan=True), f
