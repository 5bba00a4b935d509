"""The per-age table of tools/shift_deltas.py (--ages): at which iteration of its life a ray's
far-anchor shifts (stage 2's and stage 4's theta, the advances of state[2] and state[3]) are
beyond the 1/64 bound of the narrow-first form (bhrt_trace_core.h BHRT_NARROW_SITES). CPU only:
the numpy replay against the oracle's step counts."""
import os
import sys

import numpy as np

from conftest import ROOT
from bhrt import configs

sys.path.insert(0, os.path.join(ROOT, "tools"))
import shift_deltas  # noqa: E402

SETTLED = 8  # profiles/nursery/shift_ages.txt: from this age on no camera-B lane is beyond 1/64


def test_camera_b_rays_are_settled_after_seven_iterations(oracle):
    """Camera B at 96 x 54: every lane beyond 1/64 at any of the four sites is in the first seven
    iterations of its ray; every ray alive then is such a lane in iterations 2..5; none is from
    iteration SETTLED to the step budget."""
    res = shift_deltas.replay(configs.camera("B"), 96, 54, oracle)
    ages = res["ages"]
    assert len(ages["alive"]) == 1000 and ages["alive"][-1] > 0  # rays run to the step budget
    K = shift_deltas.settled_age(ages)
    print("camera B 96x54: settled age", K, "; lanes beyond 1/64 by age 1..8:",
          {s: ages[s][:8].tolist() for s in shift_deltas.AGE_SITES})
    assert 0 < K < SETTLED
    for s in shift_deltas.AGE_SITES:
        assert ages[s][SETTLED - 1:].sum() == 0, s
        assert (ages[s] <= ages["alive"]).all(), s
    for k in range(1, 5):
        assert ages["stage4"][k] == ages["alive"][k] > 0
    # the age table's totals are the site table's: lanes beyond 1/64 over the whole frame
    j64 = shift_deltas.TS.index(1 / 64)
    for s in shift_deltas.AGE_SITES:
        assert int(ages[s].sum()) == int(res[s]["lane_over"][j64]), s
    assert int(ages["alive"].sum()) == res["lane_evals"]


def test_settled_age_of_made_up_tables():
    z = np.zeros(6, dtype=np.int64)
    ages = {s: z.copy() for s in shift_deltas.AGE_SITES}
    ages["alive"] = np.full(6, 9)
    assert shift_deltas.settled_age(ages) == 0
    ages["adv_y2"][3] = 2
    assert shift_deltas.settled_age(ages) == 4
    ages["stage2"][0] = 1
    assert shift_deltas.settled_age(ages) == 4
