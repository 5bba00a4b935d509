"""The trace loop's high-word guard (bhrt_trace_core.h all_below_2): the plain-value
test of a stage's three accelerations is filtered by one OR of their high words and one 32-bit
compare, and a lane the filter holds back takes the exact test (every |d| <= 10) in the rare
block before anything else.

  * the filter and the exact test on crafted operands (bhrt_check_guard_words, the device helper
    the loop uses): the filter never keeps a triple the exact test fails, and it is exactly "all
    three finite and below 2 in magnitude" -- so it holds back no triple below 2 (a filter that
    always said "rare block" would fail);
  * 64 x 36 frames against the oracle, every ray compared: C2 from camera B, from camera A on
    the polar axis and from the close "polar" camera of test_gpu_shift_chain (where the |d| <= 10
    clamp binds, so lanes run the rare block's exact test and the literal form inside the frame),
    and a C4 and a C5 frame.

Measured figures are in profiles/guardwords/test_figures.txt."""
import ctypes as C

import numpy as np
import pytest

import guard_words_rule as gw
from conftest import compare, sky_pinned
from bhrt import abi, configs
from test_gpu_parity import RTOL
from test_gpu_shift_chain import CAMS as CHAIN_CAMS

W, H = 64, 36
FRAMES = [("C2", "B"), ("C2", "A"), ("C2", "polar"), ("C4", "B"), ("C5", "B")]


def _camera(name):
    if name in configs.CAMERAS:
        return configs.camera(name)
    p, fov = CHAIN_CAMS[name]
    return abi.Camera(abi.v3(*p), abi.v3(*[-x for x in p]), abi.v3(0.0, 0.0, 1.0), fov)


def _guard_words(bhrt_lib, triples, kind=0):
    import torch
    t = np.ascontiguousarray(triples, dtype=np.float64)
    d_a = torch.from_numpy(t.ravel()).cuda()
    out = torch.full((len(t), 2), -7, dtype=torch.int32, device="cuda")
    rc = bhrt_lib.check_guard_words(d_a.data_ptr(), None, len(t), kind, out.data_ptr(),
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.gpu
def test_filter_on_operands(bhrt_lib):
    """Special operands (each threshold, its neighbours, the first double of the neighbouring
    high words, +-0, denormals, +-Inf, both NaNs, +-2^1017, +-2^-1017) in every position, 4096
    random triples over [1e-8, 30] and NaN / Inf in each position."""
    sets = {"special": gw.special_triples(), "random": gw.random_triples(4096),
            "non-finite": gw.nonfinite_triples()}
    for what, t in sets.items():
        rc, out = _guard_words(bhrt_lib, t)
        assert rc == 0, what
        f, e = out[:, 0] == 1, out[:, 1] == 1
        assert set(np.unique(out)) <= {0, 1}, what
        # condition 1: the filter keeps no triple that the exact test fails
        assert not (f & ~e).any(), (what, t[f & ~e][:5])
        # the exact test is the stated one, and the filter exactly "all finite and below 2":
        # no triple below 2 is held back
        assert np.array_equal(e, gw.exact_test(t)), (what, t[e != gw.exact_test(t)][:5])
        assert np.array_equal(f, gw.below_2(t)), (what, t[f != gw.below_2(t)][:5])
        assert np.array_equal(f, gw.filter_words(t)), what
        print(f"guard words, {what}: {len(t)} triples, {int(f.sum())} kept by the filter, "
              f"{int((~f & e).sum())} sent back by the exact test, {int((~e).sum())} to the "
              f"literal form")
    rc, out = _guard_words(bhrt_lib, sets["non-finite"])
    assert not out.any()


@pytest.mark.gpu
def test_other_kind_is_refused(bhrt_lib):
    """bhrt_check_guard_words knows kind 0; any other is an error and nothing is launched."""
    rc, out = _guard_words(bhrt_lib, gw.random_triples(8), kind=1)
    assert rc != 0 and (out == -7).all()


@pytest.fixture(scope="module")
def oracle_frames(oracle):
    cache = {}

    def get(cname, camname):
        if (cname, camname) not in cache:
            c = configs.CONFIGS[cname]
            bh, dk, cfg = c.scene()
            cache[cname, camname] = oracle.render_frame(bh, dk, cfg, _camera(camname), W, H,
                                                        c.method, c.flags)
        return cache[cname, camname]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("cname,camname", FRAMES)
def test_small_frames_vs_oracle(bhrt_lib, oracle_frames, cname, camname):
    """result and steps equal the oracle's for EVERY ray of the frame, the float fields within
    the parity tests' tolerance; no ray is left out."""
    c = configs.CONFIGS[cname]
    bh, dk, cfg = c.scene()
    want = oracle_frames(cname, camname)
    got = bhrt_lib.render_frame(bh, dk, cfg, _camera(camname), W, H, c.method, c.flags)
    assert len(got["result"]) == W * H
    worst = compare(got, want, RTOL, sky_pinned(c.method), f"{cname} camera {camname}")
    print(cname, camname, "rays", W * H, "classes",
          np.bincount(got["result"], minlength=5).tolist(), "max rel err", worst)
