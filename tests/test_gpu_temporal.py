"""Temporal accumulation on the GPU (bhrt_accum_*): one jittered plain frame per step, blended
into the accumulator's running image by k_ta_blend / k_ta_edges. The rule is stated in
include/bhrt_api.h; tests/temporal_rule.py restates it in numpy float32 and holds the case table,
on which test_temporal_cpu.py::test_cases_on_the_oracle shows that no ray is a knife-edge ray and
how few display values the powf exemption covers.

Display bytes: identical to the rule's, except that a byte may differ by 1 where 0 < c' < 1 and the
rule's g * 255 lies within 255 * 16 * 2^-24 of an integer (OpenCL's 16-ulp bound for
single-precision pow, the loosest a device powf can be). The library computes the gamma in double
and is expected to need none of it; the count of differing bytes goes to
profiles/temporal/test_figures.txt.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT
from bhrt import abi, configs
import temporal_rule as tr

pytestmark = pytest.mark.gpu
F = np.float32
FIGURES = os.path.join(ROOT, "profiles", "temporal", "test_figures.txt")


def _figure(key, text):
    """One line per key in profiles/temporal/test_figures.txt, rewritten in place."""
    lines = {}
    if os.path.exists(FIGURES):
        for l in open(FIGURES).read().splitlines():
            if ": " in l:
                k, v = l.split(": ", 1)
                lines[k] = v
    lines[key] = text
    os.makedirs(os.path.dirname(FIGURES), exist_ok=True)
    with open(FIGURES, "w") as f:
        f.write("".join(f"{k}: {v}\n" for k, v in sorted(lines.items())))


class _DeviceArray:
    """A float32 device array at a raw address, for torch.as_tensor (zero-copy)."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4",
                                         "data": (int(ptr), False), "version": 2, "strides": None}


def _state_arrays(lib, acc, n):
    """The accumulator's own acc [n][3] and edge [n], read in place (synchronises)."""
    import torch
    rgb_ptr, edge_ptr = lib.accum_device_buffers(acc)
    torch.cuda.synchronize()
    rgb = torch.as_tensor(_DeviceArray(rgb_ptr, (n, 3)), device="cuda").cpu().numpy()
    edge = torch.as_tensor(_DeviceArray(edge_ptr, (n,)), device="cuda").cpu().numpy()
    return rgb, edge


def _outputs(n, edge=True, fill=7):
    import torch
    t = {"rgba8": torch.full((n, 4), fill, dtype=torch.uint8, device="cuda"),
         "rgb": torch.full((n, 3), fill, dtype=torch.float32, device="cuda")}
    if edge:
        t["edge_factor"] = torch.full((n,), fill, dtype=torch.float32, device="cuda")
    return t


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    nan = np.isnan(got) & np.isnan(want)     # (a NaN's payload is not part of the rule)
    bad = np.nonzero((g != w) & ~nan)
    assert bad[0].size == 0, (what, [b[:5] for b in bad], np.asarray(got)[bad][:5],
                              np.asarray(want)[bad][:5])


def _check_bytes(got, want, exempt, what):
    """The display rule of the module docstring; returns (differing bytes, exempt values)."""
    assert (got[:, 3] == 255).all(), what
    d = got[:, :3].astype(np.int32) - want[:, :3].astype(np.int32)
    differ = d != 0
    assert not (differ & ~exempt).any(), (what, np.nonzero(differ & ~exempt)[0][:5])
    assert (np.abs(d) <= 1).all(), what
    return int(differ.sum()), int(exempt.sum())


def _plain_frame(lib, case, offset):
    """bhrt_render_frame_device's rgba32f at a sub-pixel offset: float32 [n][3]."""
    import torch
    bh, dk, cfg, method, flags = tr.scene(case.name)
    cam = configs.camera("B")
    cam.use_offset, cam.offset_x, cam.offset_y = 1, float(offset[0]), float(offset[1])
    t = {"rgba32f": torch.full((case.W * case.H, 4), 7, dtype=torch.float32, device="cuda")}
    torch.cuda.synchronize()
    lib.render_frame_device(bh, dk, cfg, cam, case.W, case.H, None, method, flags,
                            lib.soa_from_tensors(t), None)
    torch.cuda.synchronize()
    got = t["rgba32f"].cpu().numpy()
    assert (got[:, 3] == 1.0).all()
    return got[:, :3].copy()


_plain = {}


def _plain_frames(lib, case):
    """The plain frames of a case's sample set, once per case; never modified."""
    key = (case.name, case.W, case.H, case.jm, case.spp)
    if key not in _plain:
        frames = [_plain_frame(lib, case, o) for o in lib.sample_offsets(tr.case_ss(case))]
        for f in frames:
            f.setflags(write=False)
        _plain[key] = frames
    return _plain[key]


def _run_case(lib, case, schedule=tr.REFERENCE, rows=None, stream=None, frames=None):
    """A case through bhrt_accum_frame_device: per frame (acc, edge, rgba8, edge_factor, rgb)."""
    import torch
    bh, dk, cfg, method, flags = tr.scene(case.name)
    p = tr.case_params(case, schedule)
    acc = lib.accum_create(case.W, case.H, rows, tr.abi_params(p))
    try:
        n = lib.accum_state(acc)["pixels"]
        steps = []
        for _ in range(frames or case.frames):
            t = _outputs(n, edge=rows is None)
            torch.cuda.synchronize()
            lib.accum_frame_device(acc, bh, dk, cfg, configs.camera("B"), method, flags,
                                   tr.case_ss(case), lib.accum_out(t), stream)
            a, e = _state_arrays(lib, acc, n)
            steps.append((a, e, t["rgba8"].cpu().numpy(),
                          t["edge_factor"].cpu().numpy() if rows is None else None,
                          t["rgb"].cpu().numpy()))
        return steps
    finally:
        lib.accum_destroy(acc)


# 1. bit for bit against the rule, on caller frames ----------------------------------------------
SPECIALS = [np.nan, np.inf, -np.inf, -0.25, 1.75, 0.0, 1.0, 1e-40, -1e-42, -0.0]
PARAM_SETS = {"reference": tr.params(), "mean": tr.params(tr.MEAN),
              "reference-0.25": tr.params(blend_factor=0.25, edge_decay=0.3, edge_threshold=0.05)}
SIZES = [(1, 1), (3, 3), (64, 1), (67, 5), (2, 130), (257, 3)]


def caller_frames(W, H, seed):
    """12 seeded float32 frames [n][3]: steps 1 to 7 random in [-0.1, 1.1) with NaN, +-inf,
    negatives, values above 1, exact 0 and 1 and denormals planted in them; after the reset the
    frames are flat (one colour each), so the edge factors only decay."""
    rng = np.random.default_rng(seed)
    n = W * H
    frames = []
    for k in range(12):
        if k >= 7:
            frames.append(np.tile(rng.random(3, dtype=np.float32), (n, 1)))
            continue
        f = (rng.random((n, 3), dtype=np.float32) * F(1.2) - F(0.1)).astype(np.float32)
        flat = f.reshape(-1)
        where = rng.choice(flat.size, size=min(flat.size, len(SPECIALS)), replace=False)
        for j, i in enumerate(where):
            flat[i] = F(SPECIALS[(j + k) % len(SPECIALS)])
        frames.append(f)
    return frames


@pytest.mark.parametrize("pname", list(PARAM_SETS))
def test_caller_frames_bit_for_bit_against_the_rule(bhrt_lib, pname):
    """12 steps with a reset after step 7 at every image size: acc, the rgb copy and edge_factor
    bit for bit at every step, rgba8 under the display rule; the exempt share is taken over the
    channel values of all sizes (a 1 x 1 image has 36 of them)."""
    import torch
    p = PARAM_SETS[pname]
    differing = exempt_total = values = walks = 0
    for W, H in SIZES:
        n = W * H
        rule = tr.Accumulator(W, H, p)
        acc = bhrt_lib.accum_create(W, H, None, tr.abi_params(p))
        walk = []
        try:
            for k, f in enumerate(caller_frames(W, H, seed=1000 * W + H)):
                what = f"{W}x{H} step {k + 1}"
                if k == 7:
                    bhrt_lib.accum_reset(acc)
                    rule.reset()
                want8, exempt = rule.step(f)
                d_f = torch.from_numpy(f).cuda()
                t = _outputs(n)
                torch.cuda.synchronize()
                bhrt_lib.accum_blend_device(acc, d_f.data_ptr(), bhrt_lib.accum_out(t), None)
                a, e = _state_arrays(bhrt_lib, acc, n)
                _same_bits(a, rule.acc, f"acc, {what}")
                _same_bits(t["rgb"].cpu().numpy(), rule.acc, f"rgb copy, {what}")
                _same_bits(e, rule.edge, f"edge, {what}")
                _same_bits(t["edge_factor"].cpu().numpy(), rule.edge, f"edge_factor, {what}")
                dif, ex = _check_bytes(t["rgba8"].cpu().numpy(), want8, exempt, f"rgba8, {what}")
                differing += dif
                exempt_total += ex
                values += exempt.size
                walk.append(rule.edge.copy())
                if k < 7:
                    assert np.isnan(rule.acc).any() or n < 4     # the specials are in play
            assert not np.isnan(rule.acc).any()                  # the reset cleared them
        finally:
            bhrt_lib.accum_destroy(acc)
        # the pixels at 1.0 before the reset walk down by the decay: 1.0 -> 0.8 -> 0.6 -> ... -> 0
        at_one = walk[6] == 1
        assert at_one.any() or (W - 2) * (H - 2) < 100
        if at_one.any():
            e, seq = F(1), []
            for _ in range(5):
                dec = e - p.edge_decay
                e = dec if F(0) < dec else F(0)
                seq.append(e)
            for j in range(5):
                assert (walk[7 + j][at_one] == seq[j]).all(), (W, H, j, seq)
            assert seq[0] == F(1) - p.edge_decay and seq[-1] < 1e-6
            walks += 1
    print(f"{pname}: {differing} differing bytes, {exempt_total} exempt of {values} values")
    assert walks >= 2
    assert exempt_total <= tr.EXEMPT_SHARE * values
    _figure(f"caller frames {pname}",
            f"{differing} differing bytes, {exempt_total} exempt of {values} channel values")


# 2. bit for bit against the rule, on libbhrt's own plain frames -----------------------------------
@pytest.mark.parametrize("case", tr.CASES, ids=tr.CASE_IDS)
def test_own_frames_bit_for_bit_against_the_rule(bhrt_lib, case):
    plain = _plain_frames(bhrt_lib, case)
    assert len(plain) == case.spp
    rule = tr.Accumulator(case.W, case.H, tr.case_params(case))
    got = _run_case(bhrt_lib, case)
    differing = exempt_total = values = 0
    for k, (a, e, rgba8, edge_factor, rgb) in enumerate(got):
        want8, exempt = rule.step(plain[k % case.spp], case.spp)
        _same_bits(a, rule.acc, f"acc, frame {k + 1}")
        _same_bits(rgb, rule.acc, f"rgb copy, frame {k + 1}")
        _same_bits(e, rule.edge, f"edge, frame {k + 1}")
        _same_bits(edge_factor, rule.edge, f"edge_factor, frame {k + 1}")
        dif, ex = _check_bytes(rgba8, want8, exempt, f"rgba8, frame {k + 1}")
        differing += dif
        exempt_total += ex
        values += exempt.size
    ones = int((rule.edge == 1).sum())
    nan_px = np.isnan(rule.acc).any(axis=1)
    print(f"{case}: {differing} differing bytes, {exempt_total} exempt of {values} values, {ones} "
          f"edge pixels at 1.0, {int(nan_px.sum())} NaN pixels")
    assert exempt_total <= tr.EXEMPT_SHARE * values and ones > 0
    if case.name == "kerr099":     # the NaN pixels stay NaN and read 255
        assert nan_px.any() and (got[-1][2][:, :3][np.isnan(rule.acc)] == 255).all()
    _figure(f"own frames {tr.CASE_IDS[tr.CASES.index(case)]}",
            f"{differing} differing bytes, {exempt_total} exempt of {values} channel values")


# 3. against the oracle ------------------------------------------------------------------------
@pytest.mark.parametrize("case", tr.CASES, ids=tr.CASE_IDS)
def test_frames_vs_oracle(bhrt_lib, oracle, case):
    """acc against the rule run over the oracle's frames: per value (1e-5 + (3K + 1) 2^-24) m, K
    the number of frames and m that pixel-channel's largest oracle colour over the frames -- the
    1e-5 colour contract carried through a convex combination of non-negative colours, three
    roundings per blend and one for the (float) conversion. The NaN pattern is identical."""
    want, margin_min = tr.oracle_run(oracle, case)
    frames, _ = tr.oracle_frames(oracle, case)
    K = case.frames
    got = _run_case(bhrt_lib, case)
    worst = 0.0
    for k in range(K):
        # (checked after every frame: m over the frames blended so far -- a pixel that a later
        # sample turns NaN has a colour until then)
        with np.errstate(invalid="ignore"):
            m = np.max(np.stack([frames[j % case.spp] for j in range(k + 1)]), axis=0)
        bound = (1e-5 + (3 * K + 1) * 2.0 ** -24) * m
        a, w = got[k][0].astype(np.float64), want[k][0].astype(np.float64)
        assert np.array_equal(np.isnan(a), np.isnan(w)), f"NaN pattern, frame {k + 1}"
        ok = ~np.isnan(w)
        err = np.abs(a - w)
        assert (err[ok] <= bound[ok]).all(), (k + 1, float(np.max(err[ok] - bound[ok])))
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(m > 0, err / m, 0.0)
        worst = max(worst, float(np.nanmax(rel)))
    print(f"{case}: oracle min margin {margin_min:.2e}, max err / m {worst:.2e} "
          f"(bound {1e-5 + (3 * K + 1) * 2.0 ** -24:.2e})")


# 4. shards ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,row_block,shards", tr.SHARD_CASES,
                         ids=[f"{c.name}-{c.W}x{c.H}-block{rb}-of{s}" for c, rb, s in tr.SHARD_CASES])
def test_shard_accumulators_equal_the_whole_image(bhrt_lib, case, row_block, shards):
    import adaptive_rule as ar
    whole = _run_case(bhrt_lib, case)[-1]
    sizes = []
    for s in range(shards):
        rows = abi.Rows(row_block, s, shards)
        image_rows = ar.shard_image_rows(case.H, row_block, s, shards)
        sizes.append(len(image_rows))
        shard = _run_case(bhrt_lib, case, rows=rows)[-1]
        pick = np.concatenate([np.arange(y * case.W, (y + 1) * case.W) for y in image_rows])
        assert shard[0].shape == (pick.size, 3)
        _same_bits(shard[0], whole[0][pick], f"acc of shard {s}")
        assert np.array_equal(shard[2], whole[2][pick]), f"rgba8 of shard {s}"
    if case.W == 40:
        assert sizes == [16, 16, 8]


def test_edge_factor_of_a_shard_is_refused(bhrt_lib):
    import torch
    case = tr.SHARD_CASES[1][0]
    bh, dk, cfg, method, flags = tr.scene(case.name)
    acc = bhrt_lib.accum_create(case.W, case.H, abi.Rows(3, 0, 2), None)
    try:
        n = bhrt_lib.accum_state(acc)["pixels"]
        t = _outputs(n, edge=True)
        torch.cuda.synchronize()
        before = bhrt_lib.accum_state(acc)
        with pytest.raises(bhrt_lib.BhrtError, match="edge_factor"):
            bhrt_lib.accum_frame_device(acc, bh, dk, cfg, configs.camera("B"), method, flags,
                                        tr.case_ss(case), bhrt_lib.accum_out(t), None)
        d_f = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        with pytest.raises(bhrt_lib.BhrtError, match="edge_factor"):
            bhrt_lib.accum_blend_device(acc, d_f.data_ptr(), bhrt_lib.accum_out(t), None)
        torch.cuda.synchronize()
        assert all((v.cpu().numpy() == 7).all() for v in t.values())
        assert bhrt_lib.accum_state(acc) == before and before["sharded"] == 1
    finally:
        bhrt_lib.accum_destroy(acc)


# 5. state ---------------------------------------------------------------------------------------
def test_state_stats_and_host_form(bhrt_lib):
    import torch
    case = tr.CASES[1]      # C2 23x7, grid 4
    bh, dk, cfg, method, flags = tr.scene(case.name)
    p = tr.case_params(case)
    ss = tr.case_ss(case)
    offsets = bhrt_lib.sample_offsets(ss)
    n = case.W * case.H
    rule = tr.Accumulator(case.W, case.H, p)
    dev = bhrt_lib.accum_create(case.W, case.H, None, tr.abi_params(p))
    host = bhrt_lib.accum_create(case.W, case.H, None, tr.abi_params(p))
    try:
        for k in range(7):
            if k == 5:      # what the viewer does on a camera move
                bhrt_lib.accum_reset(dev)
                bhrt_lib.accum_reset(host)
                rule.reset()
                assert bhrt_lib.accum_state(dev, ss)["reset_pending"] == 1
            st = bhrt_lib.accum_state(dev, ss)
            assert (st["frame_count"], st["jitter_index"], st["frames_total"], st["pixels"]) == \
                (rule.frame_count, rule.jitter_index, rule.frames_total, n)
            assert F(st["next_alpha"]) == rule.next_alpha() and st["cycle"] == case.spp
            assert (st["next_offset_x"], st["next_offset_y"]) == tuple(offsets[rule.jitter_index])
            if k == 5:      # after a reset the next alpha is 1.0 and jitter_index continues
                assert st["next_alpha"] == 1.0 and st["jitter_index"] == 5 % case.spp
            t = _outputs(n)
            torch.cuda.synchronize()
            bhrt_lib.stats(reset=True)
            bhrt_lib.accum_frame_device(dev, bh, dk, cfg, configs.camera("B"), method, flags, ss,
                                        bhrt_lib.accum_out(t), None)
            torch.cuda.synchronize()
            stats = bhrt_lib.stats(reset=True)
            assert stats["rays"] == n and stats["launches"] == 1, stats
            rule.step(np.zeros((n, 3), dtype=np.float32), case.spp)   # (the counters alone)
            h = bhrt_lib.accum_frame(host, bh, dk, cfg, configs.camera("B"), method, flags, ss)
            assert bhrt_lib.accum_state(host, ss) == bhrt_lib.accum_state(dev, ss)
            _same_bits(h["rgb"], t["rgb"].cpu().numpy(), f"host rgb, frame {k + 1}")
            _same_bits(h["edge_factor"], t["edge_factor"].cpu().numpy(), f"host edge, frame {k + 1}")
            assert np.array_equal(h["rgba8"], t["rgba8"].cpu().numpy())
        st = bhrt_lib.accum_state(dev, ss)
        assert (st["frame_count"], st["jitter_index"], st["frames_total"]) == (2, 7 % case.spp, 7)
    finally:
        bhrt_lib.accum_destroy(dev)
        bhrt_lib.accum_destroy(host)


# 6. asynchrony ----------------------------------------------------------------------------------
def test_two_accumulators_on_two_streams_from_one_thread(bhrt_lib):
    """Frames issued alternately on two streams with no synchronise in between give the bits of
    the serial runs."""
    import torch
    cases = (tr.CASES[0], tr.CASES[3])
    serial = [_run_case(bhrt_lib, c, frames=6) for c in cases]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    accs, outs = [], [[], []]
    try:
        for c in cases:
            accs.append(bhrt_lib.accum_create(c.W, c.H, None, tr.abi_params(tr.case_params(c))))
        for i, c in enumerate(cases):
            outs[i] = [_outputs(c.W * c.H) for _ in range(6)]
        torch.cuda.synchronize()
        for k in range(6):
            for i, c in enumerate(cases):
                bh, dk, cfg, method, flags = tr.scene(c.name)
                bhrt_lib.accum_frame_device(accs[i], bh, dk, cfg, configs.camera("B"), method,
                                            flags, tr.case_ss(c), bhrt_lib.accum_out(outs[i][k]),
                                            streams[i].cuda_stream)
        torch.cuda.synchronize()
        for i, c in enumerate(cases):
            for k in range(6):
                _same_bits(outs[i][k]["rgb"].cpu().numpy(), serial[i][k][4], f"{c.name} frame {k + 1}")
                _same_bits(outs[i][k]["edge_factor"].cpu().numpy(), serial[i][k][3], c.name)
                assert np.array_equal(outs[i][k]["rgba8"].cpu().numpy(), serial[i][k][2])
            a, e = _state_arrays(bhrt_lib, accs[i], c.W * c.H)
            _same_bits(a, serial[i][5][0], f"{c.name} acc")
            _same_bits(e, serial[i][5][1], f"{c.name} edge")
    finally:
        for a in accs:
            bhrt_lib.accum_destroy(a)


def test_null_stream_orders_after_default_stream_fills(bhrt_lib):
    """Outputs poison-filled on the default stream behind a busy kernel, no sync before the
    NULL-stream calls, read back on the default stream: the frames, not the fill."""
    import torch
    assert torch.cuda.current_stream().cuda_stream == 0
    case = tr.CASES[0]
    want = _run_case(bhrt_lib, case, frames=2)
    bh, dk, cfg, method, flags = tr.scene(case.name)
    acc = bhrt_lib.accum_create(case.W, case.H, None, tr.abi_params(tr.case_params(case)))
    try:
        t = [_outputs(case.W * case.H, fill=0) for _ in range(2)]
        torch.cuda.synchronize()  # (allocation done; everything below stays queued)
        sleep = getattr(torch.cuda, "_sleep", None)
        if sleep is not None:
            sleep(20_000_000)
        else:
            m = torch.ones(2048, 2048, device="cuda")
            for _ in range(8):
                m = m @ m * 1e-3
        for k in range(2):
            for v in t[k].values():
                v.fill_(3)
            bhrt_lib.accum_frame_device(acc, bh, dk, cfg, configs.camera("B"), method, flags,
                                        tr.case_ss(case), bhrt_lib.accum_out(t[k]), None)
        for k in range(2):
            _same_bits(t[k]["rgb"].cpu().numpy(), want[k][4], f"rgb, frame {k + 1}")
            _same_bits(t[k]["edge_factor"].cpu().numpy(), want[k][3], f"edge, frame {k + 1}")
            assert np.array_equal(t[k]["rgba8"].cpu().numpy(), want[k][2])
    finally:
        bhrt_lib.accum_destroy(acc)


# 7. convergence ---------------------------------------------------------------------------------
def test_mean_schedule_converges_to_the_sample_mean(bhrt_lib):
    """BHRT_ACCUM_MEAN over the 4 samples of a 2x2 grid: acc against the sequential float64 mean
    of the four plain frames, per value (3 * 4 + 1) 2^-24 m -- three roundings per blend, one for
    the mean's own conversion -- with m the pixel-channel's largest colour over the frames."""
    case = tr.Case("C2", 40, 24, tr.GRID, 4, 4, 0.1)
    plain = [f.astype(np.float64) for f in _plain_frames(bhrt_lib, case)]
    acc = plain[0]
    for f in plain[1:]:
        acc = acc + f
    mean = acc / 4.0
    m = np.max(np.stack(plain), axis=0)
    got = _run_case(bhrt_lib, case, schedule=tr.MEAN)[-1][0].astype(np.float64)
    err = np.abs(got - mean)
    bound = (3 * 4 + 1) * 2.0 ** -24 * m
    assert not np.isnan(got).any()
    print(f"mean of 4: max err {err.max():.3e}, worst err / bound "
          f"{np.max(np.where(bound > 0, err / np.maximum(bound, 1e-300), 0)):.3f}")
    assert (err <= bound).all(), float(np.max(err - bound))
    # and it is not just the first frame
    assert np.abs(got - plain[0]).max() > 1e-3


# 8. refusals --------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["use_offset", "random", "65 samples", "blackhole NULL",
                                  "out NULL"])
def test_bad_frame_arguments_are_refused_and_write_nothing(bhrt_lib, what):
    import torch
    L = bhrt_lib.load()
    case = tr.CASES[1]
    bh, dk, cfg, method, flags = tr.scene(case.name)
    cam = configs.camera("B")
    ss = tr.case_ss(case)
    n = case.W * case.H
    acc = bhrt_lib.accum_create(case.W, case.H, None, None)
    try:
        t = _outputs(n)
        out = bhrt_lib.accum_out(t)
        p_bh, p_out = C.byref(bh), C.byref(out)
        if what == "use_offset":
            cam.use_offset, cam.offset_x, cam.offset_y = 1, 0.25, 0.25
        elif what == "random":
            ss = abi.SupersamplingParams(4, abi.JITTER_RANDOM, 1.0)
        elif what == "65 samples":
            ss = abi.SupersamplingParams(65, tr.HALTON, 1.0)
        elif what == "blackhole NULL":
            p_bh = None
        elif what == "out NULL":
            p_out = None
        torch.cuda.synchronize()
        before = bhrt_lib.accum_state(acc)
        assert L.bhrt_accum_frame_device(acc, p_bh, C.byref(dk), C.byref(cfg), C.byref(cam), method,
                                         flags, C.byref(ss), p_out, None) == -1
        assert bhrt_lib.last_error()
        host = abi.AccumOut()
        if what != "out NULL":
            sentinel = np.full((n, 4), 7, dtype=np.uint8)
            host = abi.AccumOut(rgba8=sentinel.ctypes.data)
        assert L.bhrt_accum_frame(acc, p_bh, C.byref(dk), C.byref(cfg), C.byref(cam), method, flags,
                                  C.byref(ss), C.byref(host) if what != "out NULL" else None) == -1
        torch.cuda.synchronize()
        assert all((v.cpu().numpy() == 7).all() for v in t.values())
        assert what == "out NULL" or (sentinel == 7).all()
        assert bhrt_lib.accum_state(acc) == before
        a, e = _state_arrays(bhrt_lib, acc, n)
        assert (a == 0).all() and (e == 0).all()
    finally:
        bhrt_lib.accum_destroy(acc)
