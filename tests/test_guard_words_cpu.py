"""CPU check of the rule behind the trace loop's high-word guard (bhrt_trace_core.h all_below_2,
restated in guard_words_rule.py): on fixed special operands and seeded random ones the filter
says "straight-line path" exactly for the triples whose members are all finite and below 2 in
magnitude, so it never passes a triple the exact test (every |x| <= 10) fails."""
import numpy as np

import guard_words_rule as gw


def _random_bit_patterns(count, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 64, (count, 3), dtype=np.uint64).view(np.float64)


def _near_thresholds(count, seed):
    """Triples whose members lie in the high word of a threshold or a neighbouring one."""
    rng = np.random.default_rng(seed)
    c = rng.choice(gw.THRESHOLDS, (count, 3))
    hi = gw.hiword(c).astype(np.int64) + rng.integers(-1, 2, (count, 3))
    lo = rng.integers(0, 2 ** 32, (count, 3))
    sign = rng.integers(0, 2, (count, 3)) << 63
    return ((hi << 32) | lo | sign).astype(np.uint64).view(np.float64)


def test_filter_is_below_2_and_implies_exact():
    cases = {
        "special": gw.special_triples(),
        "random magnitudes": gw.random_triples(1 << 18),
        "non-finite": gw.nonfinite_triples(),
        "random bit patterns": _random_bit_patterns(1 << 19, 41),
        "near thresholds": _near_thresholds(1 << 18, 43),
    }
    total = 0
    for what, t in cases.items():
        f, e, b = gw.filter_words(t), gw.exact_test(t), gw.below_2(t)
        assert np.array_equal(f, b), (what, t[f != b][:5])
        assert not (f & ~e).any(), (what, t[f & ~e][:5])
        total += len(t)
    assert total >= 1_000_000
    # the filter is no constant: the operand sets hold triples of every kind
    t = np.concatenate([cases["special"], cases["random magnitudes"]])
    f, e = gw.filter_words(t), gw.exact_test(t)
    assert f.any() and (~f & e).any() and (~e).any()


def test_special_values_are_what_they_say():
    s = gw.special_values()
    assert np.isnan(s).sum() == 2 and np.isinf(s).sum() == 2
    assert np.signbit(s[np.isnan(s)]).tolist() == [False, True]
    for c in gw.THRESHOLDS:
        assert (s == c).sum() == 1 and (s == -c).sum() == 1
        assert (s == np.nextafter(c, 0.0)).sum() == 1 and (s == np.nextafter(c, np.inf)).sum() == 1
        hi = int(gw.hiword(c))
        first_next = s[(gw.hiword(s) == hi + 1) & (s.view(np.uint64) & np.uint64(0xFFFFFFFF) == 0)]
        assert first_next.size == 1 and first_next[0] > c
    assert (s == 5e-324).any() and (s == 2.0 ** 1017).any() and (s == -(2.0 ** -1017)).any()
