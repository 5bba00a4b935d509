"""The high-word filter of the trace loop's plain-value test (bhrt_trace_core.h all_below_2), restated
in numpy for the CPU and GPU tests, and the operands both run it on.

The filter ORs the high 32 bits of three doubles and reads the result as a float: its magnitude
is below 2.0f exactly when bit 30 is clear, which is exactly when all three doubles are finite
and below 2 in magnitude. The exact test it filters for is "every |x| <= 10" (NaN fails)."""
import numpy as np

THRESHOLDS = (2.0, 10.0)  # the filter's own bound and the exact test's


def hiword(x):
    return (np.asarray(x, dtype=np.float64).view(np.uint64) >> np.uint64(32)).astype(np.uint32)


def filter_words(t):
    """all_below_2 on triples t[n, 3], as the kernel forms it: the OR of the three high words read
    as a float, |.| < 2.0f (an ordered compare: a NaN pattern fails)."""
    w = hiword(t[:, 0]) | hiword(t[:, 1]) | hiword(t[:, 2])
    with np.errstate(invalid="ignore"):
        return np.abs(w.view(np.float32)) < np.float32(2.0)


def exact_test(t):
    with np.errstate(invalid="ignore"):
        return (np.abs(t) <= 10.0).all(axis=1)


def below_2(t):
    """What the filter is meant to say: all three finite and below 2 in magnitude."""
    with np.errstate(invalid="ignore"):
        return (np.abs(t) < 2.0).all(axis=1)


def _from_bits(hi, lo=0):
    return np.array([(int(hi) << 32) | int(lo)], dtype=np.uint64).view(np.float64)[0]


def special_values():
    """Each threshold with its two neighbours and the first double of the next and of the
    previous high word, both signs; +-0, the smallest and largest denormal, +-Inf, NaN of both
    signs, +-2^1017, +-2^-1017."""
    v = []
    for c in THRESHOLDS:
        hi = int(hiword(c))
        v += [c, np.nextafter(c, 0.0), np.nextafter(c, np.inf), _from_bits(hi + 1),
              _from_bits(hi - 1)]
    v += [0.0, 5e-324, _from_bits(0x000FFFFF, 0xFFFFFFFF), np.inf, 2.0 ** 1017, 2.0 ** -1017]
    v = np.array(v, dtype=np.float64)
    nan_pos = _from_bits(0x7FF80000)
    nan_neg = _from_bits(0xFFF80000, 1)
    return np.concatenate([v, -v, [nan_pos, nan_neg]])


def special_triples():
    """Every special value in each of the three positions, beside two benign values (0.5, -1.25),
    and every pair of special values beside one benign value."""
    s = special_values()
    rows = []
    for pos in range(3):
        t = np.tile(np.array([0.5, -1.25, 0.5]), (len(s), 1))
        t[:, pos] = s
        rows.append(t)
    a, b = np.meshgrid(s, s, indexing="ij")
    rows.append(np.stack([a.ravel(), b.ravel(), np.full(a.size, 0.5)], axis=1))
    return np.concatenate(rows)


def random_triples(count=4096, seed=31):
    """Magnitudes log-uniform over [1e-8, 30] with random signs."""
    rng = np.random.default_rng(seed)
    m = 10.0 ** rng.uniform(-8.0, np.log10(30.0), (count, 3))
    return m * rng.choice([-1.0, 1.0], (count, 3))


def nonfinite_triples(seed=37):
    """NaN, +Inf and -Inf in each position of random triples that are otherwise below 2."""
    rng = np.random.default_rng(seed)
    rows = []
    for bad in (np.nan, np.inf, -np.inf):
        for pos in range(3):
            t = rng.uniform(-1.9, 1.9, (8, 3))
            t[:, pos] = bad
            rows.append(t)
    return np.concatenate(rows)
