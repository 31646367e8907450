"""The LK kernels test a level's minimum eigenvalue without dividing: upstream's

    minEig = num / (2 * win * win) < 0.001f          (num = A22 + A11 - sqrt(...), win = 21: the divisor is 882)

is taken as  num < T  with one float T (csrc/lk_common.h, kMinEigNumBelow).  Correctly rounded division by a positive
constant is monotone, so such a T exists; this file finds it by bisection over the float32 bit patterns (numpy's float32
division is IEEE, correctly rounded), checks the equivalence around T, at the special values and over random floats, and
checks that the constant in the source is that float.  No GPU."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LK_COMMON = os.path.join(ROOT, "stereo-visual-odometry_amd", "csrc", "lk_common.h")
DIVISOR = np.float32(2 * 21 * 21)
BOUND = np.float32(0.001)


def _floats(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _bits(x):
    return int(np.asarray([x], dtype=np.float32).view(np.uint32)[0])


def _quotient_below(x):
    """fl(x / 882.f) < 0.001f, elementwise, in float32."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        q = x / DIVISOR
    assert q.dtype == np.float32
    return q < BOUND


def _threshold_bits():
    """The smallest non-negative float32 bit pattern whose quotient is NOT below the bound (patterns of non-negative floats
    order like the floats themselves)."""
    lo, hi = 0, 0x7F800000                      # 0.0: below; +inf: not below
    assert _quotient_below(_floats([lo]))[0] and not _quotient_below(_floats([hi]))[0]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _quotient_below(_floats([mid]))[0]:
            lo = mid
        else:
            hi = mid
    return hi


T_BITS = _threshold_bits()
T = _floats([T_BITS])[0]


def _assert_equivalent(x):
    x = np.asarray(x, dtype=np.float32)
    want = _quotient_below(x)
    with np.errstate(invalid="ignore"):
        got = x < T
    bad = np.flatnonzero(want != got)
    assert bad.size == 0, [(float(x[i]), hex(_bits(x[i]))) for i in bad[:8]]


def test_threshold_is_where_the_quotient_reaches_the_bound():
    assert T_BITS == 0x3F61CAC1
    below, at = _floats([T_BITS - 1, T_BITS]) / DIVISOR
    assert below < BOUND <= at


def test_every_float_within_4096_ulps_of_the_threshold():
    _assert_equivalent(_floats(np.arange(T_BITS - 4096, T_BITS + 4097, dtype=np.uint32)))


def test_special_values():
    tiny = _floats([1, 2, 0x007FFFFF])                                  # denormals
    x = np.concatenate([np.float32([0.0, -0.0]), tiny, -tiny,
                        np.float32([-1e-30, -0.882, -1.0, -882.0, -3e38, -np.inf]),
                        _floats([0x00800000, 0x7F7FFFFF]),              # smallest normal, largest finite
                        np.float32([np.inf, np.nan]), _floats([0xFFC00000, 0x7FA00000])])
    _assert_equivalent(x)
    # both forms are false for a NaN and for +inf, true for every negative value
    assert not _quotient_below(np.float32([np.nan, np.inf])).any()
    with np.errstate(invalid="ignore"):
        assert not (np.float32([np.nan, np.inf]) < T).any()
    assert _quotient_below(np.float32([-np.inf, -1.0, -0.0])).all()


def test_a_million_random_positive_floats():
    rng = np.random.default_rng(882)
    # random bit patterns of positive finite floats: every exponent, so both sides of T and the far ends are covered ...
    _assert_equivalent(_floats(rng.integers(1, 0x7F800000, 500_000, dtype=np.uint32)))
    # ... and values at the scale of the test itself
    _assert_equivalent(rng.uniform(0.0, 4.0, 500_000).astype(np.float32))


def test_the_source_constant_is_the_threshold():
    src = open(LK_COMMON).read()
    m = re.search(r"constexpr\s+float\s+kMinEigNumBelow\s*=\s*([^;]+);", src)
    assert m, "kMinEigNumBelow not found in lk_common.h"
    lit = m.group(1).strip()
    assert lit.endswith("f"), lit
    value = float.fromhex(lit[:-1]) if lit.lower().startswith("0x") else float(lit[:-1])
    assert np.float32(value) == value, "the literal is not a float32 value"
    assert _bits(np.float32(value)) == T_BITS, (lit, hex(T_BITS))
    # and the comparison in the source is against the numerator, not the quotient
    assert re.search(r"mask_lt\(\s*minEigNum\s*,\s*kMinEigNumBelow\s*\)", src)
