"""Exact float64 sums (fdb_plan_set_exact_sums), host side: fdb_selftest_exact_sum runs the digit split, normalize and rounding code the
device kernels run (fdb_kernels.h) and must give the correctly rounded exact sum — the bits of float(sum(Fraction(v))) — on every input.
No device is touched."""
import math
import random
import struct
from fractions import Fraction

import pytest


@pytest.fixture(scope="module")
def pp():
    from frostdb_amd import build
    build.build()
    from frostdb_amd import physicalplan
    return physicalplan


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def reference(xs):
    """IEEE semantics for the non-finite inputs, else the exact rational sum rounded once (Python rounds half to even)."""
    if any(math.isnan(x) for x in xs) or (math.inf in xs and -math.inf in xs):
        return math.nan
    if math.inf in xs:
        return math.inf
    if -math.inf in xs:
        return -math.inf
    s = sum((Fraction(x) for x in xs), Fraction(0))
    try:
        return float(s) + 0.0  # (+ 0.0: a zero sum is +0.0)
    except OverflowError:
        return math.inf if s > 0 else -math.inf


def check(pp, xs):
    got, want = pp.selftest_exact_sum(xs), reference(xs)
    if math.isnan(want):
        assert math.isnan(got), xs
    else:
        assert bits(got) == bits(want), (xs[:8], got, want)


def test_subnormals_alone_and_with_normals(pp):
    tiny = 5e-324
    check(pp, [tiny] * 7)
    check(pp, [tiny, -tiny * 3, 2.2250738585072009e-308, 2.2250738585072014e-308])
    check(pp, [2.2250738585072014e-308, -tiny])               # the smallest normal minus the smallest subnormal: a subnormal
    check(pp, [1.0, tiny, -1.0])
    rng = random.Random(7)
    check(pp, [rng.choice([-1, 1]) * rng.randint(1, 2**52) * tiny for _ in range(500)] + [1e-300, -3e-310])


def test_huge_values_cancel_exactly(pp):
    check(pp, [1e308, 1e308, -1e308, -1e308, 5e-324])
    assert pp.selftest_exact_sum([1e308, 1e308, -1e308, -1e308, 5e-324]) == 5e-324


def test_ties_to_even_and_the_sticky_bit(pp):
    assert pp.selftest_exact_sum([2.0**53, 1.0]) == 2.0**53                 # a tie: to even
    assert pp.selftest_exact_sum([2.0**53, 1.0, 2.0**-60]) == 2.0**53 + 2    # just above the tie: up
    assert pp.selftest_exact_sum([2.0**53, 3.0]) == 2.0**53 + 4             # a tie whose lower neighbour is odd: up
    assert pp.selftest_exact_sum([-(2.0**53), -1.0, -(2.0**-60)]) == -(2.0**53 + 2)
    check(pp, [1.0, 2.0**-53])
    check(pp, [1.0, 2.0**-53, 2.0**-1074])


def test_heavy_cancellation(pp):
    rng = random.Random(2026)
    xs = []
    for _ in range(300):
        x = rng.choice([-1, 1]) * rng.random() * 2.0 ** rng.randint(-1074, 1000)
        xs += [x, -x * (1 + 2.0**-40)]
    rng.shuffle(xs)
    assert len(xs) == 600
    check(pp, xs)
    for seed in range(200):
        r = random.Random(seed)
        ys = [r.choice([-1, 1]) * r.random() * 2.0 ** r.randint(-1074, 1023) for _ in range(r.randint(1, 60))]
        ys += [-y for y in ys[: len(ys) // 2]]
        check(pp, ys)


def test_beyond_dbl_max_rounds_to_infinity(pp):
    assert pp.selftest_exact_sum([1.7976931348623157e308, 1.7976931348623157e308]) == math.inf
    assert pp.selftest_exact_sum([-1.7976931348623157e308] * 3) == -math.inf
    assert pp.selftest_exact_sum([1.7976931348623157e308, 1.7976931348623157e308, -1.7976931348623157e308]) == 1.7976931348623157e308
    check(pp, [1.7976931348623157e308, 2.0**970])   # rounds up past DBL_MAX (half an ulp there is 2^970)
    check(pp, [1.7976931348623157e308, 2.0**969])


def test_nan_and_infinities(pp):
    inf = math.inf
    assert math.isnan(pp.selftest_exact_sum([1.0, math.nan]))
    assert math.isnan(pp.selftest_exact_sum([inf, -inf]))
    assert math.isnan(pp.selftest_exact_sum([inf, math.nan]))
    assert pp.selftest_exact_sum([inf, 1.0, 1e308, 1e308]) == inf
    assert pp.selftest_exact_sum([-inf, -1e308, 1.0]) == -inf
    assert pp.selftest_exact_sum([inf, inf]) == inf


def test_negative_zeros_give_positive_zero(pp):
    for xs in ([-0.0], [-0.0, -0.0, -0.0], [], [1.5, -1.5], [-0.0, 5e-324, -5e-324]):
        r = pp.selftest_exact_sum(xs)
        assert r == 0.0 and bits(r) == 0, xs


def test_permutations_give_identical_bits(pp):
    rng = random.Random(99)
    xs = [1e308, -1e308, 2.0**53, 1.0, 2.0**-60, 5e-324, -3.0, 1e-300, 123456.789, -1e16, 1e16, 0.1, 0.2, 0.3, -0.6]
    want = bits(reference(xs))
    assert bits(pp.selftest_exact_sum(xs)) == want
    for _ in range(100_000):
        rng.shuffle(xs)
        assert bits(pp.selftest_exact_sum(xs)) == want


def test_invalid_arguments(pp):
    import ctypes
    out = ctypes.c_double()
    assert pp.lib().fdb_selftest_exact_sum(None, 3, ctypes.byref(out)) == pp.FDB_ERR_INVALID
    assert pp.lib().fdb_selftest_exact_sum(None, -1, ctypes.byref(out)) == pp.FDB_ERR_INVALID
