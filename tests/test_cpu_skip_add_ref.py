"""tests/skip_add_ref.py against exact rational arithmetic: fma32 is the correctly rounded fp32 fma -- on random draws and on constructed cases where
rounding the fp64 sum to nearest first lands on the wrong side --, and skip_add_expected is the chain of such fmas with one rounding to f16."""
from fractions import Fraction

import numpy as np

from skip_add_ref import fma32, skip_add_expected


def _round(x: Fraction, bits: int, emin: int) -> float:
    """x rounded to nearest even in a binary format of `bits` significand bits and least normal exponent emin (no overflow here)"""
    if x == 0:
        return 0.0
    e = max((abs(x).numerator.bit_length() - abs(x).denominator.bit_length()), emin)
    if Fraction(2) ** e > abs(x) and e > emin:
        e -= 1
    elif Fraction(2) ** (e + 1) <= abs(x):
        e += 1
    q = Fraction(2) ** (e - (bits - 1))
    return float(round(x / q) * q)      # (round() of a Fraction rounds halves to even)


def _fma_exact(s, a, v) -> np.float32:
    return np.float32(_round(Fraction(float(s)) * Fraction(float(a)) + Fraction(float(v)), 24, -126))


def _midpoint_cases():
    """s a = 2^-24 (1 - k^2 2^-40) lies just under half a unit of v = 1 + odd 2^-23: the exact sum rounds down to v, while fp64 cannot hold
    the k^2 2^-64 for small k, rounds the sum to the midpoint, and the cast's tie goes up to the even neighbour"""
    k = np.arange(1, 2001, dtype=np.float64)
    s = (2.0 ** -12 * (1 + k * 2.0 ** -20)).astype(np.float32)
    a = (2.0 ** -12 * (1 - k * 2.0 ** -20)).astype(np.float32)
    v = (1 + (2 * ((k * 7919) % 4000000) + 1) * 2.0 ** -23).astype(np.float32)
    return s, a, v


def test_fma32_is_correctly_rounded_on_random_draws():
    rng = np.random.default_rng(0)
    n = 4000
    s, a, v = [(rng.standard_normal(n) * np.exp2(rng.integers(-6, 7, n))).astype(np.float32) for _ in range(3)]
    v[::5] = (-s[::5].astype(np.float64) * a[::5]).astype(np.float32)      # cancellation: the result is the product's own rounding error
    got = fma32(s, a, v)
    want = np.array([_fma_exact(*x) for x in zip(s, a, v)], dtype=np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_fma32_on_constructed_double_rounding_cases():
    s, a, v = _midpoint_cases()
    want = np.array([_fma_exact(*x) for x in zip(s, a, v)], dtype=np.float32)
    assert np.array_equal(want, v), "the construction: the exact sum lies under the midpoint"
    plain = (s.astype(np.float64) * a + v).astype(np.float32)
    wrong = int((plain != want).sum())
    print(f"plain fp64 then fp32: wrong on {wrong} of {len(s)} constructed cases")
    assert wrong >= 1, "the constructed cases do not separate fma32 from the plain fp64 path: they test nothing"
    assert np.array_equal(fma32(s, a, v).view(np.int32), want.view(np.int32))
    assert np.array_equal(fma32(-s, a, -v).view(np.int32), (-want).view(np.int32))


def _chain_exact(dst, srcs, scales, skip_zero=True):
    f = Fraction(float(dst))
    for s, a in zip(scales, srcs):
        if not (skip_zero and s == 0):
            f = Fraction(_round(Fraction(float(np.float32(s))) * Fraction(float(a)) + f, 24, -126))
    return np.float16(_round(f, 11, -14))


def test_f16_chain_rounds_once_at_the_end():
    h = np.float16
    cases = [
        # (dst, sources, scales)
        (h(1.0), [h(2.0 ** -11)], [1.0]),                              # 1 + 2^-11: a tie of f16, to the even 1
        (h(1.0 + 2.0 ** -10), [h(2.0 ** -11)], [1.0]),                 # a tie, to the even 1 + 2^-9
        (h(1.0), [h(2.0 ** -11), h(2.0 ** -14)], [1.0, 1.0]),          # the fp32 sum is past the tie: rounding after each source would lose it
        (h(1.0), [h(2.0 ** -11), h(2.0 ** -14)], [1.0, -1.0]),
        (h(0.333), [h(-1.7), h(0.0123), h(1000.0), h(-3.0)], [-0.37, 2.0, 2.0 ** -12, 0.25]),
        (h(6.0e-5), [h(-5.9e-5), h(3.0e-6)], [1.0, 0.5]),              # a subnormal f16 result
        (h(-0.1), [h(7.0), h(0.1)], [0.0, 1.0]),                       # a dead source in front of a live one
    ]
    for dst, srcs, scales in cases:
        got = skip_add_expected(np.array([dst]), [np.array([a]) for a in srcs], scales, np.float16)
        want = _chain_exact(dst, srcs, scales)
        assert got.dtype == np.float16 and got.view(np.int16)[0] == np.array([want]).view(np.int16)[0], (dst, srcs, scales, got, want)
    assert skip_add_expected(np.array([h(1.0)]), [np.array([h(2.0 ** -11)]), np.array([h(2.0 ** -14)])], [1.0, 1.0], np.float16)[0] == h(1.0 + 2.0 ** -10)


def test_scale_zero_and_signed_zeros():
    h, nan = np.float16, np.array([np.float16("nan")])
    one = np.array([h(1.5)])
    # the table forms never look at a source at scale 0; the one-scalar form computes fma(0, src, dst)
    assert skip_add_expected(one, [nan, one], [0.0, 2.0], np.float16)[0] == h(4.5)
    assert skip_add_expected(one, [nan], [0.0], np.float16).view(np.int16)[0] == one.view(np.int16)[0]
    assert np.isnan(skip_add_expected(one, [nan], [0.0], np.float16, skip_zero=False)[0])
    assert skip_add_expected(one, [one], [0.0], np.float16, skip_zero=False)[0] == h(1.5)
    mz, pz = np.array([h(-0.0)]), np.array([h(0.0)])
    for dt in (np.float16, np.float32):
        assert np.signbit(skip_add_expected(mz.astype(dt), [mz.astype(dt)], [1.0], dt)[0])            # 1 * -0 + -0 = -0
        assert not np.signbit(skip_add_expected(mz.astype(dt), [pz.astype(dt)], [1.0], dt)[0])        # 1 * +0 + -0 = +0
        assert not np.signbit(skip_add_expected(mz.astype(dt), [mz.astype(dt)], [-1.0], dt)[0])       # -1 * -0 + -0 = +0
        assert np.signbit(skip_add_expected(mz.astype(dt), [pz.astype(dt)], [0.0], dt)[0])            # skipped: dst keeps its sign
        assert not np.signbit(skip_add_expected(mz.astype(dt), [pz.astype(dt)], [0.0], dt, skip_zero=False)[0])      # 0 * 0 + -0 = +0
    assert fma32(np.float32(3.0), np.float32(-0.0), np.float32(0.0)).view(np.int32).item() == 0
