"""The numpy references of the Value / Gradient fill (value_gradient_ref.extrapolate) and of the advection timescale
(reduction_ref.cell_advection_timescale) at the IEEE special values of tests/special_values.py, against a high-precision layer that shares
nothing with numpy's floating point: every single operation is recomputed EXACTLY with fractions.Fraction and rounded once to the field
type -- nearest, ties to even, on the type's grid with its subnormal range, overflowing to +-Inf -- and operations with a non-finite or
zero-divisor operand go through the short explicit table of IEEE 754 rules below.  numpy's bits are required (NaN: NaN-ness).  The GPU
tests (tests/test_gpu_special_values.py) hold the kernels to the same numpy references on the same cases."""
import math
from fractions import Fraction

import numpy as np
import pytest

import special_values as sv
from reduction_ref import cell_advection_timescale
from value_gradient_ref import GRADIENT, VALUE, extrapolate

FORMATS = {np.float32: (24, -126, 127), np.float64: (53, -1022, 1023)}     # precision, emin, emax
DTYPES = [np.float32, np.float64]


def _floor_log2(x):
    """floor(log2 x) of a positive Fraction, exactly"""
    e = x.numerator.bit_length() - x.denominator.bit_length()
    return e if Fraction(2) ** e <= x else e - 1


def round_to(x, dtype):
    """the exact NONZERO rational x rounded once to `dtype`, as a Python float (every Float32 is one exactly)"""
    p, emin, emax = FORMATS[dtype]
    sign, mag = (-1.0, -x) if x < 0 else (1.0, x)
    e = max(_floor_log2(mag), emin)                                # below emin the grid is the subnormal one
    quantum = Fraction(2) ** (e - p + 1)
    n, rest = divmod(mag, quantum)
    n = int(n)
    if rest > quantum / 2 or (rest == quantum / 2 and n % 2 == 1):
        n += 1
    value = n * quantum
    if value >= Fraction(2) ** (emax + 1):
        return sign * math.inf
    return math.copysign(float(value), sign)                       # n = 0: a signed zero


def _neg(a):
    return -a


def _mul(a, b, dtype):
    if math.isnan(a) or math.isnan(b):
        return math.nan
    sign = math.copysign(1.0, a) * math.copysign(1.0, b)
    if math.isinf(a) or math.isinf(b):
        return math.nan if (a == 0 or b == 0) else sign * math.inf                 # Inf * 0 = NaN
    if a == 0 or b == 0:
        return math.copysign(0.0, sign)
    return round_to(Fraction(a) * Fraction(b), dtype)


def _div(a, b, dtype):
    if math.isnan(a) or math.isnan(b):
        return math.nan
    sign = math.copysign(1.0, a) * math.copysign(1.0, b)
    if math.isinf(a):
        return math.nan if math.isinf(b) else sign * math.inf                      # Inf / Inf = NaN
    if math.isinf(b):
        return math.copysign(0.0, sign)
    if b == 0:
        return math.nan if a == 0 else sign * math.inf                             # 0 / 0 = NaN, x / 0 = +-Inf
    if a == 0:
        return math.copysign(0.0, sign)
    return round_to(Fraction(a) / Fraction(b), dtype)


def _add(a, b, dtype):
    if math.isnan(a) or math.isnan(b):
        return math.nan
    if math.isinf(a) or math.isinf(b):
        if math.isinf(a) and math.isinf(b):
            return a if a == b else math.nan                                       # Inf - Inf = NaN
        return a if math.isinf(a) else b
    exact = Fraction(a) + Fraction(b)
    if exact == 0:                                                                 # x + (-x) = +0; -0 + -0 = -0
        return -0.0 if (math.copysign(1.0, a) < 0 and math.copysign(1.0, b) < 0) else 0.0
    return round_to(exact, dtype)


def _sub(a, b, dtype):
    return _add(a, _neg(b), dtype)


def _extrapolate(kind, c1, cond, d, upper, dtype):
    """value_gradient_ref's rule, one operation at a time"""
    if kind == VALUE:
        half = _div(d, 2.0, dtype)
        grad = _div(_sub(cond, c1, dtype) if upper else _sub(c1, cond, dtype), half, dtype)
    else:
        grad = cond
    return _add(c1, _mul(grad, d if upper else _neg(d), dtype), dtype)


def _same(got, want, dtype):
    got, want = dtype(got), dtype(want)
    return bool(sv.same_bits_or_both_nan(np.array([got]), np.array([want]))[0])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_round_to_is_the_types_own_rounding(dtype):
    """the rounding itself, against conversions that are exact by construction: every pool value is a fixed point; halfway cases go to the
    even neighbour at 1, at the smallest normal, in the subnormal range and at the overflow threshold"""
    p, emin, emax = FORMATS[dtype]
    for x in sv.pool(dtype):
        if np.isfinite(x) and x != 0:
            assert round_to(Fraction(float(x)), dtype) == float(x)
    ulp1 = Fraction(2) ** (1 - p)
    assert round_to(1 + ulp1 / 2, dtype) == 1.0 and round_to(1 + 3 * ulp1 / 2, dtype) == float(1 + 2 * ulp1)
    assert round_to(1 + ulp1 / 2 + ulp1 / 1024, dtype) == float(1 + ulp1)
    sub = Fraction(float(np.finfo(dtype).smallest_subnormal))
    assert sub == Fraction(2) ** (emin - p + 1)
    assert round_to(sub / 2, dtype) == 0.0 and math.copysign(1.0, round_to(-sub / 2, dtype)) == -1.0
    assert round_to(3 * sub / 2, dtype) == float(2 * sub) and round_to(sub * 3 / 4, dtype) == float(sub)
    big = Fraction(float(np.finfo(dtype).max))
    half_ulp = Fraction(2) ** (emax - p)
    assert round_to(big + half_ulp - 1, dtype) == float(big) and round_to(big + half_ulp, dtype) == math.inf
    assert round_to(-(big + half_ulp), dtype) == -math.inf
    tiny = Fraction(float(np.finfo(dtype).tiny))
    assert round_to(tiny - sub / 2, dtype) == float(tiny) and round_to(tiny - sub, dtype) == float(tiny - sub)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_extrapolate_matches_exact_arithmetic_on_every_pair(dtype):
    """both kinds, lower and upper side, the five spacings, the 361 pairs: numpy's result of every cell has the bits of the exact
    computation; per case at most 30 % of the cells are NaN (so that NaN cannot swamp a case), and subnormal and signed-zero results occur"""
    src, cond = sv.pairs(dtype)
    shares, subnormal, negzero = [], 0, 0
    tiny = np.finfo(dtype).tiny
    for kind in (VALUE, GRADIENT):
        for upper in (False, True):
            for d in sv.spacings(dtype):
                with np.errstate(all="ignore"):
                    got = extrapolate(kind, src, cond, d, upper)
                assert got.dtype == dtype
                for q in range(src.size):
                    want = _extrapolate(kind, float(src[q]), float(cond[q]), float(d), upper, dtype)
                    assert _same(got[q], want, dtype), (kind, upper, float(d), float(src[q]), float(cond[q]), float(got[q]), want)
                shares.append(float(np.isnan(got).mean()))
                subnormal += int(((got != 0) & (np.abs(got) < tiny)).sum())
                negzero += int(((got == 0) & np.signbit(got)).sum())
    assert max(shares) <= 0.30, shares
    assert subnormal > 0 and negzero > 0
    print(f"{np.dtype(dtype).name}: NaN share per case min {min(shares):.3f} max {max(shares):.3f}; subnormal results {subnormal}, -0 results {negzero}")


def _tau_of(cell, dtype):
    a = lambda x: abs(float(x))
    s = _add(_add(_div(a(cell["u"]), float(cell["dx"]), dtype), _div(a(cell["v"]), float(cell["dy"]), dtype), dtype),
             _div(a(cell["w"]), float(cell["dz"]), dtype), dtype)
    return _div(1.0, s, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_timescale_matches_exact_arithmetic_on_every_row(dtype):
    """every row of the table on a small array: the reference's minimum equals the exact computation over the four classes of cells the
    row creates -- the planted cell, the other levels of its column (its dx, dy), the other columns of its level (its dz), the rest --
    with a NaN in any of them winning.  The Float32 rows named in the table have the values the table states."""
    size, halo = (6, 4, 3), (1, 1, 1)
    at = (2, 3, 5)
    one, zero = dtype(1), dtype(0)
    seen = {}
    for name, cell in sv.timescale_rows(dtype):
        u, v, w, dx, dy, dz = sv.timescale_arrays(cell, size, halo, at)
        got = cell_advection_timescale(u, v, w, dx, dy, dz, size, halo)
        classes = [cell,
                   {**cell, "u": zero, "v": zero, "w": zero, "dz": one},
                   {**cell, "u": zero, "v": zero, "w": zero, "dx": one, "dy": one},
                   dict(u=zero, v=zero, w=zero, dx=one, dy=one, dz=one)]
        taus = [_tau_of(c, dtype) for c in classes]
        want = math.nan if any(math.isnan(t) for t in taus) else min(taus)
        assert _same(dtype(got), want, dtype), (name, float(got), want, taus)
        seen[name] = float(got)
    assert seen["smallest subnormal over 1"] == math.inf and seen["max over smallest normal"] == 0.0
    assert math.isfinite(seen["largest subnormal over 1"]) and seen["largest subnormal over 1"] > 0
    assert math.isfinite(seen["0.3 smallest normal over 1"])
    assert math.isnan(seen["0 over 0"]) and math.isnan(seen["Inf over Inf"])
    assert seen["all three -0"] == math.inf and seen["0.75 max + 0.75 max"] == 0.0 and seen["1 over smallest subnormal"] == 0.0
    for name in list(seen):
        if name + " (w, dz)" in seen:
            a, b = seen[name], seen[name + " (w, dz)"]
            assert a == b or (math.isnan(a) and math.isnan(b)), name
    if dtype == np.float32:
        assert 8.4e37 < seen["largest subnormal over 1"] < 8.6e37
