"""The numpy reference of the AB2 step and the barotropic forcing (tests/ab2_ref.py) held without a device: against exact rational
arithmetic with one rounding per operation (the scalar operations of tests/test_special_value_refs.py) on a small case with special values
among the data, and against integer data with power-of-two spacings, step and factors, where every result is the exact integer expression."""
import math
from fractions import Fraction

import numpy as np
import pytest

from ab2_ref import EULER, STORE, ab2_step, cells_read, constants, interior_step, same_bits
from special_values import pool
from test_special_value_refs import _add, _mul, _sub

DTYPES = [np.float32, np.float64]
SIZE, HALO, HY2 = (6, 4, 3), (2, 1, 1), 3
DT, CHI = 0.3, 0.1


def _case(rng, dtype):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = SIZE, HALO
    parent = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    x, Gn, Gm = (rng.uniform(-1, 1, parent).astype(dtype) for _ in range(3))
    return x, Gn, Gm, rng.uniform(0.5, 2, Nz).astype(dtype)


def _bits_equal(got, want):
    """a numpy scalar against a Python float: the same bits, NaN by NaN-ness"""
    got = float(got)
    if math.isnan(want):
        return math.isnan(got)
    return got == want and math.copysign(1.0, got) == math.copysign(1.0, want)


def _counts(rng):
    (Nx, Ny, Nz) = SIZE
    n = rng.integers(0, Nz + 1, (Ny, Nx)).astype(np.int32)
    n[0, 0], n[0, 1], n[0, 2], n[0, 3], n[0, 4] = 0, 2, Nz, Nz + 2, -1
    return n


@pytest.mark.parametrize("euler", [False, True], ids=["ab2", "euler"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_equals_rational_arithmetic_rounded_once_per_operation(dtype, euler):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = SIZE, HALO
    rng = np.random.default_rng(1)
    x, Gn, Gm, dz = _case(rng, dtype)
    p = pool(dtype)
    for a in (x, Gn, Gm):                                          # special values among the data: every IEEE rule of *, +, -
        where = rng.random(a.shape) < 0.15
        a[where] = p[rng.integers(0, p.size, int(where.sum()))]
    # a column whose integral is -0 only if the first term is the product itself: every g is -0 (c1 * -0 - c2 * +0 = -0 - +0 = -0)
    Gn[Hz:Hz + Nz, Hy + 1, Hx] = -0.0
    Gm[Hz:Hz + Nz, Hy + 1, Hx] = 0.0
    x[Hz, Hy + 2, Hx + 1], Gn[Hz + 1, Hy + 2, Hx + 2], x[Hz + 1, Hy + 2, Hx + 2] = np.nan, np.inf, 1.0   # one NaN, one Inf, whatever the draw
    n = _counts(rng)
    n[1, 0] = 0
    flags = EULER if euler else 0
    plain, open_sum = interior_step(x, Gn, Gm, DT, CHI, flags, SIZE, HALO, dz)
    masked, masked_sum = interior_step(x, Gn, Gm, DT, CHI, flags, SIZE, HALO, dz, n)
    assert same_bits(plain, masked) == 0                           # the field is stepped with the unmasked g
    assert open_sum.dtype == dtype and np.signbit(open_sum[1, 0]) and open_sum[1, 0] == 0 and np.signbit(masked_sum[1, 0])
    f = float
    c1, c2, dt = (f(c) for c in constants(DT, CHI, dtype))
    assert c1 == _add(1.5, f(dtype(CHI)), dtype) and c2 == _add(0.5, f(dtype(CHI)), dtype) and dt == f(dtype(DT))
    for j in range(Ny):
        for i in range(Nx):
            m = min(max(int(n[j, i]), 0), Nz)
            acc = acc_m = None
            for k in range(Nz):
                at = (Hz + k, j + Hy, i + Hx)
                g = _mul(c1, f(Gn[at]), dtype)
                if not euler:
                    g = _sub(g, _mul(c2, f(Gm[at]), dtype), dtype)
                assert _bits_equal(plain[k, j, i], _add(f(x[at]), _mul(dt, g, dtype), dtype)), (i, j, k)
                gh = 0.0 if k + 1 <= m else g
                t, tm = _mul(f(dz[k]), g, dtype), _mul(f(dz[k]), gh, dtype)
                acc, acc_m = (t, tm) if k == 0 else (_add(acc, t, dtype), _add(acc_m, tm, dtype))
            assert _bits_equal(open_sum[j, i], acc) and _bits_equal(masked_sum[j, i], acc_m), (i, j)
    assert np.isnan(plain).any() and np.isinf(plain).any() and np.isfinite(plain).any()
    # counts 0, 2, Nz, Nz + 2 and -1: 0 and -1 mask nothing, Nz and Nz + 2 every level (the integral is +0 or NaN from 0 * Inf alone)
    for i, levels in ((0, 0), (1, 2), (2, Nz), (3, Nz), (4, 0)):
        assert min(max(int(n[0, i]), 0), Nz) == levels
    assert same_bits(masked_sum[0, 0], open_sum[0, 0]) == 0 and same_bits(masked_sum[0, 4], open_sum[0, 4]) == 0
    if np.isfinite(dz).all():
        assert masked_sum[0, 2] == 0 and not np.signbit(masked_sum[0, 2]) and masked_sum[0, 3] == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_euler_never_reads_the_previous_tendency(dtype):
    """with EULER a Gm full of NaN leaves no NaN anywhere: not in the field, not in the integral, and with STORE it is overwritten"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = SIZE, HALO
    rng = np.random.default_rng(2)
    x, Gn, Gm, dz = _case(rng, dtype)
    nan = np.full(Gm.shape, np.nan, dtype)
    G0 = np.full((Ny + 2 * HY2, Nx + 2 * Hx), 7, dtype)
    for flags in (EULER, EULER | STORE):
        got = ab2_step(x, Gn, nan, DT, CHI, flags, SIZE, HALO, G0, dz, HY2, _counts(rng))
        want = ab2_step(x, Gn, Gm, DT, CHI, flags, SIZE, HALO, G0, dz, HY2, None)
        assert not np.isnan(got[0]).any() and not np.isnan(got[2]).any() and same_bits(got[0], want[0]) == 0
        inner = got[1][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
        assert np.isnan(inner).all() != bool(flags & STORE)
        if flags & STORE:
            assert same_bits(inner, Gn[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]) == 0
    none = ab2_step(x, Gn, None, DT, CHI, EULER, SIZE, HALO)
    assert none[1] is None and none[2] is None and same_bits(none[0], want[0]) == 0
    with pytest.raises((AttributeError, TypeError)):               # without EULER the previous tendency IS read
        ab2_step(x, Gn, None, DT, CHI, 0, SIZE, HALO)


@pytest.mark.parametrize("dtype", DTYPES)
def test_parents_keep_every_halo_cell(dtype):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = SIZE, HALO
    rng = np.random.default_rng(3)
    x, Gn, Gm, dz = _case(rng, dtype)
    G0 = np.full((Ny + 2 * HY2, Nx + 2 * Hx), 7, dtype)
    out, prev, G = ab2_step(x, Gn, Gm, DT, CHI, STORE, SIZE, HALO, G0, dz, HY2)
    inner = cells_read(SIZE, HALO, HY2)["field"]
    assert inner.sum() == Nx * Ny * Nz and not cells_read(SIZE, HALO, HY2)["plane"].any()
    assert same_bits(out[~inner], x[~inner]) == 0 and same_bits(prev[~inner], Gm[~inner]) == 0 and same_bits(prev[inner], Gn[inner]) == 0
    assert (out[inner] != x[inner]).mean() > 0.9
    edge = np.ones(G.shape, bool)
    edge[HY2:HY2 + Ny, Hx:Hx + Nx] = False
    assert (G[edge] == 7).all() and (G0 == 7).all() and not (G[~edge] == 7).any()
    kept = ab2_step(x, Gn, Gm, DT, CHI, 0, SIZE, HALO)
    assert same_bits(kept[1], Gm) == 0 and kept[2] is None and same_bits(kept[0], out) == 0
    # cells outside the rule are not read
    poisoned = [np.where(inner, a, np.nan).astype(dtype) for a in (x, Gn, Gm)]
    got = ab2_step(*poisoned, DT, CHI, STORE, SIZE, HALO, G0, dz, HY2)
    assert same_bits(got[0][inner], out[inner]) == 0 and same_bits(got[2], G) == 0 and not np.isnan(got[2]).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_data_with_power_of_two_factors_is_the_exact_expression(dtype):
    """integer x, Gn, Gm; dt = 2, chi = 0.5 (c1 = 2, c2 = 1), dz_c powers of two: every product, difference and partial sum is
    representable, so every result is the exact integer expression"""
    size, halo, Hy2 = (8, 5, 4), (1, 2, 1), 2
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(5)
    parent = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    x, Gn, Gm = (rng.integers(-9, 10, parent).astype(dtype) for _ in range(3))
    dz = np.array([1, 2, 4, 1], dtype)
    n = rng.integers(-1, Nz + 2, (Ny, Nx)).astype(np.int32)
    assert tuple(float(c) for c in constants(2.0, 0.5, dtype)) == (2.0, 1.0, 2.0)
    for flags in (0, EULER):
        step, integral = interior_step(x, Gn, Gm, 2.0, 0.5, flags, size, halo, dz, n)
        for j in range(Ny):
            for i in range(Nx):
                total = Fraction(0)
                for k in range(Nz):
                    at = (Hz + k, j + Hy, i + Hx)
                    g = 2 * Fraction(int(Gn[at])) - (0 if flags else Fraction(int(Gm[at])))
                    assert Fraction(float(step[k, j, i])) == Fraction(int(x[at])) + 2 * g
                    total += int(dz[k]) * (g if k + 1 > min(max(int(n[j, i]), 0), Nz) else 0)
                assert Fraction(float(integral[j, i])) == total
