"""The numpy reference of the barotropic mode and the split-explicit velocity correction (tests/barotropic_ref.py) held without a device:
against exact rational arithmetic with one rounding per operation (the scalar operations of tests/test_special_value_refs.py) on a small case
with special values among the data, and against integer data with power-of-two spacings, where the mode is exactly the integer sum."""
import math
from fractions import Fraction

import numpy as np
import pytest

from barotropic_ref import barotropic_correction, barotropic_mode, cells_read, interior_correction, interior_mode, same_bits
from special_values import pool
from test_special_value_refs import _add, _div, _mul, _sub

DTYPES = [np.float32, np.float64]


def _case(rng, size, halo, Hy2, dtype):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy2, Nx + 2 * Hx)
    u, v = rng.uniform(-1, 1, parent).astype(dtype), rng.uniform(-1, 1, parent).astype(dtype)
    U, V, Ub, Vb = (rng.uniform(-1, 1, plane).astype(dtype) for _ in range(4))
    return u, v, U, V, Ub, Vb, rng.uniform(0.5, 2, Nz).astype(dtype), rng.uniform(0.5, 2, Nz + 1).astype(dtype)


def _bits_equal(got, want):
    """a numpy scalar against a Python float: the same bits, NaN by NaN-ness"""
    got = float(got)
    if math.isnan(want):
        return math.isnan(got)
    return got == want and math.copysign(1.0, got) == math.copysign(1.0, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_equals_rational_arithmetic_rounded_once_per_operation(dtype):
    size, halo, Hy2 = (6, 4, 3), (2, 1, 1), 3
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(1)
    u, v, U, V, Ub, Vb, dz, depth = _case(rng, size, halo, Hy2, dtype)
    p = pool(dtype)
    for a in (u, v, U, Ub):                                        # special values among the data: every IEEE rule of *, +, -, /
        where = rng.random(a.shape) < 0.15
        a[where] = p[rng.integers(0, p.size, int(where.sum()))]
    u[Hz, Hy, Hx] = -0.0                                           # a column whose sum is -0 only if the first term is the product itself
    u[Hz + 1:Hz + Nz, Hy, Hx] = -0.0
    depth[2], depth[Nz] = -0.0, 0.0
    n = rng.integers(0, Nz + 3, (Ny, Nx)).astype(np.int32)
    n[0, 0], n[0, 1] = 2, Nz + 2
    mode_u, mode_v = interior_mode(u, dz, size, halo), interior_mode(v, dz, size, halo)
    assert mode_u.dtype == dtype and np.signbit(mode_u[0, 0]) and mode_u[0, 0] == 0
    plain = interior_correction(u, U, Ub, depth, size, halo, Hy2)
    masked = interior_correction(u, U, Ub, depth, size, halo, Hy2, n, 0.1)
    f = float
    for j in range(Ny):
        for i in range(Nx):
            for field, got in ((u, mode_u), (v, mode_v)):
                acc = _mul(f(dz[0]), f(field[Hz, j + Hy, i + Hx]), dtype)
                for k in range(1, Nz):
                    acc = _add(acc, _mul(f(dz[k]), f(field[Hz + k, j + Hy, i + Hx]), dtype), dtype)
                assert _bits_equal(got[j, i], acc), (i, j)
            diff = _sub(f(U[j + Hy2, i + Hx]), f(Ub[j + Hy2, i + Hx]), dtype)
            c0 = _div(diff, f(depth[0]), dtype)
            cn = _div(diff, f(depth[min(int(n[j, i]), Nz)]), dtype)
            for k in range(Nz):
                x = f(u[Hz + k, j + Hy, i + Hx])
                assert _bits_equal(plain[k, j, i], _add(x, c0, dtype)), (i, j, k)
                want = f(dtype(0.1)) if k + 1 <= n[j, i] else _add(x, cn, dtype)
                assert _bits_equal(masked[k, j, i], want), (i, j, k)
    assert np.isnan(plain).any() and np.isinf(plain).any() and np.isfinite(plain).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_parents_keep_every_halo_cell_and_the_forms_agree(dtype):
    size, halo, Hy2 = (6, 4, 3), (2, 1, 1), 3
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    u, v, U, V, Ub, Vb, dz, depth = _case(np.random.default_rng(2), size, halo, Hy2, dtype)
    s = np.full(U.shape, 7, dtype)
    mu, mv = barotropic_mode(u, v, s, s, dz, size, halo, Hy2)
    assert same_bits(mu[Hy2:Hy2 + Ny, Hx:Hx + Nx], interior_mode(u, dz, size, halo)) == 0
    assert same_bits(mv[Hy2:Hy2 + Ny, Hx:Hx + Nx], interior_mode(v, dz, size, halo)) == 0
    edge = np.ones(s.shape, bool)
    edge[Hy2:Hy2 + Ny, Hx:Hx + Nx] = False
    assert (mu[edge] == 7).all() and (mv[edge] == 7).all() and (s == 7).all()
    only_u, none = barotropic_mode(u, None, s, None, dz, size, halo, Hy2)
    assert none is None and same_bits(only_u, mu) == 0
    none, only_v = barotropic_mode(None, v, None, s, dz, size, halo, Hy2)
    assert none is None and same_bits(only_v, mv) == 0
    n = np.zeros((Ny, Nx), np.int32)
    n[0, 0], n[1, 2], n[3, 5] = 3, 1, 5
    cu, cv = barotropic_correction(u, v, U, V, Ub, Vb, depth, size, halo, Hy2, n_fc=n, mask_value=-3.0)
    inner = np.zeros(u.shape, bool)
    inner[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = True
    assert same_bits(cu[~inner], u[~inner]) == 0 and same_bits(cv[~inner], v[~inner]) == 0
    got = cu[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    assert (got[:, 0, 0] == -3).all() and got[0, 1, 2] == -3 and (got[:, 3, 5] == -3).all() and (got == -3).sum() == 3 + 1 + 3
    c = (V[Hy2:Hy2 + Ny, Hx:Hx + Nx] - Vb[Hy2:Hy2 + Ny, Hx:Hx + Nx]) / depth[0]         # v has no plane: depth_of_count[0], no mask
    assert same_bits(cv[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], v[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] + c[None]) == 0
    only_u, none = barotropic_correction(u, None, U, None, Ub, None, depth, size, halo, Hy2, n_fc=n, mask_value=-3.0)
    assert none is None and same_bits(only_u, cu) == 0
    # the cells read: the interiors, and the entries of depth_of_count some count selects
    read = cells_read(size, halo, Hy2, n, None)
    assert read["field"].sum() == Nx * Ny * Nz and read["plane"].sum() == Nx * Ny and np.array_equal(read["field"], inner)
    assert read["depth_of_count"].tolist() == [True, True, False, True]
    assert cells_read(size, halo, Hy2)["depth_of_count"].tolist() == [True, False, False, False]
    poisoned = [np.where(read["field"], a, np.nan).astype(dtype) for a in (u, v)] + [np.where(read["plane"], a, np.nan).astype(dtype) for a in (U, V, Ub, Vb)]
    pd = np.where(read["depth_of_count"], depth, np.nan).astype(dtype)
    pu, pv = barotropic_correction(*poisoned, pd, size, halo, Hy2, n_fc=n, mask_value=-3.0)
    assert same_bits(pu[inner], cu[inner]) == 0 and same_bits(pv[inner], cv[inner]) == 0 and not np.isnan(pu[inner]).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_data_with_power_of_two_spacings_is_the_exact_sum(dtype):
    """integer u, power-of-two dz_c: every product and partial sum is representable, so Ubar is the integer sum exactly; with U given and
    H = sum dz_c a power of two, the corrected u has mode(u) == U exactly"""
    size, halo, Hy2 = (8, 5, 4), (1, 2, 1), 2
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(5)
    parent, plane = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy2, Nx + 2 * Hx)
    u = rng.integers(-9, 10, parent).astype(dtype)
    dz = np.array([1, 2, 4, 1], dtype)                             # sum 8
    got = interior_mode(u, dz, size, halo)
    exact = [[sum(Fraction(int(dz[k])) * Fraction(int(u[Hz + k, j + Hy, i + Hx])) for k in range(Nz)) for i in range(Nx)] for j in range(Ny)]
    assert all(Fraction(float(got[j, i])) == exact[j][i] for j in range(Ny) for i in range(Nx))
    U = rng.integers(-64, 65, plane).astype(dtype)
    Ubar, _ = barotropic_mode(u, None, np.zeros(plane, dtype), None, dz, size, halo, Hy2)
    depth = np.array([8, 7, 5, 1, 0], dtype)
    corrected, _ = barotropic_correction(u, None, U, None, Ubar, None, depth, size, halo, Hy2)
    again = interior_mode(corrected, dz, size, halo)
    assert same_bits(again, U[Hy2:Hy2 + Ny, Hx:Hx + Nx]) == 0
