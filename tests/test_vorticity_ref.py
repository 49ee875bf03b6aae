"""The numpy reference of the vertical vorticity (tests/vorticity_ref.py) held three ways, without a device: against a scalar triple loop
written from the rule, against exact rational arithmetic on cases whose every intermediate is representable, and against the discrete
Stokes identity on integer data."""
from fractions import Fraction

import numpy as np
import pytest

from vorticity_ref import STENCIL, cells_read, interior_vorticity, same_bits, vertical_vorticity


def _random_case(rng, size, halo, dtype):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)
    u, v = rng.uniform(-1, 1, parent).astype(dtype), rng.uniform(-1, 1, parent).astype(dtype)
    dx, dy, az = (rng.uniform(0.5, 2, plane).astype(dtype) for _ in range(3))
    return u, v, dx, dy, az


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_equals_a_scalar_loop_written_from_the_rule(dtype):
    size, halo = (6, 4, 2), (2, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    u, v, dx, dy, az = _random_case(np.random.default_rng(1), size, halo, dtype)
    U = lambda i, j, k: u[k + Hz - 1, j + Hy - 1, i + Hx - 1]
    V = lambda i, j, k: v[k + Hz - 1, j + Hy - 1, i + Hx - 1]
    M = lambda m, i, j: m[j + Hy - 1, i + Hx - 1]
    want = np.empty((Nz, Ny, Nx), dtype)
    for k in range(1, Nz + 1):
        for j in range(1, Ny + 1):
            for i in range(1, Nx + 1):
                a = dtype(M(dy, i, j) * V(i, j, k))
                b = dtype(M(dy, i - 1, j) * V(i - 1, j, k))
                c = dtype(M(dx, i, j) * U(i, j, k))
                d = dtype(M(dx, i, j - 1) * U(i, j - 1, k))
                want[k - 1, j - 1, i - 1] = dtype(dtype(dtype(a - b) - dtype(c - d)) / M(az, i, j))
    got = interior_vorticity(u, v, dx, dy, az, size, halo)
    assert got.dtype == dtype and same_bits(got, want) == 0
    # the parent form: interior replaced, every halo cell of zeta untouched; the mask by its plane
    z0 = np.full(u.shape, 7, dtype)
    out = vertical_vorticity(u, v, z0, dx, dy, az, size, halo)
    assert same_bits(out[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], want) == 0
    halo_cells = np.ones(u.shape, bool)
    halo_cells[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = False
    assert (out[halo_cells] == 7).all()
    n = np.zeros((Ny, Nx), np.int32)
    n[0, 0], n[1, 2], n[3, 5] = 2, 1, 5                           # whole column, one level, more than Nz
    masked = vertical_vorticity(u, v, z0, dx, dy, az, size, halo, n_ff=n, mask_value=-3.0)
    inner = masked[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    expect = want.copy()
    expect[:, 0, 0] = expect[0, 1, 2] = expect[:, 3, 5] = -3
    assert same_bits(inner, expect) == 0


def test_cells_read_are_the_stencil_and_nothing_else():
    size, halo = (6, 4, 2), (2, 3, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    read = cells_read(size, halo)
    assert len(STENCIL) == 9
    # u: rows j = 0..Ny, columns 1..Nx; v: rows 1..Ny, columns 0..Nx; interior levels only
    assert read["u"].sum() == Nz * (Ny + 1) * Nx and read["v"].sum() == Nz * Ny * (Nx + 1)
    assert read["u"][Hz:Hz + Nz, Hy - 1:Hy + Ny, Hx:Hx + Nx].all() and read["v"][Hz:Hz + Nz, Hy:Hy + Ny, Hx - 1:Hx + Nx].all()
    assert not read["u"][:Hz].any() and not read["u"][Hz + Nz:].any() and not read["v"][:Hz].any() and not read["v"][Hz + Nz:].any()
    assert read["dx_fc"].sum() == (Ny + 1) * Nx and read["dy_cf"].sum() == Ny * (Nx + 1) and read["az_ff"].sum() == Ny * Nx
    # poisoning every unread cell changes nothing
    rng = np.random.default_rng(2)
    arrays = dict(zip(("u", "v", "dx_fc", "dy_cf", "az_ff"), _random_case(rng, size, halo, np.float64)))
    want = interior_vorticity(*arrays.values(), size, halo)
    poisoned = {k: np.where(read[k], a, np.nan) for k, a in arrays.items()}
    got = interior_vorticity(*poisoned.values(), size, halo)
    assert not np.isnan(got).any() and same_bits(got, want) == 0


def _exact(u, v, dx, dy, az, size, halo):
    """the rule in exact rational arithmetic, [k][j][i] nested lists of Fractions"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    F = lambda x: Fraction(float(x))
    out = []
    for k in range(Hz, Hz + Nz):
        out.append([[((F(dy[j, i]) * F(v[k, j, i]) - F(dy[j, i - 1]) * F(v[k, j, i - 1]))
                      - (F(dx[j, i]) * F(u[k, j, i]) - F(dx[j - 1, i]) * F(u[k, j - 1, i]))) / F(az[j, i])
                     for i in range(Hx, Hx + Nx)] for j in range(Hy, Hy + Ny)])
    return out


def _equals_exact(got, exact):
    return all(Fraction(float(got[k, j, i])) == exact[k][j][i]
               for k in range(got.shape[0]) for j in range(got.shape[1]) for i in range(got.shape[2]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_cases_against_rational_arithmetic(dtype):
    size, halo = (8, 5, 2), (1, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = (Nz + 2, Ny + 2, Nx + 2), (Ny + 2, Nx + 2)
    ones = np.ones(plane, dtype)
    jj = (np.arange(Ny + 2) - Hy + 1).astype(dtype)[None, :, None]              # the 1-based row index j of every parent row
    ii = (np.arange(Nx + 2) - Hx + 1).astype(dtype)[None, None, :]
    zero = np.zeros(parent, dtype)
    # all metrics 1, u = j: zeta = -(j - (j - 1)) = -1 everywhere
    u = np.broadcast_to(jj, parent).astype(dtype)
    z = interior_vorticity(u, zero, ones, ones, ones, size, halo)
    assert (z == -1).all() and _equals_exact(z, _exact(u, zero, ones, ones, ones, size, halo))
    # v = i with the periodic halo filled (column 0 holds column Nx): +1 for i >= 2, 1 - Nx at i = 1
    v = np.broadcast_to(ii, parent).astype(dtype).copy()
    v[:, :, 0] = v[:, :, Nx]
    v[:, :, Nx + 1] = v[:, :, 1]
    z = interior_vorticity(zero, v, ones, ones, ones, size, halo)
    assert (z[:, :, 1:] == 1).all() and (z[:, :, 0] == 1 - Nx).all()
    assert _equals_exact(z, _exact(zero, v, ones, ones, ones, size, halo))
    # power-of-two metrics, small integer velocities: every product, difference and quotient is representable
    rng = np.random.default_rng(5)
    dx, dy, az = (np.exp2(rng.integers(-3, 4, plane)).astype(dtype) for _ in range(3))
    u, v = rng.integers(-9, 10, parent).astype(dtype), rng.integers(-9, 10, parent).astype(dtype)
    z = interior_vorticity(u, v, dx, dy, az, size, halo)
    assert _equals_exact(z, _exact(u, v, dx, dy, az, size, halo))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_discrete_stokes_identity_on_integer_data(dtype):
    """sum of zeta * Az_ff over an index box [i0, i1] x [j0, j1] = the circulation of (dx u, dy v) round it, exactly: the interior edges cancel.
    Az = 1 keeps every zeta an integer, so the sum is exact in either type."""
    size, halo = (10, 7, 2), (2, 2, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)
    rng = np.random.default_rng(9)
    dx, dy = rng.integers(1, 9, plane).astype(dtype), rng.integers(1, 9, plane).astype(dtype)
    az = np.ones(plane, dtype)
    u, v = rng.integers(-20, 21, parent).astype(dtype), rng.integers(-20, 21, parent).astype(dtype)
    z = interior_vorticity(u, v, dx, dy, az, size, halo)
    U = lambda i, j, k: int(dx[j + Hy - 1, i + Hx - 1]) * int(u[k + Hz - 1, j + Hy - 1, i + Hx - 1])
    V = lambda i, j, k: int(dy[j + Hy - 1, i + Hx - 1]) * int(v[k + Hz - 1, j + Hy - 1, i + Hx - 1])
    boxes = [(1, Nx, 1, Ny), (1, 1, 1, 1), (3, 7, 2, 5), (Nx, Nx, Ny, Ny), (2, Nx, 1, 3)]
    for k in range(1, Nz + 1):
        for i0, i1, j0, j1 in boxes:
            total = int(z[k - 1, j0 - 1:j1, i0 - 1:i1].astype(np.float64).sum())
            # east side v[i1, j] up, west side v[i0-1, j] down; south side u[i, j0-1] eastwards, north side u[i, j1] westwards
            circ = (sum(V(i1, j, k) - V(i0 - 1, j, k) for j in range(j0, j1 + 1))
                    + sum(U(i, j0 - 1, k) - U(i, j1, k) for i in range(i0, i1 + 1)))
            assert total == circ, (k, i0, i1, j0, j1)
