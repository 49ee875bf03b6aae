"""The numpy reference of w from continuity and the horizontal divergence (tests/continuity_ref.py) held three ways, without a device: against
a scalar triple loop written from the rule, against exact rational arithmetic on cases whose every intermediate is representable, and against
the discrete Gauss identity on such data."""
from fractions import Fraction

import numpy as np
import pytest

from continuity_ref import STENCIL, cells_read, interior_w_and_divergence, same_bits, w_and_divergence


def _random_case(rng, size, halo, dtype):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)
    u, v = rng.uniform(-1, 1, parent).astype(dtype), rng.uniform(-1, 1, parent).astype(dtype)
    dy, dx, az = (rng.uniform(0.5, 2, plane).astype(dtype) for _ in range(3))
    dz = rng.uniform(0.5, 2, Nz).astype(dtype)
    return u, v, dy, dx, az, dz


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_equals_a_scalar_loop_written_from_the_rule(dtype):
    size, halo = (6, 4, 3), (2, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    u, v, dy, dx, az, dz = _random_case(np.random.default_rng(1), size, halo, dtype)
    U = lambda i, j, k: u[k + Hz - 1, j + Hy - 1, i + Hx - 1]
    V = lambda i, j, k: v[k + Hz - 1, j + Hy - 1, i + Hx - 1]
    M = lambda m, i, j: m[j + Hy - 1, i + Hx - 1]
    want_w, want_d = np.empty((Nz + 1, Ny, Nx), dtype), np.empty((Nz, Ny, Nx), dtype)
    for j in range(1, Ny + 1):
        for i in range(1, Nx + 1):
            w = dtype(0)
            want_w[0, j - 1, i - 1] = w
            for k in range(1, Nz + 1):
                d = dz[k - 1]
                fe = dtype(dtype(M(dy, i + 1, j) * d) * U(i + 1, j, k))
                fw = dtype(dtype(M(dy, i, j) * d) * U(i, j, k))
                fn = dtype(dtype(M(dx, i, j + 1) * d) * V(i, j + 1, k))
                fs = dtype(dtype(M(dx, i, j) * d) * V(i, j, k))
                vol = dtype(M(az, i, j) * d)
                div = dtype(dtype(dtype(1) / vol) * dtype(dtype(fe - fw) + dtype(fn - fs)))
                w = dtype(w - dtype(d * div))
                want_d[k - 1, j - 1, i - 1] = div
                want_w[k, j - 1, i - 1] = w
    got_w, got_d = interior_w_and_divergence(u, v, dy, dx, az, dz, size, halo)
    assert got_w.dtype == dtype and got_d.dtype == dtype
    assert same_bits(got_w, want_w) == 0 and same_bits(got_d, want_d) == 0
    assert not np.signbit(got_w[0]).any()                          # +0
    # the parent form: interior replaced, every halo cell keeps the sentinel (w: Nz + 1 levels and both extra halo planes)
    w0, d0 = np.full((Nz + 1 + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), 7, dtype), np.full(u.shape, 7, dtype)
    pw, pd = w_and_divergence(u, v, w0, d0, dy, dx, az, dz, size, halo)
    assert same_bits(pw[Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx:Hx + Nx], want_w) == 0 and same_bits(pd[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], want_d) == 0
    hw, hd = np.ones(w0.shape, bool), np.ones(d0.shape, bool)
    hw[Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx:Hx + Nx] = False
    hd[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = False
    assert (pw[hw] == 7).all() and (pd[hd] == 7).all() and hw.sum() == w0.size - (Nz + 1) * Ny * Nx
    assert w_and_divergence(u, v, None, d0, dy, dx, az, dz, size, halo)[0] is None
    assert w_and_divergence(u, v, w0, None, dy, dx, az, dz, size, halo)[1] is None
    # the mask by its plane: a whole column, one level, more than Nz; everywhere else n = 0 (w's bottom face is always masked)
    n = np.zeros((Ny, Nx), np.int32)
    n[0, 0], n[1, 2], n[3, 5] = 3, 1, 5
    mw, md = w_and_divergence(u, v, w0, d0, dy, dx, az, dz, size, halo, n_cc=n, mask_value=-3.0)
    ew, ed = want_w.copy(), want_d.copy()
    ed[:, 0, 0] = ed[0, 1, 2] = ed[:, 3, 5] = -3
    ew[0] = -3                                                     # k = 1 <= min(n + 1, Nz) for every n >= 0
    ew[:3, 0, 0] = ew[:2, 1, 2] = ew[:3, 3, 5] = -3                # faces 1..min(n + 1, Nz): the top face Nz + 1 is never masked
    assert same_bits(mw[Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx:Hx + Nx], ew) == 0 and same_bits(md[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], ed) == 0
    assert (mw[hw] == 7).all() and (md[hd] == 7).all()


def test_cells_read_are_the_stencil_and_nothing_else():
    size, halo = (6, 4, 2), (2, 3, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    read = cells_read(size, halo)
    assert len(STENCIL) == 9
    # u: columns 1..Nx+1, rows 1..Ny; v: columns 1..Nx, rows 1..Ny+1; interior levels only
    assert read["u"].sum() == Nz * Ny * (Nx + 1) and read["v"].sum() == Nz * (Ny + 1) * Nx
    assert read["u"][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx + 1].all() and read["v"][Hz:Hz + Nz, Hy:Hy + Ny + 1, Hx:Hx + Nx].all()
    assert not read["u"][:Hz].any() and not read["u"][Hz + Nz:].any() and not read["v"][:Hz].any() and not read["v"][Hz + Nz:].any()
    assert read["dy_fc"].sum() == Ny * (Nx + 1) and read["dx_cf"].sum() == (Ny + 1) * Nx and read["az_cc"].sum() == Ny * Nx
    assert read["dy_fc"][Hy:Hy + Ny, Hx:Hx + Nx + 1].all() and read["dx_cf"][Hy:Hy + Ny + 1, Hx:Hx + Nx].all() and read["az_cc"][Hy:Hy + Ny, Hx:Hx + Nx].all()
    # poisoning every unread cell changes nothing
    rng = np.random.default_rng(2)
    u, v, dy, dx, az, dz = _random_case(rng, size, halo, np.float64)
    arrays = {"u": u, "v": v, "dy_fc": dy, "dx_cf": dx, "az_cc": az}
    want = interior_w_and_divergence(u, v, dy, dx, az, dz, size, halo)
    poisoned = {k: np.where(read[k], a, np.nan) for k, a in arrays.items()}
    assert all(np.isnan(p).any() for p in poisoned.values())
    got = interior_w_and_divergence(*poisoned.values(), dz, size, halo)
    for g, wnt in zip(got, want):
        assert not np.isnan(g).any() and same_bits(g, wnt) == 0


def _exact_case(rng, size, halo, dtype):
    """integer u, v with power-of-two metrics and spacings: every product, difference, reciprocal and quotient of the rule is representable"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)
    dy, dx, az = (np.exp2(rng.integers(-3, 4, plane)).astype(dtype) for _ in range(3))
    dz = np.exp2(rng.integers(-2, 3, Nz)).astype(dtype)
    u, v = rng.integers(-9, 10, parent).astype(dtype), rng.integers(-9, 10, parent).astype(dtype)
    return u, v, dy, dx, az, dz


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_cases_against_rational_arithmetic(dtype):
    size, halo = (8, 5, 3), (1, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    F = lambda x: Fraction(float(x))
    u, v, dy, dx, az, dz = _exact_case(np.random.default_rng(5), size, halo, dtype)
    w, div = interior_w_and_divergence(u, v, dy, dx, az, dz, size, halo)
    for j in range(Hy, Hy + Ny):
        for i in range(Hx, Hx + Nx):
            acc = Fraction(0)
            assert F(w[0, j - Hy, i - Hx]) == 0
            for k in range(Nz):
                d, kk = F(dz[k]), k + Hz
                fe, fw = F(dy[j, i + 1]) * d * F(u[kk, j, i + 1]), F(dy[j, i]) * d * F(u[kk, j, i])
                fn, fs = F(dx[j + 1, i]) * d * F(v[kk, j + 1, i]), F(dx[j, i]) * d * F(v[kk, j, i])
                dv = (1 / (F(az[j, i]) * d)) * ((fe - fw) + (fn - fs))
                acc -= d * dv
                assert F(div[k, j - Hy, i - Hx]) == dv and F(w[k + 1, j - Hy, i - Hx]) == acc, (i, j, k)
    # all metrics and spacings 1, u = i with the periodic halo filled, v = 0: div = 1 for i < Nx, 1 - Nx at i = Nx; w[k+1] = -k div
    ones, one_z = np.ones((Ny + 2, Nx + 2), dtype), np.ones(Nz, dtype)
    ii = (np.arange(Nx + 2) - Hx + 1).astype(dtype)
    ui = np.broadcast_to(ii[None, None, :], (Nz + 2, Ny + 2, Nx + 2)).astype(dtype).copy()
    ui[:, :, Nx + 1] = ui[:, :, 1]
    w, div = interior_w_and_divergence(ui, np.zeros_like(ui), ones, ones, ones, one_z, size, halo)
    assert (div[:, :, :-1] == 1).all() and (div[:, :, -1] == 1 - Nx).all()
    assert all((w[k] == -k * div[0]).all() for k in range(Nz + 1))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_discrete_gauss_identity_on_exact_data(dtype):
    """x-periodic halos: at each level the sum of V * div over the interior equals the north flux row minus the south flux row exactly (the
    x-fluxes telescope round the circle, the inner y-fluxes cancel), and w[Nz+1] = -sum_k d * div"""
    size, halo = (10, 7, 3), (2, 2, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    u, v, dy, dx, az, dz = _exact_case(np.random.default_rng(9), size, halo, dtype)
    for a in (u, dy):                                              # the periodic image: column Nx + 1 is column 1
        a[..., Hx + Nx:] = a[..., Hx:2 * Hx]
    w, div = interior_w_and_divergence(u, v, dy, dx, az, dz, size, halo)
    F = lambda x: Fraction(float(x))
    for k in range(Nz):
        d = F(dz[k])
        total = sum(F(az[j + Hy, i + Hx]) * d * F(div[k, j, i]) for j in range(Ny) for i in range(Nx))
        north = sum(F(dx[Hy + Ny, i]) * d * F(v[Hz + k, Hy + Ny, i]) for i in range(Hx, Hx + Nx))
        south = sum(F(dx[Hy, i]) * d * F(v[Hz + k, Hy, i]) for i in range(Hx, Hx + Nx))
        assert total == north - south, k
    for j in range(Ny):
        for i in range(Nx):
            assert F(w[Nz, j, i]) == -sum(F(dz[k]) * F(div[k, j, i]) for k in range(Nz))
