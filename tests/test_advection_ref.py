"""The numpy reference of the tracer advection tendency (tests/advection_ref.py) held without a device, every check in Python Fractions:
against the rule evaluated node by node with every intermediate rounded by hand, against the telescoping identity and the constant-tracer
identity in exact rationals on data whose every intermediate is representable, and its stencil and mask."""
from fractions import Fraction

import numpy as np
import pytest

from advection_ref import STENCIL, cells_read, interior_tendency, same_bits, tendency
from continuity_ref import interior_w_and_divergence

FORMAT = {np.float32: (24, -126), np.float64: (53, -1022)}         # significand bits, exponent of the smallest normal number


def rnd(x, dtype):
    """the Fraction x rounded to the nearest number of `dtype`, ties to even, as a Fraction (the cases stay far from overflow)"""
    if x == 0:
        return Fraction(0)
    p, emin = FORMAT[dtype]
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (max(e, emin) - p + 1)
    n = a / ulp
    lo = n.numerator // n.denominator
    rem = n - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2):
        lo += 1
    return (lo * ulp) * (1 if x > 0 else -1)


def test_rounding_by_hand_is_the_formats():
    rng = np.random.default_rng(0)
    for dtype in (np.float32, np.float64):
        a, b = rng.uniform(-2, 2, 200).astype(dtype), rng.uniform(0.5, 2, 200).astype(dtype)
        F = lambda x: Fraction(float(x))
        for x, y in zip(a, b):
            assert rnd(F(x) * F(y), dtype) == F(x * y) and rnd(F(x) + F(y), dtype) == F(x + y) and rnd(F(x) / F(y), dtype) == F(x / y)
        tiny = np.finfo(dtype).smallest_subnormal
        assert rnd(F(tiny) / 2, dtype) == 0 and rnd(F(tiny) * Fraction(3, 2), dtype) == 2 * F(tiny)      # ties to even, subnormal spacing


def _random_case(rng, size, halo, dtype):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)
    c, u, v = (rng.uniform(-1, 1, parent).astype(dtype) for _ in range(3))
    w = rng.uniform(-1, 1, (parent[0] + 1,) + plane).astype(dtype)
    dy, dx, az = (rng.uniform(0.5, 2, plane).astype(dtype) for _ in range(3))
    dz = rng.uniform(0.5, 2, Nz).astype(dtype)
    return c, u, v, w, dy, dx, az, dz


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("size,halo", [((4, 4, 3), (1, 1, 1)), ((6, 4, 2), (2, 1, 3))], ids=["4x4x3", "6x4x2"])
def test_reference_equals_the_rule_rounded_by_hand(size, halo, dtype):
    """every node of the fixed cases from the rule, one operation at a time, each exact result rounded once to the format: numpy's value is
    that number (a zero's sign is not held by a Fraction: the sign flip of the rule is checked on the device tests' bit comparison)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    c, u, v, w, dy, dx, az, dz = _random_case(np.random.default_rng([3, *size]), size, halo, dtype)
    F = lambda x: Fraction(float(x))
    R = lambda x: rnd(x, dtype)
    at = lambda a, i, j, k: F(a[k + Hz - 1, j + Hy - 1, i + Hx - 1])
    at2 = lambda a, i, j: F(a[j + Hy - 1, i + Hx - 1])
    half = Fraction(1, 2)
    Fx = lambda i, j, k: R(R(R(at2(dy, i, j) * F(dz[k - 1])) * at(u, i, j, k)) * R(half * R(at(c, i - 1, j, k) + at(c, i, j, k))))
    Fy = lambda i, j, k: R(R(R(at2(dx, i, j) * F(dz[k - 1])) * at(v, i, j, k)) * R(half * R(at(c, i, j - 1, k) + at(c, i, j, k))))
    Fz = lambda i, j, k: R(R(at2(az, i, j) * at(w, i, j, k)) * R(half * R(at(c, i, j, k - 1) + at(c, i, j, k))))
    got = interior_tendency(c, u, v, w, dy, dx, az, dz, size, halo)
    assert got.dtype == dtype and np.isfinite(got).all()
    for k in range(1, Nz + 1):
        for j in range(1, Ny + 1):
            for i in range(1, Nx + 1):
                V = R(at2(az, i, j) * F(dz[k - 1]))
                hx, hy, hz = R(Fx(i + 1, j, k) - Fx(i, j, k)), R(Fy(i, j + 1, k) - Fy(i, j, k)), R(Fz(i, j, k + 1) - Fz(i, j, k))
                want = -R(R(1 / V) * R(R(hx + hy) + hz))
                assert F(got[k - 1, j - 1, i - 1]) == want, (i, j, k)
    # the parent form: interior replaced, every halo cell keeps what it held
    G0 = np.full(c.shape, 7, dtype)
    out = tendency(c, u, v, w, G0, dy, dx, az, dz, size, halo)
    assert same_bits(out[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], got) == 0
    edge = np.ones(c.shape, bool)
    edge[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = False
    assert (out[edge] == 7).all() and edge.sum() == c.size - Nx * Ny * Nz and (G0 == 7).all()


def _exact_case(rng, size, halo, dtype):
    """small integer c, u, v, w with power-of-two metrics and spacings: every product, mean, difference and reciprocal of the rule is
    representable, so the reference computes the rule in exact arithmetic"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)
    dy, dx, az = (np.exp2(rng.integers(-3, 4, plane)).astype(dtype) for _ in range(3))
    dz = np.exp2(rng.integers(-2, 3, Nz)).astype(dtype)
    c, u, v = (rng.integers(-9, 10, parent).astype(dtype) for _ in range(3))
    w = rng.integers(-9, 10, (parent[0] + 1,) + plane).astype(dtype)
    return c, u, v, w, dy, dx, az, dz


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_telescoping_in_exact_rationals(dtype):
    """sum V G = -[(sum Fx[Nx+1] - sum Fx[1]) + (sum Fy[Ny+1] - sum Fy[1]) + (sum Fz[Nz+1] - sum Fz[1])]: the inner fluxes cancel in pairs"""
    size, halo = (6, 5, 3), (1, 2, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    c, u, v, w, dy, dx, az, dz = _exact_case(np.random.default_rng(5), size, halo, dtype)
    G = interior_tendency(c, u, v, w, dy, dx, az, dz, size, halo)
    F = lambda x: Fraction(float(x))
    at = lambda a, i, j, k: F(a[k + Hz - 1, j + Hy - 1, i + Hx - 1])
    at2 = lambda a, i, j: F(a[j + Hy - 1, i + Hx - 1])
    half = Fraction(1, 2)
    Fx = lambda i, j, k: at2(dy, i, j) * F(dz[k - 1]) * at(u, i, j, k) * half * (at(c, i - 1, j, k) + at(c, i, j, k))
    Fy = lambda i, j, k: at2(dx, i, j) * F(dz[k - 1]) * at(v, i, j, k) * half * (at(c, i, j - 1, k) + at(c, i, j, k))
    Fz = lambda i, j, k: at2(az, i, j) * at(w, i, j, k) * half * (at(c, i, j, k - 1) + at(c, i, j, k))
    I, J, K = range(1, Nx + 1), range(1, Ny + 1), range(1, Nz + 1)
    # the reference IS the exact rule on such data, node by node
    for k in K:
        for j in J:
            for i in I:
                V = at2(az, i, j) * F(dz[k - 1])
                want = -(1 / V) * ((Fx(i + 1, j, k) - Fx(i, j, k)) + (Fy(i, j + 1, k) - Fy(i, j, k)) + (Fz(i, j, k + 1) - Fz(i, j, k)))
                assert F(G[k - 1, j - 1, i - 1]) == want, (i, j, k)
    total = sum(at2(az, i, j) * F(dz[k - 1]) * F(G[k - 1, j - 1, i - 1]) for k in K for j in J for i in I)
    east = sum(Fx(Nx + 1, j, k) - Fx(1, j, k) for k in K for j in J)
    north = sum(Fy(i, Ny + 1, k) - Fy(i, 1, k) for k in K for i in I)
    top = sum(Fz(i, j, Nz + 1) - Fz(i, j, 1) for j in J for i in I)
    assert total == -(east + north + top) and total != 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_constant_tracer_with_w_from_the_exact_continuity_scan_has_no_tendency(dtype):
    """c constant everywhere and w the scan of the continuity equation on the same u, v and metrics: the three flux differences cancel node
    by node, G = 0 exactly"""
    size, halo = (6, 5, 3), (1, 2, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    c, u, v, w, dy, dx, az, dz = _exact_case(np.random.default_rng(6), size, halo, dtype)
    wi, div = interior_w_and_divergence(u, v, dy, dx, az, dz, size, halo)
    F = lambda x: Fraction(float(x))
    for j in range(Ny):                                            # the scan itself is exact on such data
        for i in range(Nx):
            assert F(wi[Nz, j, i]) == -sum(F(dz[k]) * F(div[k, j, i]) for k in range(Nz))
    w[...] = np.nan                                                # w's halo cells are not read
    w[Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx:Hx + Nx] = wi
    c[...] = 3
    G = interior_tendency(c, u, v, w, dy, dx, az, dz, size, halo)
    assert (div != 0).any() and all(F(x) == 0 for x in G.ravel())
    c[Hz + 1, Hy + 2, Hx + 3] = 4                                  # not constant: the identity does not hold by accident
    assert any(F(x) != 0 for x in interior_tendency(c, u, v, w, dy, dx, az, dz, size, halo).ravel())


def test_cells_read_are_tight():
    """cells_read is the stencil: a NaN in any one read cell reaches some output, NaN in every unread cell changes nothing"""
    size, halo = (4, 4, 3), (2, 2, 2)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    read = cells_read(size, halo)
    assert len(STENCIL) == 18 and set(read) == {"c", "u", "v", "w", "dy_fc", "dx_cf", "az_cc"}
    n3 = Nx * Ny * Nz
    assert read["c"].sum() == n3 + 2 * (Ny * Nz + Nx * Nz + Nx * Ny)                      # the interior and one layer on each of the six sides
    assert not read["c"][Hz - 1, Hy - 1, :].any() and not read["c"][Hz - 1, :, Hx - 1].any() and not read["c"][:, Hy - 1, Hx - 1].any()
    assert read["u"].sum() == Nz * Ny * (Nx + 1) and read["v"].sum() == Nz * (Ny + 1) * Nx and read["w"].sum() == (Nz + 1) * Ny * Nx
    assert read["w"].shape[0] == read["c"].shape[0] + 1 and read["w"][Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx:Hx + Nx].all()
    assert read["dy_fc"].sum() == Ny * (Nx + 1) and read["dx_cf"].sum() == (Ny + 1) * Nx and read["az_cc"].sum() == Ny * Nx
    c, u, v, w, dy, dx, az, dz = _random_case(np.random.default_rng(2), size, halo, np.float64)
    arrays = {"c": c, "u": u, "v": v, "w": w, "dy_fc": dy, "dx_cf": dx, "az_cc": az}
    call = lambda a: interior_tendency(a["c"], a["u"], a["v"], a["w"], a["dy_fc"], a["dx_cf"], a["az_cc"], dz, size, halo)
    want = call(arrays)
    F = lambda x: Fraction(float(x))
    poisoned = {k: np.where(read[k], a, np.nan) for k, a in arrays.items()}
    assert all(np.isnan(p).any() for p in poisoned.values())
    got = call(poisoned)
    assert not np.isnan(got).any() and all(F(g) == F(x) for g, x in zip(got.ravel(), want.ravel()))
    for name, a in arrays.items():
        for idx in zip(*np.nonzero(read[name])):
            one = dict(arrays)
            one[name] = a.copy()
            one[name][idx] = np.nan
            assert np.isnan(call(one)).any(), (name, idx)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_mask_levels(dtype):
    """the nodes k <= min(max(n, 0), Nz) hold the mask value converted once to the type: n < 0 and n = 0 mask nothing, n = Nz and n > Nz the
    whole column"""
    size, halo = (4, 4, 3), (1, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    c, u, v, w, dy, dx, az, dz = _random_case(np.random.default_rng(8), size, halo, dtype)
    raw = interior_tendency(c, u, v, w, dy, dx, az, dz, size, halo)
    n = np.zeros((Ny, Nx), np.int32)
    n[0, 0], n[0, 1], n[1, 2], n[2, 3], n[3, 3] = -2, 1, Nz, Nz + 4, 2
    G0 = np.full(c.shape, 7, dtype)
    out = tendency(c, u, v, w, G0, dy, dx, az, dz, size, halo, n_cc=n, mask_value=0.1)
    got = out[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    F = lambda x: Fraction(float(x))
    mv = F(dtype(0.1))
    assert mv != Fraction(1, 10)
    levels = {(0, 0): 0, (0, 1): 1, (1, 2): Nz, (2, 3): Nz, (3, 3): 2}
    for j in range(Ny):
        for i in range(Nx):
            m = levels.get((j, i), 0)
            for k in range(Nz):
                assert F(got[k, j, i]) == (mv if k < m else F(raw[k, j, i])), (i, j, k)
    edge = np.ones(c.shape, bool)
    edge[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = False
    assert (out[edge] == 7).all()
    assert same_bits(tendency(c, u, v, w, G0, dy, dx, az, dz, size, halo)[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx], raw) == 0
