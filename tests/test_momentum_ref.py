"""The numpy reference of the momentum advection tendency (tests/momentum_ref.py) held without a device, every check in Python Fractions:
against the rule evaluated node by node with every intermediate rounded by hand, against vorticity_ref, against identities in exact
rationals on data whose every intermediate is representable, and its stencil and mask."""
from fractions import Fraction

import numpy as np
import pytest

from momentum_ref import METRICS, STENCIL, STENCIL_U, STENCIL_V, cells_read, interior_tendencies, same_bits, tendencies, terms, zeta
from test_advection_ref import rnd
from vorticity_ref import interior_vorticity

F = lambda x: Fraction(float(x))                                   # noqa: E731


def _shapes(size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Nz + 1 + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)


def _random_case(rng, size, halo, dtype):
    parent, wparent, plane = _shapes(size, halo)
    u, v = (rng.uniform(-1, 1, parent).astype(dtype) for _ in range(2))
    w = rng.uniform(-1, 1, wparent).astype(dtype)
    m = {k: rng.uniform(0.5, 2, plane).astype(dtype) for k in METRICS}
    dz = rng.uniform(0.5, 2, size[2] + 1).astype(dtype)
    return u, v, w, m, dz


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("size,halo", [((4, 4, 3), (1, 1, 1)), ((6, 4, 2), (2, 1, 3))], ids=["4x4x3", "6x4x2"])
def test_reference_equals_the_rule_rounded_by_hand(size, halo, dtype):
    """every node of the fixed cases from the rule, one operation at a time, each exact result rounded once to the format: numpy's value is
    that number (a zero's sign is not held by a Fraction: the sign flips of the rule are checked on the device tests' bit comparison)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    u, v, w, m, dz = _random_case(np.random.default_rng([3, *size]), size, halo, dtype)
    R = lambda x: rnd(x, dtype)                                    # noqa: E731
    at = lambda a, i, j, k: F(a[k + Hz - 1, j + Hy - 1, i + Hx - 1])   # noqa: E731
    M = lambda name, i, j: F(m[name][j + Hy - 1, i + Hx - 1])      # noqa: E731
    h = Fraction(1, 2)
    D = lambda kf: F(dz[kf - 1])                                   # noqa: E731
    Z = lambda i, j, k: R(R(R(R(M("dy_cf", i, j) * at(v, i, j, k)) - R(M("dy_cf", i - 1, j) * at(v, i - 1, j, k)))                         # noqa: E731
                            - R(R(M("dx_fc", i, j) * at(u, i, j, k)) - R(M("dx_fc", i, j - 1) * at(u, i, j - 1, k)))) / M("az_ff", i, j))
    P = lambda i, j, k: R(M("dx_cf", i, j) * at(v, i, j, k))       # noqa: E731
    Q = lambda i, j, k: R(M("dy_fc", i, j) * at(u, i, j, k))       # noqa: E731
    A = lambda i, j, kf: R(M("az_cc", i, j) * at(w, i, j, kf))     # noqa: E731
    sq = lambda a, i, j, k: R(at(a, i, j, k) * at(a, i, j, k))     # noqa: E731
    K = lambda i, j, k: R(h * R(R(h * R(sq(u, i, j, k) + sq(u, i + 1, j, k))) + R(h * R(sq(v, i, j, k) + sq(v, i, j + 1, k)))))           # noqa: E731
    S = lambda i, j, kf: R(R(h * R(A(i - 1, j, kf) + A(i, j, kf))) * R(R(at(u, i, j, kf) - at(u, i, j, kf - 1)) / D(kf)))                 # noqa: E731
    Rr = lambda i, j, kf: R(R(h * R(A(i, j - 1, kf) + A(i, j, kf))) * R(R(at(v, i, j, kf) - at(v, i, j, kf - 1)) / D(kf)))                # noqa: E731
    got = terms(u, v, w, m, dz, size, halo)
    assert all(a.dtype == dtype and np.isfinite(a).all() for a in got.values())
    for k in range(1, Nz + 1):
        for j in range(1, Ny + 1):
            for i in range(1, Nx + 1):
                zb = R(h * R(Z(i, j, k) + Z(i, j + 1, k)))
                vh = R(h * R(R(h * R(P(i - 1, j, k) + P(i - 1, j + 1, k))) + R(h * R(P(i, j, k) + P(i, j + 1, k)))))
                hu = -R(R(zb * vh) / M("dx_fc", i, j))
                bu = R(R(K(i, j, k) - K(i - 1, j, k)) / M("dx_fc", i, j))
                vu = R(R(h * R(S(i, j, k) + S(i, j, k + 1))) / M("az_fc", i, j))
                Gu = -R(R(hu + vu) + bu)
                zb = R(h * R(Z(i, j, k) + Z(i + 1, j, k)))
                uh = R(h * R(R(h * R(Q(i, j - 1, k) + Q(i + 1, j - 1, k))) + R(h * R(Q(i, j, k) + Q(i + 1, j, k)))))
                hv = R(R(zb * uh) / M("dy_cf", i, j))
                bv = R(R(K(i, j, k) - K(i, j - 1, k)) / M("dy_cf", i, j))
                vv = R(R(h * R(Rr(i, j, k) + Rr(i, j, k + 1))) / M("az_cf", i, j))
                Gv = -R(R(hv + vv) + bv)
                want = dict(hu=hu, vu=vu, bu=bu, Gu=Gu, hv=hv, vv=vv, bv=bv, Gv=Gv)
                for name, x in want.items():
                    assert F(got[name][k - 1, j - 1, i - 1]) == x, (name, i, j, k)
    # the parent form: interiors replaced, every halo cell keeps what it held
    G0 = np.full(u.shape, 7, dtype)
    Gu, Gv = tendencies(u, v, w, G0, G0, m, dz, size, halo)
    cut = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    assert same_bits(Gu[cut], got["Gu"]) == 0 and same_bits(Gv[cut], got["Gv"]) == 0
    a, b = interior_tendencies(u, v, w, m, dz, size, halo)
    assert same_bits(a, got["Gu"]) == 0 and same_bits(b, got["Gv"]) == 0 and same_bits(a, b) > 0
    edge = np.ones(u.shape, bool)
    edge[cut] = False
    assert (Gu[edge] == 7).all() and (Gv[edge] == 7).all() and edge.sum() == u.size - Nx * Ny * Nz and (G0 == 7).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_rules_vorticity_is_vorticity_refs(dtype):
    size, halo = (6, 4, 2), (2, 1, 3)
    u, v, w, m, dz = _random_case(np.random.default_rng(4), size, halo, dtype)
    assert same_bits(zeta(u, v, m, size, halo), interior_vorticity(u, v, m["dx_fc"], m["dy_cf"], m["az_ff"], size, halo)) == 0


def _exact_case(rng, size, halo, dtype):
    """small integer u, v, w with power-of-two metrics and spacings: every product, mean, difference and quotient of the rule is
    representable, so the reference computes the rule in exact arithmetic"""
    parent, wparent, plane = _shapes(size, halo)
    m = {k: np.exp2(rng.integers(-3, 4, plane)).astype(dtype) for k in METRICS}
    dz = np.exp2(rng.integers(-2, 3, size[2] + 1)).astype(dtype)
    u, v = (rng.integers(-9, 10, parent).astype(dtype) for _ in range(2))
    w = rng.integers(-9, 10, wparent).astype(dtype)
    return u, v, w, m, dz


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_identities_in_exact_rationals(dtype):
    size, halo = (6, 5, 3), (1, 2, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    u, v, w, m, dz = _exact_case(np.random.default_rng(5), size, halo, dtype)
    # periodic x halos: column 0 is column Nx, column Nx + 1 is column 1
    for a in (u, v, w, *m.values()):
        a[..., Hx - 1] = a[..., Hx + Nx - 1]
        a[..., Hx + Nx] = a[..., Hx]
    t = terms(u, v, w, m, dz, size, halo)
    # the reference IS the exact rule on such data: bu against K in rationals, node by node
    at = lambda a, i, j, k: F(a[k + Hz - 1, j + Hy - 1, i + Hx - 1])   # noqa: E731
    K = lambda i, j, k: (at(u, i, j, k) ** 2 + at(u, i + 1, j, k) ** 2 + at(v, i, j, k) ** 2 + at(v, i, j + 1, k) ** 2) / 4              # noqa: E731
    dx = lambda i, j: F(m["dx_fc"][j + Hy - 1, i + Hx - 1])        # noqa: E731
    for k in range(1, Nz + 1):
        for j in range(1, Ny + 1):
            for i in range(1, Nx + 1):
                assert F(t["bu"][k - 1, j - 1, i - 1]) == (K(i, j, k) - K(i - 1, j, k)) / dx(i, j), (i, j, k)
            # the gradient of K telescopes around a periodic row: sum_i dx_fc * bu = 0
            assert sum(dx(i, j) * F(t["bu"][k - 1, j - 1, i - 1]) for i in range(1, Nx + 1)) == 0
    assert (t["bu"] != 0).any()
    # u, v uniform and w = 0: no vorticity, no KE gradient, no vertical term -- zero everywhere
    u1, v1, w0 = np.full_like(u, 3), np.full_like(v, -2), np.zeros_like(w)
    one = {k: np.ones_like(a) for k, a in m.items()}               # uniform metrics: a uniform flow is irrotational on them
    t = terms(u1, v1, w0, one, dz, size, halo)
    assert all((a == 0).all() for a in t.values())
    # u, v constant in z: vu = vv = +-0 whatever w is
    uz, vz = np.broadcast_to(u[:1], u.shape).copy(), np.broadcast_to(v[:1], v.shape).copy()
    t = terms(uz, vz, w, m, dz, size, halo)
    assert (t["vu"] == 0).all() and (t["vv"] == 0).all() and (t["hu"] != 0).any() and (t["bv"] != 0).any()
    assert (terms(u, v, w, m, dz, size, halo)["vu"] != 0).any()


def test_cells_read_are_tight():
    """cells_read is the stencil: a NaN in any one read cell reaches some output, NaN in every unread cell changes nothing"""
    size, halo = (4, 4, 3), (2, 2, 2)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    read = cells_read(size, halo)
    assert set(read) == {"u", "v", "w", *METRICS}
    offsets = lambda st, name: {(di, dj, dk) for n, di, dj, dk in st if n == name}                   # noqa: E731
    assert offsets(STENCIL, "u") == {(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (1, -1, 0), (0, 0, 1), (0, 0, -1)}
    assert offsets(STENCIL, "v") == {(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (-1, 1, 0), (0, 0, 1), (0, 0, -1)}
    assert offsets(STENCIL, "w") == {(0, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, 1), (-1, 0, 1), (0, -1, 1)}
    assert set(STENCIL) == set(STENCIL_U) | set(STENCIL_V)
    # the two corner halo cells, and w's west column and south row
    assert read["u"][Hz, Hy - 1, Hx + Nx] and read["v"][Hz, Hy + Ny, Hx - 1]
    assert not read["u"][Hz, Hy - 1, Hx - 1] and not read["u"][Hz, Hy + Ny, Hx + Nx] and not read["v"][Hz, Hy - 1, Hx + Nx]
    assert read["w"][Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx - 1].all() and read["w"][Hz:Hz + Nz + 1, Hy - 1, Hx:Hx + Nx].all()
    assert not read["w"][Hz, Hy - 1, Hx - 1] and not read["w"][Hz - 1].any() and not read["w"][Hz + Nz + 1].any()
    assert read["w"].sum() == (Nz + 1) * (Nx * Ny + Nx + Ny)
    assert read["u"][Hz - 1].sum() == Nx * Ny == read["u"][Hz + Nz].sum() and not read["u"][Hz - 2].any()
    assert read["u"][Hz].sum() == (Nx + 2) * (Ny + 2) - 3 == read["v"][Hz].sum()          # one corner of the four each
    assert read["az_fc"].sum() == Nx * Ny == read["az_cf"].sum() and read["az_cc"].sum() == Nx * Ny + Nx + Ny
    u, v, w, m, dz = _random_case(np.random.default_rng(2), size, halo, np.float64)
    arrays = {"u": u, "v": v, "w": w, **m}
    call = lambda a: np.stack(interior_tendencies(a["u"], a["v"], a["w"], {k: a[k] for k in METRICS}, dz, size, halo))       # noqa: E731
    want = call(arrays)
    poisoned = {k: np.where(read[k], a, np.nan) for k, a in arrays.items()}
    assert all(np.isnan(p).any() for p in poisoned.values())
    got = call(poisoned)
    assert not np.isnan(got).any() and same_bits(got, want) == 0
    for name, a in arrays.items():
        for idx in zip(*np.nonzero(read[name])):
            one = dict(arrays)
            one[name] = a.copy()
            one[name][idx] = np.nan
            assert np.isnan(call(one)).any(), (name, idx)
    for kf in range(Nz + 1):
        d1 = dz.copy()
        d1[kf] = np.nan
        assert np.isnan(np.stack(interior_tendencies(u, v, w, m, d1, size, halo))).any(), kf


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_mask_levels(dtype):
    """the nodes k <= min(max(n, 0), Nz) hold the mask value converted once to the type: n < 0 and n = 0 mask nothing, n = Nz and n > Nz the
    whole column; Gu goes by n_fc, Gv by n_cf"""
    size, halo = (4, 4, 3), (1, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    u, v, w, m, dz = _random_case(np.random.default_rng(8), size, halo, dtype)
    raw = interior_tendencies(u, v, w, m, dz, size, halo)
    nfc, ncf = np.zeros((Ny, Nx), np.int32), np.zeros((Ny, Nx), np.int32)
    nfc[0, 0], nfc[0, 1], nfc[1, 2], nfc[2, 3], nfc[3, 3] = -2, 1, Nz, Nz + 4, 2
    ncf[1, 1], ncf[0, 1], ncf[2, 2], ncf[3, 0], ncf[3, 3] = -7, 2, Nz, Nz + 1, 1
    levels = ({(0, 0): 0, (0, 1): 1, (1, 2): Nz, (2, 3): Nz, (3, 3): 2}, {(1, 1): 0, (0, 1): 2, (2, 2): Nz, (3, 0): Nz, (3, 3): 1})
    G0 = np.full(u.shape, 7, dtype)
    out = tendencies(u, v, w, G0, G0, m, dz, size, halo, n_fc=nfc, n_cf=ncf, mask_value=0.1)
    mv = F(dtype(0.1))
    assert mv != Fraction(1, 10)
    cut = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    edge = np.ones(u.shape, bool)
    edge[cut] = False
    for parent, r, lv in zip(out, raw, levels):
        got = parent[cut]
        for j in range(Ny):
            for i in range(Nx):
                for k in range(Nz):
                    assert F(got[k, j, i]) == (mv if k < lv.get((j, i), 0) else F(r[k, j, i])), (i, j, k)
        assert (parent[edge] == 7).all()
    plain = tendencies(u, v, w, G0, G0, m, dz, size, halo)
    assert same_bits(plain[0][cut], raw[0]) == 0 and same_bits(plain[1][cut], raw[1]) == 0
    with pytest.raises(AssertionError):
        tendencies(u, v, w, G0, G0, m, dz, size, halo, n_fc=nfc)
