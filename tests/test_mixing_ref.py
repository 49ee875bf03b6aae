"""tests/mixing_ref.py, the numpy statement of the rule of csrc/staged/tripolar_hip_mixing.h, held to properties that need no second
implementation (no GPU): what a stable and an inverted column get, the taper's shape, Ri against exact rational arithmetic, the cells read
(found by perturbing every cell of every input) against the header's list, mirror symmetry in x, the time average's rate, and -- together
with tests/vertical_diffusion_ref.py -- that an inverted pair of cells is mixed by the implicit step."""
from fractions import Fraction

import numpy as np
import pytest

import mixing_ref as R
import vertical_diffusion_ref as V
from mixing_cases import CA, F32, F64, MASK_VALUE, RI, SENTINEL, draw
from vorticity_ref import same_bits

SIZE, HALO = (6, 5, 4), (2, 2, 1)


def _interior(a, size=SIZE, halo=HALO):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return a[Hz:Hz + Nz + 1, Hy:Hy + Ny, Hx:Hx + Nx]


def _stable_b(dtype, size=SIZE, halo=HALO):
    """b that grows upwards in every column, halos included"""
    shape = R.cell_shape(size, halo)
    rng = np.random.default_rng(3)
    return np.cumsum(rng.uniform(0.1, 1, shape), axis=0).astype(dtype)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_a_stable_column_gets_the_background_values_on_every_evaluated_face(dtype):
    p, into = draw("ca", SIZE, HALO, dtype, nan_unread=False)
    p["b"] = _stable_b(dtype)
    out = R.reference(p, into)
    Nz = SIZE[2]
    for name, value in (("kappa_c", CA["background_kappa"]), ("nu_c", CA["background_nu"]), ("kappa_u", CA["background_nu"]), ("kappa_v", CA["background_nu"])):
        got = _interior(out[name])
        assert (got[1:Nz] == dtype(value)).all(), name
        assert (got[0] == 0).all() and (got[Nz] == 0).all(), name      # the closed faces
        halo = out[name].copy()
        _interior(halo)[...] = SENTINEL
        assert (halo == dtype(SENTINEL)).all(), name                   # no halo cell is written


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_one_inverted_pair_of_cells(dtype):
    """the convective value at exactly that face of kappa_c; the half-sum at exactly the two kappa_u nodes and the two kappa_v nodes beside it"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = SIZE, HALO
    p, into = draw("ca", SIZE, HALO, dtype, nan_unread=False)
    b = _stable_b(dtype)
    i, j, k = 3, 2, 3                                              # 1-based: the face k between the cells k - 1 and k of column (i, j)
    lo, hi = b[Hz + k - 2, Hy + j - 1, Hx + i - 1], b[Hz + k - 1, Hy + j - 1, Hx + i - 1]
    b[Hz + k - 2, Hy + j - 1, Hx + i - 1], b[Hz + k - 1, Hy + j - 1, Hx + i - 1] = hi, lo
    assert b[Hz + k, Hy + j - 1, Hx + i - 1] > hi and (k == 2 or b[Hz + k - 3, Hy + j - 1, Hx + i - 1] < lo)      # the faces around it stay stable
    p["b"] = b
    out = R.reference(p, into)
    T = dtype
    mixed = T(0.5) * (T(CA["background_nu"]) + T(CA["convective_nu"]))
    expect = {"kappa_c": ({(k, j, i): T(CA["convective_kappa"])}, T(CA["background_kappa"])),
              "nu_c": ({(k, j, i): T(CA["convective_nu"])}, T(CA["background_nu"])),
              "kappa_u": ({(k, j, i): mixed, (k, j, i + 1): mixed}, T(CA["background_nu"])),
              "kappa_v": ({(k, j, i): mixed, (k, j + 1, i): mixed}, T(CA["background_nu"]))}
    for name, (planted, background) in expect.items():
        want = np.full((Nz + 1, Ny, Nx), background, T)
        want[0] = want[Nz] = 0
        for (kk, jj, ii), value in planted.items():
            want[kk - 1, jj - 1, ii - 1] = value
        assert same_bits(np.ascontiguousarray(_interior(out[name])), want) == 0, name


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_the_taper_is_one_then_falls_to_zero(dtype):
    Ri0, delta = 0.1, 0.4
    Ri = np.concatenate([np.linspace(-5, 5, 2001), [Ri0, Ri0 + delta, -np.inf, np.inf, -0.0, 0.0]]).astype(dtype)
    Ri.sort()
    tau = R.taper(Ri, Ri0, delta)
    assert tau.dtype == dtype
    assert (tau[Ri <= dtype(Ri0)] == 1).all() and (tau[Ri >= dtype(Ri0) + dtype(delta)] == 0).all()
    assert (np.diff(tau) <= 0).all() and ((tau >= 0) & (tau <= 1)).all()
    between = (Ri > dtype(Ri0)) & (Ri < dtype(Ri0) + dtype(delta) * dtype(0.99))
    assert between.any() and ((tau[between] > 0) & (tau[between] < 1)).all()
    assert R.taper(np.array([np.nan], dtype), Ri0, delta)[0] == 1      # the header: a NaN Ri gives tau = one


def test_ri_on_linear_profiles_is_the_exact_rational_value_rounded_once_per_operation():
    """Float64: every operation of the rule redone in exact rational arithmetic on the operands the rule has at that point, and rounded once"""
    size, halo = (4, 3, 5), (1, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    p, _ = draw("ri", size, halo, F64, nan_unread=False)
    z = np.cumsum(np.r_[0.0, 1.0, p["dz_f"][1:Nz], 1.0])           # the planes' heights: the centres k - 1 and k lie dz_f[k] apart
    assert len(z) == Nz + 2 * Hz and z[Hz + 1] - z[Hz] == p["dz_f"][1]
    jj, ii = np.mgrid[0:Ny + 2 * Hy, 0:Nx + 2 * Hx]
    line = lambda slope, at: (at[None] + slope[None] * z.reshape(-1, 1, 1)).astype(F64)       # noqa: E731
    p["b"] = line(0.3 + 0.01 * ii + 0.02 * jj, 1.0 + 0.1 * ii)
    p["u"] = line(0.7 - 0.03 * ii + 0.01 * jj, 0.2 * jj)
    p["v"] = line(-0.4 + 0.02 * ii * jj, 0.5 + 0 * ii)
    N2, S2, Ri = R.richardson_of(p)
    rnd = lambda q: Fraction(float(q))                             # noqa: E731 -- float(Fraction) rounds correctly, once
    F = lambda x: Fraction(float(x))                               # noqa: E731 -- exact
    for kf in range(2, Nz + 1):
        for j in range(Ny):
            for i in range(Nx):
                dz = F(p["dz_f"][kf - 1])

                def dk(a, si=0, sj=0):
                    return rnd(rnd(F(a[Hz + kf - 1, Hy + j + sj, Hx + i + si]) - F(a[Hz + kf - 2, Hy + j + sj, Hx + i + si])) / dz)
                n2, du0, du1, dv0, dv1 = dk(p["b"]), dk(p["u"]), dk(p["u"], si=1), dk(p["v"]), dk(p["v"], sj=1)
                su = rnd(rnd(du0 * du0) + rnd(du1 * du1))
                sv = rnd(rnd(dv0 * dv0) + rnd(dv1 * dv1))
                s2 = rnd(rnd(su / 2) + rnd(sv / 2))
                want = Fraction(0) if n2 == 0 else rnd(n2 / s2)
                assert F(Ri[kf - 2, j, i]) == want and F(N2[kf - 2, j, i]) == n2 and F(S2[kf - 2, j, i]) == s2, (kf, j, i)
    # and it is what the profiles say: N2 / S2 of the slopes at the parent column (Hy, Hx).  A slope is a difference of values up to 16 in
    # size over a distance of at least 0.125, so each carries at most 16 eps / 0.125 = 128 eps; Ri has one in N2 and each twice in S2
    i0, j0 = Hx, Hy
    slope_b, slope_u0, slope_u1 = 0.3 + 0.01 * i0 + 0.02 * j0, 0.7 - 0.03 * i0 + 0.01 * j0, 0.7 - 0.03 * (i0 + 1) + 0.01 * j0
    slope_v0, slope_v1 = -0.4 + 0.02 * i0 * j0, -0.4 + 0.02 * i0 * (j0 + 1)
    exact = slope_b / (0.5 * (slope_u0 ** 2 + slope_u1 ** 2) + 0.5 * (slope_v0 ** 2 + slope_v1 ** 2))
    assert np.abs(p["b"]).max() < 16 and np.abs(p["u"]).max() < 16 and np.abs(p["v"]).max() < 16
    assert abs(Ri[1, 0, 0] - exact) <= 5 * 128 * np.finfo(F64).eps * abs(exact)


@pytest.mark.parametrize("closure,prev", [("ca", False), ("ri", False), ("ri", True)], ids=["ca", "ri", "ri-prev"])
@pytest.mark.parametrize("outputs", [("kappa_c",), ("nu_c",), ("kappa_u",), ("kappa_v",), R.OUTPUTS], ids=lambda o: "+".join(o))
def test_the_cells_read_are_the_headers_list(closure, prev, outputs):
    """every cell of every input, halo cells included, is set to +1000 and to -1000: an output changes iff the header lists the cell.  The
    taper is kept in its linear range so that every cell read shows"""
    size, halo = (4, 3, 3), (2, 2, 1)
    params = dict(RI, Ri0=-1e6, Ri_delta=2e6) if closure == "ri" else None
    p, into = draw(closure, size, halo, F64, prev=prev, outputs=outputs, params=params, nan_unread=False)
    base = R.reference(p, into)
    if closure == "ri":
        tau = R.taper(R.richardson_of(p)[2], -1e6, 2e6)
        assert ((tau > 0) & (tau < 1)).all()
    listed = R.cells_read(p)
    arrays = {"b": p["b"], "u": p["u"], "v": p["v"]}
    if p["prev"] is not None:
        arrays.update(kappa_c_prev=p["prev"][0], nu_c_prev=p["prev"][1])
    for name, a in arrays.items():
        if a is None:
            continue
        found = np.zeros(a.shape, bool)
        for at in np.ndindex(a.shape):
            for value in (1000.0, -1000.0):
                changed = a.copy()
                changed[at] = value
                q = dict(p)
                if name.endswith("_prev"):
                    q["prev"] = tuple(changed if n == name else x for n, x in zip(("kappa_c_prev", "nu_c_prev"), p["prev"]))
                else:
                    q[name] = changed
                out = R.reference(q, into)
                if any(same_bits(out[o], base[o]) for o in outputs):
                    found[at] = True
                    break
        assert (found == listed[name]).all(), (name, np.argwhere(found != listed[name])[:8])
    for o in outputs:                                              # and no halo cell of an output is written
        halo_cells = base[o].copy()
        _interior(halo_cells, size, halo)[...] = SENTINEL
        assert (halo_cells == SENTINEL).all()


@pytest.mark.parametrize("closure", ["ca", "ri"])
def test_mirror_symmetry_in_x(closure):
    """the arrays mirrored in x (cells i -> Nx + 1 - i, x-faces i -> Nx + 2 - i) give the mirrored diffusivities, bit for bit"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = SIZE, HALO
    p, into = draw(closure, SIZE, HALO, F64, prev=closure == "ri", nan_unread=False)
    cells = lambda a: None if a is None else np.ascontiguousarray(a[..., ::-1])                     # noqa: E731
    xfaces = lambda a: None if a is None else np.ascontiguousarray(np.roll(a[..., ::-1], 1, axis=-1))   # noqa: E731
    q = dict(p, b=cells(p["b"]), u=xfaces(p["u"]), v=cells(p["v"]), prev=None if p["prev"] is None else tuple(cells(a) for a in p["prev"]))
    out, mirrored = R.reference(p, into), R.reference(q, into)
    for name in ("kappa_c", "nu_c", "kappa_v"):
        assert same_bits(np.ascontiguousarray(_interior(mirrored[name])), np.ascontiguousarray(_interior(out[name])[..., ::-1])) == 0, name
    got, want = _interior(mirrored["kappa_u"]), _interior(out["kappa_u"])
    assert same_bits(np.ascontiguousarray(got[..., 1:]), np.ascontiguousarray(want[..., :0:-1])) == 0      # the faces i = 2..Nx


def test_the_time_average_approaches_the_instantaneous_value_at_its_rate():
    """steady inputs: nu_i - nu_n = Cav / (1 + Cav) * (nu_i - nu_(n-1)) per call, to the three roundings of a call (bound: 8 eps |nu_i|)"""
    p, into = draw("ri", SIZE, HALO, F64, prev=True, nan_unread=False)
    Nz = SIZE[2]
    instant = R.reference(dict(p, prev=None), into)
    rate = RI["Cav"] / (1 + RI["Cav"])
    eps = np.finfo(F64).eps
    old = {k: _interior(a)[1:Nz].copy() for k, a in zip(("kappa_c", "nu_c"), p["prev"])}
    for n in range(12):
        out = R.reference(p, into)
        for name in ("kappa_c", "nu_c"):
            target, new = _interior(instant[name])[1:Nz], _interior(out[name])[1:Nz]
            scale = np.maximum(np.abs(target), np.abs(old[name]))
            assert (np.abs((target - new) - rate * (target - old[name])) <= 8 * eps * scale).all(), (n, name)
            old[name] = new.copy()
        # ping-pong: the outputs become the previous values; the halos keep the drawn values, which only the neighbour outputs read
        p = dict(p, prev=tuple(np.where(out[k] == SENTINEL, q, out[k]) for k, q in zip(("kappa_c", "nu_c"), p["prev"])))
    for name in ("kappa_c", "nu_c"):
        target = _interior(instant[name])[1:Nz]
        assert (np.abs(target - old[name]) <= rate ** 12 * 2.2 + 64 * eps).all()       # previous values in [0, 2], instantaneous ones in [0, 2.2]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_an_inverted_pair_is_mixed_by_the_implicit_step(dtype):
    """a two-level inverted column, kappa_conv dt / dz^2 = 100, zero background, through vertical_diffusion_ref: |b2 - b1| falls to 1/201 of
    its start (below 1 %), and the column sum is kept within 4 eps (|b1| + |b2|)"""
    size, halo = (2, 1, 2), (1, 1, 1)
    T = dtype
    b = np.zeros(R.cell_shape(size, halo), T)
    b[1], b[2] = T(1.75), T(-0.625)                                # heavy over light, every column and halo cell
    dz_f = np.array([np.nan, 0.5, np.nan], T)
    dz_c = np.array([0.5, 0.5], T)
    dt = T(0.125)
    kconv = 100 * 0.5 * 0.5 / 0.125
    p = R.problem("ca", size, halo, b, dz_f, dict(background_kappa=0.0, convective_kappa=kconv, background_nu=0.0, convective_nu=0.0))
    out = R.reference(p, {k: np.full(R.face_shape(size, halo), SENTINEL, T) for k in R.OUTPUTS})
    kappa = out["kappa_c"][1:4, 1, 1]                              # the faces 1, 2, 3 of column (1, 1)
    assert kappa[1] == T(kconv) and kappa[0] == 0 and kappa[2] == 0
    col = b[1:3, 1, 1]
    new = V.solve_column(col.copy(), kappa.copy(), dz_c, np.array([np.nan, 0.5, np.nan], T), dt)
    assert new.dtype == T
    start, end = abs(float(col[1]) - float(col[0])), abs(float(new[1]) - float(new[0]))
    assert end < 0.01 * start
    assert abs(end / start - 1 / 201) <= 64 * np.finfo(T).eps      # the exact factor of one backward-Euler step: 1 / (1 + 2 * 100)
    assert abs((float(new[0]) + float(new[1])) - (float(col[0]) + float(col[1]))) <= 4 * np.finfo(T).eps * (abs(float(col[0])) + abs(float(col[1])))
    # the stable column is left alone: zero background
    calm = R.reference(dict(p, b=np.ascontiguousarray(b[::-1])), {k: np.full(R.face_shape(size, halo), SENTINEL, T) for k in R.OUTPUTS})
    assert (calm["kappa_c"][1:4, 1, 1] == 0).all() and MASK_VALUE != 0
