"""CPU checks of the oracle's geometry utilities: the non-orthogonality diagnostic of
test/test_tripolar_grid.jl:8-34,49-75 and the frame rotation of examples/convert_to_latlong_frame.jl:12-55.

The reference bounds the tripolar grid's angle by the range found on a conformal cubed-sphere panel (:74-75); the cubed
sphere is Oceananigans' (absent here), so that bound is replaced by a stated one and is "parity unpinned": what IS
checked against reference-held facts is the test's set-up (1-degree grid, poles 35N / 75E, mask of :59-60) and the
properties the example relies on (the two conversions are inverse rotations; a zonal unit vector stays a unit vector)."""
import functools

import mpmath as mp
import numpy as np
import pytest

import geometry_ref as R


def _masked_setup(oracle):
    size, halo = (360, 180, 1), (4, 4, 4)
    g = oracle.build_grid(size, halo=halo, first_pole_longitude=75, north_poles_latitude=35)     # :52-57
    lam = g["lambda_cc"][4:-4, 4:-4]; phi = g["phi_cc"][4:-4, 4:-4]
    l1, pp = 75.0, 35.0
    l2 = l1 + 180
    mask = ((np.abs(lam - l1) < 5) & (np.abs(pp - phi) < 5)) | ((np.abs(lam - l2) < 5) & (np.abs(pp - phi) < 5)) | (phi < -78)   # :59-60
    return size, halo, g, mask


def test_acos_restatement_against_mpmath(oracle):
    mp.mp.dps = 40
    x = np.concatenate([np.linspace(-1, 1, 2001), np.random.default_rng(1).uniform(-1, 1, 4000), [1e-20, -1e-20, 0.5, -0.5, 0.4999999, 0.975]])
    y = oracle.math_probe("acos", x)
    worst = 0.0
    for a, b in zip(x, y):
        e = mp.acos(mp.mpf(float(a)))
        ulp = np.spacing(abs(float(e))) if e != 0 else 1.0
        worst = max(worst, abs(float((mp.mpf(float(b)) - e) / ulp)))
    assert worst < 1.0, worst                       # msun acos: < 1 ulp


def test_tripolar_grid_is_orthogonal_away_from_the_singularities(oracle):
    size, halo, g, mask = _masked_setup(oracle)
    ang = oracle.nonorthogonality_angle(g["lambda_ff"], g["phi_ff"], size, halo, immersed=mask)
    assert ang.shape == (180, 360)
    assert np.all(ang[-1] == 0) and np.all(ang[:, -1] == 0)          # outside the (Nx-1, Ny-1) launch (:70)
    assert np.all(ang[mask] == 0)                                     # immersed -> pi/2 - pi/2 (:29)
    # builder-stated bound (the reference's is the cubed-sphere panel range, :74-75: parity unpinned)
    assert ang.max() < 2.0 and ang.min() > -2.0, (ang.min(), ang.max())
    # unmasked, the three singular neighbourhoods are NOT orthogonal: the diagnostic must see them
    raw = oracle.nonorthogonality_angle(g["lambda_ff"], g["phi_ff"], size, halo)
    assert np.abs(raw).max() > 10.0


def test_nonorthogonality_against_mpmath_on_sample_nodes(oracle):
    """the angle formula re-evaluated with 40 digits from the stored Float64 coordinates"""
    mp.mp.dps = 40
    size, halo = (60, 30, 1), (4, 4, 4)
    g = oracle.build_grid(size, halo=halo)
    ang = oracle.nonorthogonality_angle(g["lambda_ff"], g["phi_ff"], size, halo)
    def P(i, j):
        l = mp.radians(mp.mpf(float(g["lambda_ff"][j + 3, i + 3]))); p = mp.radians(mp.mpf(float(g["phi_ff"][j + 3, i + 3])))
        return mp.matrix([mp.cos(l) * mp.cos(p), mp.sin(l) * mp.cos(p), mp.sin(p)])
    for i, j in ((5, 5), (30, 20), (17, 28), (59, 29), (1, 1), (31, 29)):
        p0, p1, p2 = P(i, j), P(i + 1, j), P(i, j + 1)
        v1, v2 = p1 - p0, p2 - p0
        c = (v1.T * v2)[0] / (mp.norm(v1) * mp.norm(v2))
        want = mp.degrees(mp.acos(c) - mp.pi / 2)
        assert abs(float(want) - ang[j - 1, i - 1]) < 1e-9, (i, j, float(want), ang[j - 1, i - 1])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_frame_conversions_round_trip(oracle, dtype):
    size, halo = (180, 90, 2), (4, 4, 4)                                                  # the example's grid (:58)
    g = oracle.build_grid(size, dtype=dtype, halo=halo, north_poles_latitude=35)
    rng = np.random.default_rng(3)
    shape = (2 + 8, 90 + 8, 180 + 8)
    u = rng.uniform(-1, 1, shape).astype(dtype); v = rng.uniform(-1, 1, shape).astype(dtype)
    ul, vl = oracle.convert_frame(g, u, v, size, halo, to_native=False)
    ub, vb = oracle.convert_frame(g, ul, vl, size, halo, to_native=True)
    I = (slice(4, -4), slice(4, -4), slice(4, -4))
    tol = 1e-13 if dtype == np.float64 else 1e-5
    # the example's "native" conversion (:54) returns (u d1 + v d2, u d2 - v d1): the inverse rotation with the SECOND
    # component negated -- kept as written in the reference, so a round trip gives (u, -v)
    assert np.max(np.abs(ub[I] - u[I])) < tol and np.max(np.abs(vb[I] + v[I])) < tol
    speed2 = u[I].astype(np.float64) ** 2 + v[I].astype(np.float64) ** 2
    assert np.max(np.abs(ul[I].astype(np.float64) ** 2 + vl[I].astype(np.float64) ** 2 - speed2)) < 10 * tol   # norm kept
    assert np.all(ul[0] == 0) and np.all(ul[:, :4] == 0)                                   # only the interior is written
    # purely zonal unit flow (:64): far from the northern poles the grid lines are nearly parallels and meridians, so the
    # rotation is nearly the identity (d1 -> 1, d2 -> 0); it stays a unit vector everywhere
    one = np.ones(shape, dtype=dtype); zero = np.zeros(shape, dtype=dtype)
    uz, vz = oracle.convert_frame(g, one, zero, size, halo, to_native=True)
    assert np.max(np.abs(uz[4:-4, 4:10, 4:-4] - 1)) < 1e-4 and np.max(np.abs(vz[4:-4, 4:10, 4:-4])) < 5e-3
    assert np.max(np.abs(uz[I].astype(np.float64) ** 2 + vz[I].astype(np.float64) ** 2 - 1)) < 10 * tol


# ---- the oracle held to tests/geometry_ref.py (written from the reference's Julia text, long double) on WHOLE arrays, at every shape the GPU
# ---- tests use: validates the reference and its tolerances without a device


@functools.lru_cache(maxsize=None)
def _grid(oracle, nx, ny, halo, dtype):
    return oracle.build_grid((nx, ny, 1), dtype=dtype, halo=halo)


def _mpf(x):
    """a long double (or a double) as an mpf, exactly"""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - hi)) if np.isfinite(hi) else mp.mpf(hi)


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("halo", R.ANGLE_HALOS, ids=lambda h: "h%d%d%d" % h)
@pytest.mark.parametrize("size", R.ANGLE_SIZES, ids=lambda s: "%dx%d" % s)
def test_oracle_angle_against_the_reference(oracle, size, halo, dtype):
    g = _grid(oracle, *size, halo, dtype)
    for mask in (None, R.angle_mask(size)):
        got = oracle.nonorthogonality_angle(g["lambda_ff"], g["phi_ff"], (*size, 1), halo, immersed=mask)
        want, tol, valid = R.angle_ref(g["lambda_ff"], g["phi_ff"], (*size, 1), halo, immersed=mask)
        excluded = ~valid
        assert np.array_equal(excluded, ~valid | np.isnan(got)), "a NaN of the oracle on a node the reference calls valid"
        assert excluded.sum() <= 0.01 * (size[0] - 1) * (size[1] - 1), excluded.sum()
        err = np.abs(got - want)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = float(np.max(np.where(valid & (tol > 0), err / tol, 0)))
        assert np.all(err[valid] <= tol[valid]), f"worst error / tol = {ratio:.3f}"
        assert np.all(got[-1] == 0) and np.all(got[:, -1] == 0) and (mask is None or np.all(got[mask != 0] == 0))
        assert ratio < 1, ratio


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("geom", R.FRAME_GEOMS, ids=lambda g: "%dx%d-h%d%d%d" % (*g[0], *g[1]))
def test_oracle_frame_against_the_reference(oracle, geom, dtype):
    (nx, ny), halo = geom
    g = _grid(oracle, nx, ny, halo, dtype)
    worst = 0.0
    for nz in R.frame_levels(geom):
        size = (nx, ny, nz)
        u, v = R.frame_inputs(size, halo, dtype)
        I = tuple(slice(h, h + n) for h, n in zip(halo[::-1], size[::-1]))
        for to_native in (False, True):
            gu, gv = oracle.convert_frame(g, u, v, size, halo, to_native=to_native)
            wu, wv, scale = R.frame_ref(g, u, v, size, halo, to_native)
            tol = R.frame_tolerance(scale, dtype)
            for got, want in ((gu[I], wu), (gv[I], wv)):
                fin = np.isfinite(want)
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isfinite(got), fin)
                assert (~fin).reshape(nz, -1).sum(1).max() <= (2 if nx % 4 == 2 else 0)
                err = np.abs(got[fin] - want[fin])
                worst = max(worst, float(np.max(err / tol[fin])))
                assert np.all(err <= tol[fin]), f"worst error / tol = {worst:.3f} (to_native = {to_native}, Nz = {nz})"
    assert worst < 1, worst


def test_reference_against_mpmath_on_sampled_nodes_and_cells(oracle):
    """tests/geometry_ref.py itself, pinned to 40 digits: the formulas below are typed from test/test_tripolar_grid.jl:12-32 and
    examples/convert_to_latlong_frame.jl:14-31,54 with Julia's 1-based (i, j).  Long double has 11 more bits than the Float64 the tolerances
    are sized for, so the reference must sit within tol / 1024 (2^-11 of the bound is tol / 5700)."""
    mp.mp.dps = 40
    rad = lambda x: _mpf(x) * mp.pi / 180
    rng = np.random.default_rng(5)
    for (nx, ny), halo, dtype in (((62, 7), (4, 4, 4), np.float64), ((130, 36), (5, 5, 5), np.float32), ((128, 15), (1, 1, 1), np.float64)):
        g = _grid(oracle, nx, ny, halo, dtype)
        Hx, Hy = halo[:2]
        ang, tol, valid = R.angle_ref(g["lambda_ff"], g["phi_ff"], (nx, ny, 1), halo)
        assert valid.all()

        def P(i, j):
            l, p = rad(g["lambda_ff"][j + Hy - 1, i + Hx - 1]), rad(g["phi_ff"][j + Hy - 1, i + Hx - 1])
            return mp.matrix([mp.cos(l) * mp.cos(p), mp.sin(l) * mp.cos(p), mp.sin(p)])
        nodes = [(1, 1), (nx - 1, ny - 1), (nx // 2, ny - 1), (nx // 2 + 1, ny - 1), (min(63, nx - 1), min(7, ny - 1)), (1, ny - 1)]
        nodes += [(int(rng.integers(1, nx)), int(rng.integers(1, ny))) for _ in range(10)]
        for i, j in nodes:
            v1, v2 = P(i + 1, j) - P(i, j), P(i, j + 1) - P(i, j)
            want = mp.degrees(mp.acos((v1.T * v2)[0] / (mp.norm(v1) * mp.norm(v2))) - mp.pi / 2)
            assert abs(_mpf(ang[j - 1, i - 1]) - want) <= tol[j - 1, i - 1] / 1024, (i, j)
    for (nx, ny), halo, dtype in (((66, 12), (3, 2, 1), np.float64), ((62, 9), (5, 5, 5), np.float32)):
        g = _grid(oracle, nx, ny, halo, dtype)
        Hx, Hy, Hz = halo
        size = (nx, ny, 3)
        u, v = R.frame_inputs(size, halo, dtype)
        A = lambda name, i, j: _mpf(g[name][j + Hy - 1, i + Hx - 1])
        for to_native in (False, True):
            ru, rv, scale = R.frame_ref(g, u, v, size, halo, to_native)
            cells = [(1, 1, 1), (nx, ny, 3), (nx // 2 - 1, ny, 2), (nx // 2 + 2, ny, 1), (nx, 1, 2)]
            cells += [(int(rng.integers(1, nx + 1)), int(rng.integers(1, ny + 1)), int(rng.integers(1, 4))) for _ in range(12)]
            for i, j, k in cells:
                if A("dx_cc", i, j) == 0:                                    # a pole cell (test_pole_cells_of_the_frame_rotation)
                    assert np.isnan(ru[k - 1, j - 1, i - 1]) and np.isnan(rv[k - 1, j - 1, i - 1])
                    continue
                ut = (A("phi_cf", i, j + 1) - A("phi_cf", i, j)) * mp.pi / 180 / A("dy_cc", i, j)
                vt = -(A("phi_fc", i + 1, j) - A("phi_fc", i, j)) * mp.pi / 180 / A("dx_cc", i, j)
                U = mp.sqrt(ut ** 2 + vt ** 2)
                d1, d2 = ut / U, vt / U
                uo, vo = _mpf(u[k + Hz - 1, j + Hy - 1, i + Hx - 1]), _mpf(v[k + Hz - 1, j + Hy - 1, i + Hx - 1])
                want = (uo * d1 + vo * d2, uo * d2 - vo * d1) if to_native else (uo * d1 - vo * d2, uo * d2 + vo * d1)
                bound = float(R.frame_tolerance(scale[k - 1, j - 1, i - 1], np.float64)) / 1024
                assert abs(_mpf(ru[k - 1, j - 1, i - 1]) - want[0]) <= bound and abs(_mpf(rv[k - 1, j - 1, i - 1]) - want[1]) <= bound, (i, j, k)


def test_reference_mpmath_arithmetic_agrees_with_long_double(oracle):
    """the fall-back arithmetic of geometry_ref (platforms whose long double is a plain double) gives the same reference, NaN cells included"""
    halo, size = (3, 2, 1), (62, 9, 3)
    g = _grid(oracle, 62, 9, halo, np.float32)
    a, tol, valid = R.angle_ref(g["lambda_ff"], g["phi_ff"], size, halo, immersed=R.angle_mask(size))
    a2, tol2, valid2 = R.angle_ref(g["lambda_ff"], g["phi_ff"], size, halo, immersed=R.angle_mask(size), arith="mpmath")
    assert np.array_equal(valid, valid2) and np.all(np.abs(a - a2) <= tol / 1024 + 90 * 2.0 ** -53) and np.allclose(tol, tol2, rtol=1e-12)
    u, v = R.frame_inputs(size, halo, np.float32)
    for to_native in (False, True):
        x = R.frame_ref(g, u, v, size, halo, to_native)
        y = R.frame_ref(g, u, v, size, halo, to_native, arith="mpmath")
        for p, q in zip(x[:2], y[:2]):
            assert np.array_equal(np.isnan(p), np.isnan(q)) and (~np.isfinite(p)).sum() == 2 * 3
            fin = np.isfinite(p)
            assert np.all(np.abs(p[fin] - q[fin]) <= 2.0 ** -52 * x[2][fin])
        assert np.array_equal(x[2].astype(np.float64), y[2])


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("nx", [62, 66, 90, 130, 64, 128, 180])
def test_pole_cells_of_the_frame_rotation(oracle, nx, dtype):
    """When Nx = 2 (mod 4) the two cells i = Nx/2, Nx/2 + 1 of row Ny sit on the pole at the default pole placement: dx_cc = 0 there, and
    both conversions give NaN (-deg2rad(0) / 0, as examples/convert_to_latlong_frame.jl:24 does).  The non-finite outputs are exactly the
    cells with dx_cc == 0: two per level, both in row Ny; none when Nx = 0 (mod 4)."""
    ny, nz, halo = {62: 9, 66: 12, 90: 45, 130: 20, 64: 12, 128: 15, 180: 90}[nx], 3, (4, 4, 2)
    size = (nx, ny, nz)
    g = _grid(oracle, nx, ny, halo, dtype)
    zero = g["dx_cc"][4:4 + ny, 4:4 + nx] == 0
    if nx % 4 == 2:
        assert np.argwhere(zero).tolist() == [[ny - 1, nx // 2 - 1], [ny - 1, nx // 2]]
    else:
        assert not zero.any()
    u, v = R.frame_inputs(size, halo, dtype)
    for to_native in (False, True):
        outs = oracle.convert_frame(g, u, v, size, halo, to_native=to_native)
        refs = R.frame_ref(g, u, v, size, halo, to_native)[:2]
        for o, r in zip(outs, refs):
            for a in (o[2:2 + nz, 4:4 + ny, 4:4 + nx], r):
                assert np.array_equal(~np.isfinite(a), np.broadcast_to(zero, a.shape)) and np.array_equal(np.isnan(a), ~np.isfinite(a))
