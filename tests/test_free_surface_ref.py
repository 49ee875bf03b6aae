"""The numpy reference of the split-explicit free-surface sub-step (tests/free_surface_ref.py) held without a device: against exact rational
arithmetic with one rounding per operation (the scalar operations of tests/test_special_value_refs.py), cell by cell, on a small case with
special values among the data -- the wrap column, the carried row 1, H = 0 (a land column) and a zero metric among the cells."""
import math

import numpy as np
import pytest

from free_surface_ref import METRICS, cells_read, interior_substep, same_bits, substep
from special_values import pool
from test_special_value_refs import _add, _div, _mul, _sub

DTYPES = [np.float32, np.float64]
SIZE, HX, HY2 = (6, 4, 3), 2, 3
DTAU, G, WEIGHT = 0.3, 9.80665, 0.1                                 # none representable: each is converted once to the field type


def _case(rng, dtype, size=SIZE, Hx=HX, Hy2=HY2):
    Nx, Ny, Nz = size
    shape = (Ny + 2 * Hy2, Nx + 2 * Hx)
    state = [rng.uniform(-1, 1, shape).astype(dtype) for _ in range(3)]
    G_ = [rng.uniform(-1, 1, shape).astype(dtype) for _ in range(2)]
    metrics = {k: rng.uniform(0.5, 2, shape).astype(dtype) for k in METRICS}
    depth = rng.uniform(0.5, 2, Nz + 1).astype(dtype)
    return state, G_, metrics, depth


def _bits_equal(got, want):
    """a numpy scalar against a Python float: the same bits, NaN by NaN-ness"""
    got = float(got)
    if math.isnan(want):
        return math.isnan(got)
    return got == want and math.copysign(1.0, got) == math.copysign(1.0, want)


@pytest.mark.parametrize("counts", [False, True], ids=["full-depth", "count-planes"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_equals_rational_arithmetic_rounded_once_per_operation(dtype, counts):
    Nx, Ny, Nz = SIZE
    rng = np.random.default_rng(1)
    (eta, U, V), (GU, GV), m, depth = _case(rng, dtype)
    p = pool(dtype)
    for a in (eta, U, V, GU):                                      # special values among the data: every IEEE rule of *, +, -, /
        where = rng.random(a.shape) < 0.1
        a[where] = p[rng.integers(0, p.size, int(where.sum()))]
    eta[HY2 + 2, HX + 3], V[HY2 + 1, HX + 1] = np.nan, np.inf       # one NaN and one Inf explicitly in the interior
    m["az_cc"][HY2 + 1, HX + 2] = 0.0                              # a zero metric divides, as the rule says
    m["dx_fc"][HY2 + 2, HX] = 0.0                                  # ... in the wrap column's pressure gradient too
    m["dy_cf"][HY2 + 3, HX + 4] = -0.0
    depth[Nz] = 0.0                                                # a land column: H = 0 only drops the pressure term
    n_fc = n_cf = None
    if counts:
        n_fc, n_cf = (rng.integers(-1, Nz + 3, (Ny, Nx)).astype(np.int32) for _ in range(2))
        n_fc[1, 0], n_fc[2, 3], n_cf[1, 1], n_cf[3, 5] = Nz, Nz + 2, Nz, -1
    got = interior_substep(eta, U, V, GU, GV, m, depth, SIZE, HX, HY2, DTAU, G, n_fc, n_cf)
    f = float
    dtau, g = f(dtype(DTAU)), f(dtype(G))
    at = lambda a, j, i: f(a[j + HY2, i + HX])                     # 0-based interior (j, i); i = Nx is the east halo column, j = Ny the north row

    def eta_new(j, i):
        fe, fw = _mul(at(m["dy_fc"], j, i + 1), at(U, j, i + 1), dtype), _mul(at(m["dy_fc"], j, i), at(U, j, i), dtype)
        fn, fs = _mul(at(m["dx_cf"], j + 1, i), at(V, j + 1, i), dtype), _mul(at(m["dx_cf"], j, i), at(V, j, i), dtype)
        d = _div(_add(_sub(fe, fw, dtype), _sub(fn, fs, dtype), dtype), at(m["az_cc"], j, i), dtype)
        return _sub(at(eta, j, i), _mul(dtau, d, dtype), dtype)

    def depth_at(n, j, i):
        return f(depth[0]) if n is None else f(depth[min(max(int(n[j, i]), 0), Nz)])

    for j in range(Ny):
        for i in range(Nx):
            e = eta_new(j, i)
            assert _bits_equal(got[0][j, i], e), ("eta", i, j)
            west = eta_new(j, i - 1 if i else Nx - 1)              # column 1 takes column Nx, whose east flux is the halo column's
            px = _div(_sub(e, west, dtype), at(m["dx_fc"], j, i), dtype)
            gH = _mul(g, depth_at(n_fc, j, i), dtype)
            want = _add(at(U, j, i), _mul(dtau, _sub(at(GU, j, i), _mul(gH, px, dtype), dtype), dtype), dtype)
            assert _bits_equal(got[1][j, i], want), ("U", i, j)
            if j == 0:
                want = at(V, j, i)
            else:
                py = _div(_sub(e, eta_new(j - 1, i), dtype), at(m["dy_cf"], j, i), dtype)
                gH = _mul(g, depth_at(n_cf, j, i), dtype)
                want = _add(at(V, j, i), _mul(dtau, _sub(at(GV, j, i), _mul(gH, py, dtype), dtype), dtype), dtype)
            assert _bits_equal(got[2][j, i], want), ("V", i, j)
    assert all(np.isnan(x).any() and np.isfinite(x).any() for x in got) and any(np.isinf(x).any() for x in got) and same_bits(got[2][0], V[HY2, HX:HX + Nx]) == 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_planes_keep_every_other_cell_and_the_averages_add_the_new_state(dtype):
    Nx, Ny, Nz = SIZE
    rng = np.random.default_rng(2)
    state, G_, m, depth = _case(rng, dtype)
    shape = state[0].shape
    out0 = [np.full(shape, 7, dtype) for _ in range(3)]
    bars0 = [rng.uniform(-1, 1, shape).astype(dtype) for _ in range(3)]
    new = interior_substep(*state, *G_, m, depth, SIZE, HX, HY2, DTAU, G)
    outs, none = substep(out0, state, G_, m, depth, SIZE, HX, HY2, DTAU, G)
    assert none is None
    inner = np.zeros(shape, bool)
    inner[HY2:HY2 + Ny, HX:HX + Nx] = True
    for o, x in zip(outs, new):
        assert (o[~inner] == 7).all() and same_bits(o[inner].reshape(Ny, Nx), x) == 0
    outs2, bars = substep(out0, state, G_, m, depth, SIZE, HX, HY2, DTAU, G, averages=bars0, weight=WEIGHT)
    for o, o2, b, b0, x in zip(outs, outs2, bars, bars0, new):
        assert same_bits(o, o2) == 0 and same_bits(b[~inner], b0[~inner]) == 0
        assert same_bits(b[inner].reshape(Ny, Nx), b0[inner].reshape(Ny, Nx) + dtype(WEIGHT) * x) == 0
    # the cells read: poisoning every other cell changes nothing
    n_fc, n_cf = (rng.integers(0, Nz + 1, (Ny, Nx)).astype(np.int32) for _ in range(2))
    n_fc[:] = np.minimum(n_fc, 2)
    n_cf[1:] = np.minimum(n_cf[1:], 2)
    n_cf[0] = 3                                                    # row 1 of n_cf is not read: entry 3 of depth_of_count is selected by nothing
    read = cells_read(SIZE, HX, HY2, n_fc, n_cf)
    assert read["eta"].sum() == Nx * Ny and read["U"].sum() == Nx * Ny + Ny and read["V"].sum() == Nx * Ny + Nx
    assert read["GV"].sum() == Nx * (Ny - 1) and not read["n_cf"][0].any() and read["depth_of_count"].tolist() == [True, True, True, False]
    assert cells_read(SIZE, HX, HY2)["depth_of_count"].tolist() == [True, False, False, False]
    nan = dtype(np.nan)
    ps = [np.where(read[k], a, nan) for k, a in zip(("eta", "U", "V"), state)]
    pG = [np.where(read[k], a, nan) for k, a in zip(("GU", "GV"), G_)]
    pm = {k: np.where(read[k], m[k], nan) for k in METRICS}
    pd = np.where(read["depth_of_count"], depth, nan)
    clean = interior_substep(*state, *G_, m, depth, SIZE, HX, HY2, DTAU, G, n_fc, n_cf)
    dirty = interior_substep(*ps, *pG, pm, pd, SIZE, HX, HY2, DTAU, G, n_fc, n_cf)
    for c, d in zip(clean, dirty):
        assert same_bits(c, d) == 0 and not np.isnan(d).any()
    # ... and every cell that IS read matters: a NaN planted in it reaches some output
    for k, a in (("U", state[1]), ("V", state[2])):
        edge = read[k] & ~inner
        j, i = np.argwhere(edge)[0]
        b = a.copy()
        b[j, i] = nan
        st = [b if x is a else x for x in state]
        assert any(np.isnan(x).any() for x in interior_substep(*st, *G_, m, depth, SIZE, HX, HY2, DTAU, G))


@pytest.mark.parametrize("dtype", DTYPES)
def test_lake_at_rest_stays_at_rest(dtype):
    """eta constant, U = V = G = 0: every flux is +0, eta' = eta - dtau * (0 / Az) = eta, every gradient (eta' - eta') / d = 0"""
    Nx, Ny, Nz = SIZE
    rng = np.random.default_rng(3)
    _, _, m, depth = _case(rng, dtype)
    shape = m["az_cc"].shape
    eta = np.full(shape, 0.37, dtype)
    zero = np.zeros(shape, dtype)
    new = interior_substep(eta, zero, zero, zero, zero, m, depth, SIZE, HX, HY2, DTAU, G)
    assert (new[0] == dtype(0.37)).all() and (new[1] == 0).all() and (new[2] == 0).all()
    assert not np.signbit(new[1]).any() and not np.signbit(new[2]).any()
