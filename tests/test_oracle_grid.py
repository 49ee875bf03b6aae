"""The CPU oracle's grid build held to tests/grid_ref.py -- a whole-array long-double statement of the reference's Julia text -- on EVERY cell of
every padded parent: interiors, first and last columns, rows 2 and Ny, the pole meridians and pole nodes, coordinate and metric halos, the
continuation rows, Float32 grids and latitude bands.  tests/test_gpu_grid.py proves GPU == oracle bit for bit; this proves that the numbers
both of them hold are the reference's.  Tolerances and their derivation: the docstring of tests/grid_ref.py."""
import numpy as np
import pytest

import grid_ref as G

SMALL = [((10, 10), (4, 4, 4)), ((4, 5), (4, 4, 4)), ((8, 4), (4, 4, 1))]     # zipper test grid; fold reads row 1; Ny == Hy
CASES = ([(s, h, p, dt) for s, h in SMALL for p in G.PARAMS for dt in G.DTYPES] + G.gpu_cases()
         + [((360, 180), (4, 4, 4), "default", dt) for dt in G.DTYPES]
         + [((360, 180), (4, 4, 4), p, np.float64) for p in G.PARAMS if p != "default"])


def _oracle_and_reference(oracle, size, halo, pid, dtype, arith=None):
    kw = G.PARAMS[pid]
    got = oracle.build_grid(size + (1,), halo=halo, dtype=dtype, **kw)
    return got, G.build(size, halo, dtype=dtype, stored=got, arith=arith, **kw)


@pytest.mark.parametrize("case", CASES, ids=[G.case_id(c) for c in CASES])
def test_oracle_within_tolerance_of_the_reference_on_every_cell(oracle, case):
    size, halo, pid, dtype = case
    got, ref = _oracle_and_reference(oracle, size, halo, pid, dtype)
    print(G.case_id(case), {k: round(v, 3) for k, v in ref.worst(got).items()})
    ref.check(got, G.case_id(case))
    G.check_halo_copies(got, size, halo)


@pytest.mark.parametrize("band", G.BANDS, ids=[f"{b[0][0]}x{b[0][1]}-Hy{b[1][1]}-rows{b[2]}-{b[3]}" for b in G.BANDS])
@pytest.mark.parametrize("dtype", G.DTYPES, ids=["f64", "f32"])
def test_latitude_bands(oracle, band, dtype):
    """rows jstart - Hy .. jend + Hy of the global padded arrays (distributed_tripolar_grid.jl:41-49), one band thinner than its halo"""
    size, halo, jstart, jend = band
    glob, ref = _oracle_and_reference(oracle, size, halo, "default", dtype)
    got = oracle.build_grid(size + (1,), halo=halo, dtype=dtype, jstart=jstart, jend=jend)
    assert got["phi_cc"].shape == (jend - jstart + 1 + 2 * halo[1], size[0] + 2 * halo[0])
    ref.rows(jstart, jend).check(got, f"band {jstart}..{jend}")


def test_tables(oracle):
    """integer southernmost_latitude: bit-equal to the oracle's tables, Float32 lambda tables included; a dyadic non-integer one: within 1 ulp"""
    differing = 0
    for size in [(10, 10), (4, 5), (8, 4), (62, 7), (126, 15), (130, 36), (360, 180)]:
        for dtype in G.DTYPES:
            for south in (-80, -89):
                for a, b in zip(G.tables(size, south, dtype), oracle.tables(size + (1,), dtype=dtype, southernmost_latitude=south)):
                    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (size, dtype, south)
            mine, theirs = G.tables(size, -75.5, dtype), oracle.tables(size + (1,), dtype=dtype, southernmost_latitude=-75.5)
            for a, b in zip(mine[:2], theirs[:2]):
                assert np.array_equal(a, b)
            for a, b in zip(mine[2:], theirs[2:]):
                assert (np.abs(a - b) <= np.spacing(np.abs(a))).all(), (size, "phi table more than 1 ulp from the rounded rational")
                differing += int((a != b).sum())
    print("phi-table elements 1 ulp from the correctly rounded rational at south = -75.5:", differing)
    lf = G.tables((130, 36), dtype=np.float32)[0]
    assert np.array_equal(lf, lf.astype(np.float32).astype(np.float64)) and not np.array_equal(lf, G.tables((130, 36))[0])


@pytest.mark.parametrize("size,halo", SMALL, ids=["10x10", "4x5", "8x4"])
@pytest.mark.parametrize("pid", ["default", "south-75.5-R1"])
def test_reference_pinned_to_40_digit_mpmath(oracle, size, halo, pid):
    """Both arithmetic backends on the smallest shapes, whole parents: the long-double reference is within 1/256 of every tolerance of the
    40-digit one.  The cells compared include a pole node, both pole-meridian columns, columns 1 and Nx, rows 2 and Ny and a wrap-crossing edge
    (asserted below), so the long-double rules for the signs of zero and the half-angles next to pi are pinned, not only the plain cells."""
    got, ld = _oracle_and_reference(oracle, size, halo, pid, np.float64, "longdouble")
    _, mp = _oracle_and_reference(oracle, size, halo, pid, np.float64, "mpmath")
    (Nx, Ny), (Hx, Hy) = size, halo[:2]
    lf, _, _, pc = G.tables(size, G.PARAMS[pid].get("southernmost_latitude", -80))
    assert lf[0] == -180.0 and lf[Nx // 2] == 0.0 and pc[-1] == 90.0                     # both pole meridians, and the pole nodes on row Ny
    formula = G.coordinates(size, southernmost_latitude=G.PARAMS[pid].get("southernmost_latitude", -80), substitute_row_Ny=False, arith="longdouble")
    for col in (Nx // 4, Nx // 4 + Nx // 2):                 # pre-shift i = 1 and N / 2 + 1 (for Nx = 2 mod 4 the fold then overwrites the second)
        assert float(formula["phi_fc"][Ny - 1, col]) == 90.0 and float(formula["lambda_fc"][Ny - 1, col]) == (70 + 270) % 360   # :75, :82, :86
    assert any(w[Hy + 1:Hy + Ny].any() for w in ld.wrap.values()), "no wrap-crossing edge in the sample"
    worst = 0.0
    for name in G.COORDS + G.METRICS:
        hi = np.asarray(ld.values[name], dtype=np.float64)                                 # long double = hi + lo exactly
        lo = np.asarray(ld.values[name] - hi, dtype=np.float64)
        d = np.abs(((mp.B.lift(hi) + mp.B.lift(lo)) - mp.values[name]).astype(np.float64))
        if name.startswith("lambda"):
            d = np.minimum(d, np.abs(d - 360))
        t = ld.tol[name]
        assert np.allclose(t, mp.tol[name], rtol=1e-9, atol=0), name
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d == 0, 0.0, d / t)
        assert (r <= 1 / 256).all(), (name, float(r.max()))
        worst = max(worst, float(r.max()))
    print("long double against mpmath, worst ratio to the tolerance:", worst)
    ld.check(got, "long double")
    mp.check(got, "mpmath")


@pytest.mark.parametrize("size", [(10, 10), (62, 7), (126, 15), (130, 36)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_Ny_substitution_Nx_2_mod_4(oracle, size):
    """zipper_boundary_condition.jl:102, :135: the fold overwrites the upper half of interior row Ny of a y-Center field with its mirror.  For
    Nx = 2 mod 4 the shift Nx / 4 is not a quarter turn, the formula row is NOT symmetric about the pivot, and the stored row differs from
    the formula's value: the upper half equals the mirrored lower half bit for bit and is far from the unsubstituted value."""
    Nx, Ny = size
    assert Nx % 4 == 2
    H = 4
    got = oracle.build_grid(size + (1,))
    formula = G.coordinates(size, substitute_row_Ny=False)
    stored = G.coordinates(size)
    i = np.arange(Nx // 2 + 1, Nx + 1)                                                    # i > Nx / 2
    for name in ("lambda_cc", "lambda_fc", "phi_cc", "phi_fc"):
        ip = Nx - i + 1 if name.endswith("cc") else Nx - i + 2                            # :125 / :90 (no wrap: i' <= Nx / 2 + 1)
        row = got[name][H + Ny - 1, H:H + Nx]
        assert np.array_equal(row[i - 1], row[ip - 1]), name
        moved = np.abs(row[i - 1] - np.asarray(formula[name][Ny - 1, i - 1], dtype=np.float64))
        if name.startswith("lambda"):
            moved = np.minimum(moved, np.abs(moved - 360))
        print(size, name, "row Ny moved by up to", float(moved.max()), "degrees;", int((moved > 100 * G.COORD_TOL).sum()), "of", i.size, "cells")
        assert moved.max() > (1.0 if name.startswith("lambda") else 0.1), name          # degrees: nowhere near the tolerance
        near = np.abs(row - np.asarray(stored[name][Ny - 1], dtype=np.float64))
        assert (np.minimum(near, np.abs(near - 360)) <= G.COORD_TOL).all(), name
        lower = np.abs(row[:Nx // 2] - np.asarray(formula[name][Ny - 1, :Nx // 2], dtype=np.float64))
        assert (np.minimum(lower, np.abs(lower - 360)) <= G.COORD_TOL).all(), name         # the lower half is the formula's


@pytest.mark.parametrize("size", [(8, 4), (64, 8), (124, 14), (128, 22)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_row_Ny_substitution_Nx_0_mod_4(oracle, size):
    """For Nx = 0 mod 4 the shift is a quarter turn and the grid is symmetric about the pivot: the formula row already equals its mirror to
    within the coordinate tolerance, so the substitution only makes the two halves bit-equal -- it moves no cell by more than 2 x COORD_TOL."""
    Nx, Ny = size
    assert Nx % 4 == 0
    H = 4
    got = oracle.build_grid(size + (1,))
    formula = G.coordinates(size, substitute_row_Ny=False)
    i = np.arange(Nx // 2 + 1, Nx + 1)
    for name in ("lambda_cc", "lambda_fc", "phi_cc", "phi_fc"):
        ip = Nx - i + 1 if name.endswith("cc") else Nx - i + 2
        row = got[name][H + Ny - 1, H:H + Nx]
        assert np.array_equal(row[i - 1], row[ip - 1]), name
        f = np.asarray(formula[name][Ny - 1], dtype=np.float64)
        d = np.abs(f[i - 1] - f[ip - 1])
        assert (np.minimum(d, np.abs(d - 360)) <= 2 * G.COORD_TOL).all(), name
