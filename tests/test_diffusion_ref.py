"""The numpy reference of the diffusive tendency (tests/diffusion_ref.py) held to properties (no GPU, nothing goes through the kernel): its
two statements agree bit for bit, a constant field gives zero, a closed basin conserves, nothing leaks through a closed face, the scheme is
second order, it commutes with the mirror in x, it reads the cells the header says and no others, its closed faces are the count planes',
the fold row closes from the filled halo alone, and the equivalent forms of a call give the same bits."""
import itertools
import math

import numpy as np
import pytest

import diffusion_ref as R
from diffusion_cases import F32, F64, bottom, draw
from vorticity_ref import same_bits

SIZE, HALO = (12, 7, 4), (2, 2, 1)


def _interior(p, a):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = p["size"], p["halo"]
    return a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_the_two_statements_of_the_rule_agree_bit_for_bit(dtype):
    combos = [(terms, mode, form, fl, mc) for terms, mode, form, fl, mc in itertools.product(
        (R.HORIZONTAL, R.VERTICAL, R.HORIZONTAL | R.VERTICAL, 0), (R.ADD, R.WRITE), (R.CONSTANT, R.PROFILE, R.FIELD),
        (((), ()), ((0,), (1,)), ("all", "all")), ((False, False), (True, False), (False, True), (True, True)))
        if terms or fl != ((), ())]
    for n, (terms, mode, form, (top, bot), (masked, closed)) in enumerate(combos):
        if n % 5 and dtype is F32:
            continue                                               # Float32 takes every fifth combination
        p = draw(SIZE, HALO, dtype, nfields=2, terms=terms, mode=mode, form=form, top=top, bottom_flux=bot, masked=masked, closed=closed, seed=n)
        for q in range(2):
            assert same_bits(R.by_columns(p, q), R.tendency_planes(p, q)) == 0, (terms, mode, form, top, bot, masked, closed, q)
    for size, halo in (((2, 1, 1), (1, 1, 1)), ((4, 2, 2), (1, 1, 0)), ((6, 3, 3), (3, 1, 2))):
        p = draw(size, halo, dtype, top=(0,), bottom_flux=(0,), form=R.FIELD, masked=True, closed=True, mode=R.ADD)
        assert same_bits(R.by_columns(p, 0), R.tendency_planes(p, 0)) == 0, size


def test_a_constant_field_gives_exactly_zero_from_both_interior_groups():
    for terms in (R.HORIZONTAL, R.VERTICAL, R.HORIZONTAL | R.VERTICAL):
        for masked, closed in ((False, False), (True, True)):
            p = draw(SIZE, HALO, F64, terms=terms, form=R.FIELD, masked=masked, closed=closed)
            p["c"] = [np.full_like(p["c"][0], 3.25)]
            assert not R.tendency_planes(p, 0).any(), terms


def _basin(dtype=F64):
    """a closed basin with land inside: land on the rows 1 and Ny and the columns 1 and Nx, drawn counts elsewhere; masked and closed"""
    size, halo = (12, 9, 5), (1, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, _) = size, halo
    p = draw(size, halo, dtype, nfields=1, form=R.FIELD, top="all", bottom_flux="all")
    h, zc, _ = bottom(size, halo, dtype)
    h = h.copy()
    h[Hy, :] = h[Hy + Ny - 1, :] = h[:, Hx] = h[:, Hx + Nx - 1] = 1.0              # above every centre: land
    h[:Hy] = h[Hy + Ny:] = 1.0
    h[:, :Hx] = h[:, Hx + Nx:] = 1.0
    from immersed_ref import column_counts
    p.update(h=h, zc=zc, counts=column_counts(h, zc, size, halo, True)["cc"])
    return p


def test_a_closed_basin_conserves_up_to_the_roundings_of_the_rule():
    """sum V G = -sum az (Jt - Jb) over the wet columns.  In exact arithmetic every interior flux cancels against its neighbour's (each is
    formed once) and the faces around the basin are closed.  The rule rounds, per cell: five times on the way to S (two differences and a sum
    for Hsum, one difference for Vsum, one sum), each by at most eps/2 relative to a partial result bounded by the sum A of |F| over the
    cell's six faces; then 1/V, the product with S and the test's own product with V, three more -- eight roundings, each at most
    (eps/2) A (1 + O(eps)).  Summed over the cells with fsum (exact), the bound is 8 (eps/2) sum_cells A, taken with eps instead of eps/2
    for the second-order terms."""
    p = _basin()
    (Nx, Ny, Nz), (Hx, Hy, Hz) = p["size"], p["halo"]
    F = {}
    G = R.tendency_planes(p, 0, F)
    m = np.clip(p["counts"], 0, Nz)
    wet = np.arange(Nz)[:, None, None] >= m[None]
    az = p["az"][Hy:Hy + Ny, Hx:Hx + Nx]
    V = az[None] * p["dz_c"][:, None, None]
    assert wet.any() and not wet.all() and not G[~wet].any()
    total = math.fsum((V * G)[wet])
    column = m < Nz
    Jt, Jb = p["top"][0][Hy:Hy + Ny, Hx:Hx + Nx], p["bottom"][0][Hy:Hy + Ny, Hx:Hx + Nx]
    want = math.fsum((-(az * Jt))[column]) - math.fsum((-(az * Jb))[column])
    A = (np.abs(F["Fx"][:, :, 1:]) + np.abs(F["Fx"][:, :, :-1]) + np.abs(F["Fy"][:, 1:]) + np.abs(F["Fy"][:, :-1])
         + np.abs(F["Fz"][1:]) + np.abs(F["Fz"][:-1]))
    bound = 8 * np.finfo(F64).eps * math.fsum(A[wet])
    print(f"\nconservation: sum V G = {total!r}, -sum az (Jt - Jb) = {want!r}, difference {abs(total - want):.3e}, bound {bound:.3e}")
    assert abs(want) > 1 and abs(total - want) <= bound


def test_nothing_leaks_through_a_closed_face():
    size, halo = (12, 7, 4), (2, 2, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    p = draw(size, halo, F64, terms=R.HORIZONTAL, closed=True, masked=False)
    _, zc, counts = bottom(size, halo, F64)
    n = counts["cc"]
    assert n[2, 3] == 0 and (n[[1, 3, 2, 2], [3, 3, 2, 4]] == Nz).all()               # the isolated wet cell of the draw
    G = R.tendency_planes(p, 0)
    assert not G[:, 2, 3].any() and G.any()
    # tracer placed only in land cells changes no wet G: with it or without it, the wet cells get the same
    land = np.arange(Nz)[:, None, None] < n[None]
    wet_only = [a.copy() for a in p["c"]]
    ina = R.inactive_planes(p, F64)
    padded_land = np.zeros(p["c"][0].shape, dtype=bool)
    padded_land[Hz:Hz + Nz, Hy - 1:Hy + Ny + 1, Hx - 1:Hx + Nx + 1] = ina
    wet_only[0][padded_land] = 0.0
    q = dict(p, c=wet_only)
    assert padded_land.any() and same_bits(R.tendency_planes(q, 0)[~land], G[~land]) == 0
    only_land = dict(p, c=[np.where(padded_land, p["c"][0], 0.0)])
    assert not R.tendency_planes(only_land, 0)[~land].any()


def test_second_order_on_a_cosine_mode_with_uniform_metrics():
    errors = []
    for N in (16, 32, 64):
        size, halo = (N, 1, N), (1, 1, 0)
        p = draw(size, halo, F64, terms=R.HORIZONTAL | R.VERTICAL)
        shape = p["c"][0].shape
        for k in ("dx_fc", "dy_fc", "dx_cf", "dy_cf", "az"):
            p[k] = np.ones_like(p[k])
        dx = dz = 1.0 / N
        p["dx_fc"][...] = dx
        p["dy_fc"][...] = 1.0
        p["az"][...] = dx
        p["dz_c"], p["dz_f"] = np.full(N, dz), np.full(N + 1, dz)
        x = (np.arange(-1, N + 1) + 0.5) * dx                      # periodic in x, its halo filled
        z = (np.arange(N) + 0.5) * dz                              # no flux through the faces 1 and Nz + 1: the cosine's own condition
        c = np.cos(2 * np.pi * x)[None, None, :] * np.cos(np.pi * z)[:, None, None]
        p["c"] = [np.broadcast_to(c, shape).copy()]
        p["kappa_h"], p["kappa_z"] = 0.5, 0.25
        G = R.tendency_planes(p, 0)[:, 0, :]
        want = -(0.5 * (2 * np.pi) ** 2 + 0.25 * np.pi ** 2) * c[:, 0, 1:-1]
        errors.append(np.abs(G - want).max())
    orders = [math.log2(a / b) for a, b in zip(errors, errors[1:])]
    assert all(1.9 < o < 2.1 for o in orders), (errors, orders)


def test_the_mirror_in_x_commutes_with_the_rule_bit_for_bit():
    p = draw(SIZE, HALO, F64, nfields=1, form=R.FIELD, top="all", bottom_flux="all", masked=True, closed=True, mode=R.ADD)
    cell = lambda a: None if a is None else np.ascontiguousarray(a[..., ::-1])                     # noqa: E731
    face = lambda a: np.ascontiguousarray(np.roll(a[..., ::-1], 1, axis=-1))                       # noqa: E731    face i -> face Nx + 2 - i
    q = dict(p, c=[cell(p["c"][0])], G=[cell(p["G"][0])], kappa_z=cell(p["kappa_z"]), top=[cell(p["top"][0])], bottom=[cell(p["bottom"][0])],
             dx_fc=face(p["dx_fc"]), dy_fc=face(p["dy_fc"]), dx_cf=cell(p["dx_cf"]), dy_cf=cell(p["dy_cf"]), az=cell(p["az"]),
             counts=cell(p["counts"]), h=cell(p["h"]))
    assert same_bits(R.tendency_planes(q, 0)[..., ::-1], R.tendency_planes(p, 0)) == 0


def _cells_read(p, name, q=None, delta=1.0):
    """the cells of the array p[name] (of its entry q) whose change by `delta` changes an output: a boolean array of its shape"""
    base = R.tendency_planes(p, 0)
    a = p[name] if q is None else p[name][q]
    read = np.zeros(a.shape, dtype=bool)
    for idx in np.ndindex(a.shape):
        b = a.copy()
        b[idx] = (0.0 if np.isnan(b[idx]) else b[idx]) + delta
        other = dict(p, **{name: b if q is None else [b]})
        read[idx] = same_bits(R.tendency_planes(other, 0), base) != 0
    return read


def test_the_cells_read_are_the_headers():
    """found by perturbing every cell of every input with a value (a closed face would swallow a NaN through its select)"""
    size, halo = (4, 3, 3), (2, 2, 2)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    ys, xs, zs = slice(Hy, Hy + Ny), slice(Hx, Hx + Nx), slice(Hz, Hz + Nz)
    p = draw(size, halo, F64, form=R.FIELD, top="all", bottom_flux="all", mode=R.ADD)
    plus = np.zeros(p["c"][0].shape, dtype=bool)                   # one cell W, E, S, N of the interior at the levels 1..Nz: no corner, no z halo
    plus[zs, ys, Hx - 1:Hx + Nx + 1] = True
    plus[zs, Hy - 1:Hy + Ny + 1, xs] = True
    assert np.array_equal(_cells_read(p, "c", 0), plus)
    own = np.zeros_like(plus)
    own[zs, ys, xs] = True
    assert np.array_equal(_cells_read(p, "G", 0), own)             # ADD reads the interior of G
    assert np.array_equal(_cells_read(dict(p, terms=R.VERTICAL), "c", 0), own)        # without the horizontal group: the own column
    faces = np.zeros(p["kappa_z"].shape, dtype=bool)
    faces[Hz + 1:Hz + Nz, ys, xs] = True                           # the faces 2..Nz of the interior columns
    assert np.array_equal(_cells_read(p, "kappa_z"), faces)
    inner = np.zeros(p["az"].shape, dtype=bool)
    inner[ys, xs] = True
    for name in ("top", "bottom"):
        assert np.array_equal(_cells_read(p, name, 0), inner), name
    assert np.array_equal(_cells_read(p, "az"), inner)
    east, north = inner.copy(), inner.copy()
    east[ys, Hx + Nx] = True
    north[Hy + Ny, xs] = True
    for name, want in (("dx_fc", east), ("dy_fc", east), ("dx_cf", north), ("dy_cf", north)):
        assert np.array_equal(_cells_read(p, name), want), name
    dzf = np.zeros(Nz + 1, dtype=bool)
    dzf[1:Nz] = True
    assert np.array_equal(_cells_read(p, "dz_f"), dzf)
    # the bottom height: one cell W, E, S, N of the interior (the south row only where the south side is no wall)
    h = np.full(p["az"].shape, -2.0)
    zc = np.linspace(-1, 0, 2 * Nz + 1)[1::2]
    cross = plus[Hz]
    for wall in (False, True):
        want = cross.copy()
        if wall:
            want[Hy - 1] = False
        assert np.array_equal(_cells_read(dict(p, h=h, zc=zc, wall=wall), "h", delta=5.0), want), wall
    # with counts, of kappa only the faces k0+1..Nz
    n = np.zeros((Ny, Nx), dtype=np.int32)
    n[1, 2], n[0, 0], n[2, 3] = 1, Nz, Nz - 1
    k0 = np.zeros(p["kappa_z"].shape, dtype=bool)
    for j, i in np.ndindex(Ny, Nx):
        k0[Hz + n[j, i] + 1:Hz + Nz, Hy + j, Hx + i] = True
    assert np.array_equal(_cells_read(dict(p, counts=n), "kappa_z"), k0)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_the_closed_faces_are_the_count_planes(dtype):
    """closed_x <=> k <= n_fc and closed_y <=> k <= n_cf on every interior face, from one filled h"""
    for size, halo in ((SIZE, HALO), ((20, 9, 6), (4, 4, 4)), ((8, 5, 1), (1, 1, 1))):
        Nx, Ny, Nz = size
        h, zc, counts = bottom(size, halo, dtype)
        p = dict(size=size, halo=halo, h=h, zc=zc, wall=True)
        cx, cy = R.closed_faces(p, dtype)
        k = np.arange(1, Nz + 1)[:, None, None]
        assert np.array_equal(cx[:, :, :Nx], k <= counts["fc"][None]) and np.array_equal(cy[:, :Ny], k <= counts["cf"][None])
        assert cx.any() and not cx.all()
        # the face i = Nx + 1 is the face 1 of the periodic image
        assert np.array_equal(cx[:, :, Nx], cx[:, :, 0])


def test_the_fold_row_closes_from_the_filled_halo_alone():
    """land at the fold partner of a wet cell of row Ny: the face j = Ny + 1 of that column is closed at every level although the cell and
    its three other neighbours say nothing of it -- no fold index map enters, only row Ny + 1 of the filled h"""
    size, halo = SIZE, HALO
    (Nx, Ny, Nz), (Hx, Hy, _) = size, halo
    h, zc, counts = bottom(size, halo, F64)
    assert counts["cc"][Ny - 1, 1] == 0                            # the wet cell (2, Ny)
    assert (zc <= h[Hy + Ny, Hx + 1]).all()                        # land in the halo row above it
    _, cy = R.closed_faces(dict(size=size, halo=halo, h=h, zc=zc, wall=True), F64)
    assert cy[:, Ny, 1].all() and not cy[:, Ny - 1, 1].all()
    # and it acts: the cell's northward flux is zero whatever the halo row of c holds
    p = draw(size, halo, F64, terms=R.HORIZONTAL, closed=True)
    other = [p["c"][0].copy()]
    other[0][:, Hy + Ny, Hx + 1] += 1.0
    assert same_bits(R.tendency_planes(dict(p, c=other), 0), R.tendency_planes(p, 0)) == 0
    open_ = dict(p, h=None, zc=None)
    assert same_bits(R.tendency_planes(dict(open_, c=other), 0), R.tendency_planes(open_, 0)) != 0


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_equivalent_forms_give_the_same_bits(dtype):
    # Nz = 1: both boundary faces sit on the one cell
    p = draw((6, 3, 1), (1, 1, 1), dtype, top="all", bottom_flux="all", form=R.PROFILE)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = p["size"], p["halo"]
    T = dtype
    az = p["az"][Hy:Hy + Ny, Hx:Hx + Nx]
    vertical = dict(p, terms=R.VERTICAL)
    want = (T(1) / (az * p["dz_c"][0])) * (-(az * p["top"][0][Hy:Hy + Ny, Hx:Hx + Nx]) - -(az * p["bottom"][0][Hy:Hy + Ny, Hx:Hx + Nx]))
    assert same_bits(R.tendency_planes(vertical, 0)[0], want) == 0
    # ADD is WRITE plus the old value
    a = draw(SIZE, HALO, dtype, mode=R.ADD, form=R.FIELD, top="all", masked=True, closed=True)
    w = dict(a, mode=R.WRITE)
    old = _interior(a, a["G"][0])
    wet = np.arange(SIZE[2])[:, None, None] >= np.clip(a["counts"], 0, SIZE[2])[None]
    assert same_bits(R.tendency_planes(a, 0)[wet], (old + R.tendency_planes(w, 0))[wet]) == 0
    assert not R.tendency_planes(a, 0)[~wet].any()                 # the mask value in both modes
    # the three kappa forms on equal values
    Nz = SIZE[2]
    f = draw(SIZE, HALO, dtype, form=R.FIELD, masked=True)
    profile = np.linspace(0.1, 1.3, Nz + 1).astype(dtype)
    field = np.empty_like(f["kappa_z"])
    field[HALO[2]:HALO[2] + Nz + 1] = profile[:, None, None]
    got = [R.tendency_planes(dict(f, kappa_z=k, form=form), 0) for k, form in ((field, R.FIELD), (profile, R.PROFILE))]
    assert same_bits(got[0], got[1]) == 0
    const = [R.tendency_planes(dict(f, kappa_z=k, form=form), 0) for k, form in ((np.full_like(field, 0.37), R.FIELD), (np.full_like(profile, 0.37), R.PROFILE),
                                                                                 (0.37, R.CONSTANT))]
    assert same_bits(const[0], const[1]) == 0 and same_bits(const[1], const[2]) == 0
    # the bits do not depend on the grouping: a field alone, or among others
    g = draw(SIZE, HALO, dtype, nfields=5, top=(1, 3), bottom_flux=(0, 3), masked=True, closed=True)
    for q in range(5):
        alone = dict(g, c=[g["c"][q]], G=[g["G"][q]], top=[g["top"][q]], bottom=[g["bottom"][q]])
        assert same_bits(R.tendency_planes(alone, 0), R.tendency_planes(g, q)) == 0
    # a table without a plane for the field is a zero flux, and it makes the vertical group present
    none = draw(SIZE, HALO, dtype, terms=R.HORIZONTAL)
    assert same_bits(R.tendency_planes(dict(none, top=[None]), 0), R.tendency_planes(none, 0) + T(0)) == 0
