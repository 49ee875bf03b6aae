"""CPU premises of tests/test_gpu_tendency_edges.py, on the numpy references alone (advection_ref, weno_ref, weno_xyz_ref, momentum_ref,
weno_momentum_ref, weno_vi_ref, free_surface_ref): the GPU tests compare one big call with calls on cut-outs of the same memory, and with the
references on cut-outs; here a cut-out is shown to be a valid stand-in.  Which GPU comparison rests on which fact:

    GPU comparison                                                        CPU fact here
    B1 b  a plane window's call == the same levels of the big output     test_a_plane_window_gives_the_levels_of_the_column (+ the shifted counts)
    B1 b  the all-WENO windows compare the levels premise A names         test_the_all_weno_windows_of_the_gpu_test, levels_that_agree
    B1 c  the reference on a strip (rows and planes) == the big output    test_a_row_cut_gives_the_rows_of_the_whole and the plane window, composed:
                                                                          test_a_strip_is_a_row_cut_of_a_plane_window
    B2    a band's call == the rows of the global call == the reference   test_a_row_cut_gives_the_rows_of_the_whole
    B1/B2 torch.equal / same_bits on integer views notice a wrong cell    test_the_comparators_have_teeth
    B3    every address of the smallest shapes lies inside its parent     test_every_address_of_the_smallest_shapes_is_inside

Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

import tendency_windows as tw
from tendency_windows import F32, F64, KERNELS, WITH_LEVELS, equal_bits, interior, levels_that_agree, plane_cut, row_cut
from vorticity_ref import same_bits
from weno_xyz_ref import face_order

CASES = [((20, 12, 9), (4, 4, 4)), ((20, 12, 3), (3, 3, 1))]
_WHOLE = {}


def _halo(kernel, halo):
    return halo if kernel.has_levels else (halo[0], halo[1], 0)       # the free surface: (Hx, Hy2) and no levels


def _whole(kernel, size, halo, dtype):
    """(problem, {masked: reference outputs}) of a case: drawn and computed once, never modified"""
    key = (kernel.name, size, halo, dtype)
    if key not in _WHOLE:
        h = tw.draw(kernel, size, halo, dtype)
        _WHOLE[key] = (h, {m: kernel.ref(h, size, halo, m) for m in (False, True)})
    return _WHOLE[key]


def _ids(v):
    return v.name if isinstance(v, tw.Kernel) else {F32: "f32", F64: "f64"}.get(v) or ("x".join(map(str, v[0])) + "-h" + "".join(map(str, v[1])))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=_ids)
@pytest.mark.parametrize("case", CASES, ids=_ids)
@pytest.mark.parametrize("kernel", KERNELS.values(), ids=_ids)
def test_a_row_cut_gives_the_rows_of_the_whole(kernel, case, dtype, masked):
    """Rows lo .. lo + rows + 2 Hy of every parent and metric plane (rows lo .. lo + rows of the count planes) for rows in {Hy, Hy + 1, 8}
    and every lo that fits: the reference on the cut equals the matching interior rows of the reference on the whole, bit for bit.

    Cells the rule reads that a cut drops: NONE.  Every rule reads at most Hy rows south and north of an interior row (three for the WENO
    arms, one for the centred ones, one row north of v, dx_cf and the face rows), and the cut keeps Hy rows on either side; in x and z it
    keeps everything.  One rule is not a stencil: the free-surface sub-step CARRIES row 1 of V (the south wall row, which the caller's Open
    fill owns).  Row 1 of a cut that starts inside the domain is a computed row of the whole, so there -- and only there -- the cut gives
    V's input instead; every other row of V, and all of eta and U, are the whole's."""
    size, halo = case[0], _halo(kernel, case[1])
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h, want = _whole(kernel, size, halo, dtype)
    for rows in (Hy, Hy + 1, 8):
        for lo in range(Ny - rows + 1):
            cut, csize = row_cut(kernel, h, size, halo, lo, rows)
            got = kernel.ref(cut, csize, halo, masked)
            for name in kernel.outputs:
                g, w = interior(kernel, got[name], csize, halo), interior(kernel, want[masked][name], size, halo)[..., lo:lo + rows, :]
                if name == "V_out" and lo > 0:
                    assert same_bits(g[0], interior(kernel, h["V"], size, halo)[lo]) == 0 and same_bits(g[0], w[0]) > 0
                    g, w = g[1:], w[1:]
                assert same_bits(g, w) == 0, (name, rows, lo)
                edge = np.ones(got[name].shape, bool)
                interior(kernel, edge, csize, halo)[...] = False
                assert (got[name][edge] == tw.SENTINEL).all()          # the cut's own halo rows: untouched


def _windows(Nz):
    return [(a, b) for a in range(1, Nz + 1) for b in range(a, Nz + 1)]


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=_ids)
@pytest.mark.parametrize("case", CASES, ids=_ids)
@pytest.mark.parametrize("kernel", WITH_LEVELS, ids=_ids)
def test_a_plane_window_gives_the_levels_of_the_column(kernel, case, dtype, masked):
    """The contiguous planes a - Hz .. b + Hz of c, u, v (b + 1 + Hz of w), the entries a .. b of dz_c (the faces a .. b + 1 of dz_f) and the
    count planes shifted to clip(n - (a - 1), 0, Nz') form a problem with Nz' = b - a + 1 levels.  For the four kernels that are centred in z
    its interior equals the levels a .. b of the whole for EVERY window (both momentum count planes are shifted); for the all-WENO tendency
    on the levels levels_that_agree names, and that set is exactly the levels whose two faces keep their order."""
    size, halo = case
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h, want = _whole(kernel, size, halo, dtype)
    for a, b in _windows(Nz):
        cut, csize = plane_cut(kernel, h, size, halo, a, b)
        assert all(cut[n].shape == tw.shape_of(kernel, n, csize, halo) for n in cut)
        got = kernel.ref(cut, csize, halo, masked)
        levels = levels_that_agree(kernel, a, b, Nz)
        assert not kernel.centred_in_z or levels == list(range(a, b + 1))
        for name in kernel.outputs:
            for k in range(a, b + 1):
                differ = same_bits(got[name][Hz + k - a], want[masked][name][Hz + k - 1])        # whole padded planes: halo cells the sentinel
                assert differ == 0 or k not in levels, (name, a, b, k)
        if masked:                                                     # the shifted counts mask what the column's counts mask
            for n in kernel.counts:
                k = np.arange(a, b + 1)[:, None, None]
                assert np.array_equal(k - (a - 1) <= np.clip(cut[n], 0, b - a + 1)[None], k <= np.clip(h[n], 0, Nz)[None])


@pytest.mark.parametrize("dtype", [F64, F32], ids=_ids)
def test_the_all_weno_windows_of_the_gpu_test(dtype):
    """weno_xyz on a column of 16 levels: the window that touches the real top wall agrees up to level Nz; an interior window of 10 levels
    agrees on its middle 4, and on no other level does it HAVE to (the bottom three and top three levels have a face of another order: with
    this data they do differ); the bottom window agrees from level 1.  And for the windows the GPU test uses (Nz = 64, the cell at 2^31 in
    level 54) the helper returns the sets written here -- never an empty one: a condition, not a measurement."""
    kernel, size, halo = KERNELS["weno_xyz"], (8, 6, 16), (3, 3, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h, want = _whole(kernel, size, halo, dtype)
    expected = {(7, 16): list(range(10, 17)), (4, 13): [7, 8, 9, 10], (1, 10): list(range(1, 8))}
    for (a, b), levels in expected.items():
        assert levels_that_agree(kernel, a, b, Nz) == levels
        cut, csize = plane_cut(kernel, h, size, halo, a, b)
        got = kernel.ref(cut, csize, halo, True)["G"]
        differ = [same_bits(got[Hz + k - a], want[True]["G"][Hz + k - 1]) for k in range(a, b + 1)]
        assert all(d == 0 for k, d in zip(range(a, b + 1), differ) if k in levels)
        assert all(d > 0 for k, d in zip(range(a, b + 1), differ) if k not in levels)
    # the order table itself, by hand: a window of ten has the orders 2 1 3 5 5 5 5 5 3 1 2 at its faces 1 .. 11
    assert [face_order(f, 10) for f in range(1, 12)] == [2, 1, 3, 5, 5, 5, 5, 5, 3, 1, 2]
    windows = tw.b1_windows(kernel, 64, 54)
    assert windows == {"bottom": (1, 10), "middle": (50, 59), "top": (55, 64)}
    assert levels_that_agree(kernel, *windows["bottom"], 64) == list(range(1, 8))
    assert levels_that_agree(kernel, *windows["middle"], 64) == [53, 54, 55, 56]
    assert levels_that_agree(kernel, *windows["top"], 64) == list(range(58, 65))
    for k in WITH_LEVELS:                                              # every kernel's windows: non-empty, level 54 and level 64 among them
        w = tw.b1_windows(k, 64, 54)
        sets = {name: levels_that_agree(k, *ab, 64) for name, ab in w.items()}
        assert all(sets.values()) and 54 in sets["middle"] and 64 in sets["top"] and 1 in sets["bottom"]
        assert sets == ({"bottom": [1, 2, 3, 4], "middle": [53, 54, 55, 56], "top": [61, 62, 63, 64]} if k.centred_in_z else
                        {"bottom": list(range(1, 8)), "middle": [53, 54, 55, 56], "top": list(range(58, 65))})


@pytest.mark.parametrize("dtype", [F64, F32], ids=_ids)
@pytest.mark.parametrize("kernel", WITH_LEVELS, ids=_ids)
def test_a_strip_is_a_row_cut_of_a_plane_window(kernel, dtype):
    """what the GPU test's numpy anchor does: rows AND planes cut, masked -- the reference on the strip equals the whole on the strip's rows
    and on the window's agreeing levels"""
    size, halo = (20, 12, 16), (4, 4, 4)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h, want = _whole(kernel, size, halo, dtype)
    for (a, b), (lo, rows) in (((4, 13), (2, 6)), ((7, 16), (Ny - 5, 5))):
        window, wsize = plane_cut(kernel, h, size, halo, a, b)
        strip, ssize = row_cut(kernel, window, wsize, halo, lo, rows)
        got = kernel.ref(strip, ssize, halo, True)
        levels = levels_that_agree(kernel, a, b, Nz)
        assert len(levels) >= 4
        for name in kernel.outputs:
            for k in levels:
                assert same_bits(got[name][Hz + k - a, Hy:Hy + rows, Hx:Hx + Nx], want[True][name][Hz + k - 1, Hy + lo:Hy + lo + rows, Hx:Hx + Nx]) == 0


@pytest.mark.parametrize("dtype", [F64, F32], ids=_ids)
def test_the_comparators_have_teeth(dtype):
    """equal_bits -- torch.equal on integer views for device arrays, same_bits for host ones, whole arrays -- reports a mismatch for one
    cell that differs in the last bit, for one level swapped with its neighbour and for one row shifted by one; and none for a copy.  This
    stands in for running a kernel with a narrowed offset or a broken clamp, which would read out of bounds"""
    kernel, size, halo = KERNELS["weno"], (20, 12, 9), (4, 4, 4)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    good = _whole(kernel, size, halo, dtype)[1][True]["G"]
    wrong = {}
    one = good.copy()
    one[Hz + 5, Hy + 7, Hx + 11] = np.nextafter(one[Hz + 5, Hy + 7, Hx + 11], dtype(np.inf))
    wrong["last bit"] = one
    swapped = good.copy()
    swapped[[Hz + 3, Hz + 4]] = swapped[[Hz + 4, Hz + 3]]
    wrong["levels swapped"] = swapped
    shifted = good.copy()
    shifted[Hz + 2, Hy + 4, Hx + 1:Hx + Nx] = good[Hz + 2, Hy + 4, Hx:Hx + Nx - 1]
    wrong["row shifted"] = shifted
    assert equal_bits(good, good.copy()) and equal_bits(torch.from_numpy(good.copy()), torch.from_numpy(good.copy()))
    for what, bad in wrong.items():
        assert same_bits(bad, good) >= 1 and (what != "last bit" or same_bits(bad, good) == 1)
        assert not equal_bits(bad, good), what
        assert not equal_bits(torch.from_numpy(bad), torch.from_numpy(good.copy())), what
        # on views, as the GPU test compares them: a level's padded plane, the interior
        k = {"last bit": 5, "levels swapped": 3, "row shifted": 2}[what]
        assert not equal_bits(torch.from_numpy(bad)[Hz + k], torch.from_numpy(good.copy())[Hz + k]), what
        assert not equal_bits(interior(kernel, torch.from_numpy(bad), size, halo), interior(kernel, torch.from_numpy(good.copy()), size, halo))
    nan = good.copy()
    nan[Hz, Hy, Hx] = np.nan
    assert equal_bits(nan, nan.copy())                                 # host: NaNs by NaN-ness


WALKED = [(k, size, halo, dtype, offset) for k in WITH_LEVELS if k.name in tw.SMALLEST for size, halo in tw.SMALLEST[k.name] for dtype in (F64, F32) for offset in (0, 1)]


def test_every_address_of_the_smallest_shapes_is_inside():
    """walk() mirrors each kernel's ro / rc / eo tables, e0, j0 and its clamps.  For every smallest shape, type and pointer offset the GPU test
    runs: no read leaves the padded parent or the count plane, no store leaves the interior, and every interior cell is stored exactly once.
    The forms the shapes are chosen for are the ones taken: (4, 4, 5) at halo 4 in Float32 is the SHARE form with ONE chunk per row (lane 0
    stores, lane 1 is the chunk past the end); Float32 at Hx = 3 is the non-SHARE GEN form with W = 4 = Nx.  The walk has teeth: one halo cell
    fewer than the rule's arm, or an unclamped chunk past the end, is reported."""
    for kernel, size, halo, dtype, offset in WALKED:
        assert all(n >= a for n, a in zip(halo, kernel.arm)) and halo[0] <= size[0] and halo[1] <= size[1]
        bad, facts = tw.walk(kernel, size, halo, dtype, offset)
        assert bad == [], (kernel, size, halo, dtype, offset, bad[:5])
        assert (facts["stores"] == 1).all(), (kernel, size, halo)
    for name in ("weno", "weno_xyz"):
        facts = tw.walk(KERNELS[name], (4, 4, 5), (4, 4, 4), F32)[1]
        assert (facts["W"], facts["gen"], facts["share"], facts["cpr"]) == (4, False, True, 1)
        facts = tw.walk(KERNELS[name], (4, 3, 1), (3, 3, 1), F32)[1]
        assert (facts["W"], facts["gen"], facts["share"], facts["cpr"]) == (4, True, False, 1)
        facts = tw.walk(KERNELS[name], (4, 3, 1), (3, 3, 1), F64)[1]
        assert (facts["W"], facts["gen"], facts["share"], facts["cpr"]) == (2, True, True, 2)
    assert tw.walk(KERNELS["advection"], (2, 1, 1), (1, 1, 1), F32)[1]["W"] == 2 and tw.walk(KERNELS["momentum"], (2, 1, 1), (1, 1, 1), F64)[1]["cpr"] == 1
    for kernel in {k for k, *_ in WALKED}:                             # teeth: one halo cell fewer, in each direction
        size, halo = tw.SMALLEST[kernel.name][-1]
        for axis in range(3):
            thin = tuple(kernel.arm[i] - 1 if i == axis else halo[i] for i in range(3))
            assert tw.walk(kernel, size, thin, F64)[0], (kernel, thin)
