"""GPU tests of the seven tendency kernels where their addressing can go wrong and no other test looks: element offsets at and past 2^31,
latitude bands, the smallest shapes check_geom admits.  The kernels: the centred, WENO5 x/y and all-WENO tracer tendencies, the
vector-invariant momentum tendency, its form with the WENO5-upwinded vorticity term and the one upwinded in every term, the free-surface
sub-step -- all driven through the C ABI from ONE adapter table (tests/tendency_windows.py: library, symbol, array list, numpy reference)
by the one launch of tests/gpu_harness.py.  Every comparison is bit for bit, on whole arrays, on
integer views; there is no tolerance anywhere in this file.  tests/test_tendency_windows_ref.py holds, on the CPU, every fact these
comparisons rest on: that a cut-out of rows or of planes is a valid stand-in for the whole, on which levels an all-WENO plane window
agrees with the column, that the comparators notice one wrong bit, and that every address of the smallest shapes lies inside its parent.

B1, past 2^31 elements: 8640 x 4320 x 64 at halo (4, 4, 4) in Float32, the geometry of tests/test_gpu_past_2g.py -- a parent has
2 694 855 168 elements (w one plane more), offset 2^31 falls in padded plane 57 (interior level 54), byte offsets cross 2^33.  One test per
3-D tendency.  The free-surface sub-step works on 2-D planes, which cannot reach 2^31 elements (check_geom refuses such a plane): it has
no such test.
B2, latitude bands: all seven kernels, at 40 x 24 x 3; the tendency upwinded in every term at 40 x 24 x 7, whose seven levels reach every
class of its z-faces' order table.  The free-surface sub-step CARRIES row 1 of V (the south wall row): row 1 of a band that starts inside
the domain holds V's input where the global call computed; every other row and array is the global call's.
B3, the smallest shapes: the six kernels of one launch, those with an entry in tendency_windows.SMALLEST (the two-launch tendency upwinded
in every term, which tendency_windows.walk does not mirror, has its smallest shapes in tests/test_gpu_weno_vi.py).  The free surface refuses Ny = 1; its smallest is (2, 2, 1)."""
import numpy as np
import pytest
import torch

import tendency_windows as tw
from gpu_harness import (BIG, BIG_HALO, COMPARED, TWO30, TWO31, _assert_only_the_interior_is_written, _big_counts, _bits_of, _budget,  # noqa: F401
                         _cell_at, _check, _dev, _free_hbm, _fresh, _launch, _random, _run)
from tendency_windows import F32, F64, KERNELS, MASK_VALUE, SENTINEL, WITH_LEVELS, equal_bits, interior
from vorticity_ref import same_bits

pytestmark = pytest.mark.gpu

UNSUPPORTED = -5                                   # TPG_ERR_UNSUPPORTED


def _ids(v):
    return v.name if isinstance(v, tw.Kernel) else {F32: "f32", F64: "f64"}.get(v)


_DRAWN = {}


def _problem(kernel, size, halo, dtype):
    """(host problem random in every cell, {masked: reference outputs}): drawn and computed once, shared, never modified"""
    key = (kernel.name, size, halo, dtype)
    if key not in _DRAWN:
        h = tw.draw(kernel, size, halo, dtype)
        _DRAWN[key] = (h, {m: kernel.ref(h, size, halo, m) for m in (False, True)})
    return _DRAWN[key]


def _assert_whole(got, want, what):
    for name in want:
        bad = same_bits(got[name], want[name])
        assert bad == 0, (what, name, bad, "cells differ of", got[name].size)


# ---- B1: past 2^31 elements -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", WITH_LEVELS, ids=_ids)
def test_float32_past_2g_elements(osg, gpu, kernel):
    """8640 x 4320 x 64, halo 4, Float32, with the fused mask.  Data drawn on the device: velocities and tracer of both signs, metrics and
    spacings in [0.5, 2], the outputs sentinel-filled.
    a. every halo cell of every output still holds the sentinel, no interior cell does;
    b. the same entry point on three plane windows -- contiguous plane slices of the SAME tensors, small offsets, fresh small outputs, the
       counts shifted -- equals the big output on the window's levels (COMPARED: all four for the kernels centred in z; for the all-WENO
       tendency the levels of a ten-level window whose faces keep their order), whole padded planes, torch.equal on integer views.  The
       bottom window lies below 2^30, the middle one holds the first interior cell at or past 2^31, the top one ends at the wall and at the
       highest addresses.  The small-shape tests hold that form of the kernel to the reference;
    c. numpy anchor: the reference on a strip of 16 rows around the row that holds offset 2^31 (the middle window's planes), and on the last
       16 rows of the top window, equals the big output there (NaNs by NaN-ness).
    Prints its wall time and peak device memory; the peak stays under half the card."""
    size, halo = BIG, BIG_HALO
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    plane = (Ny + 2 * Hy) * (Nx + 2 * Hx)
    assert np.prod(tw.shape_of(kernel, "u", size, halo), dtype=np.int64) == 2694855168 and TWO31 // plane == 57
    k31, j31, i31 = _cell_at(TWO31, size, halo)
    assert k31 + 1 == 54
    windows = tw.b1_windows(kernel, Nz, k31 + 1)
    with _budget(gpu, kernel.name):
        d = {}
        for seed, name in enumerate(kernel.inputs()):
            lo, hi = (-1.0, 1.0) if name in kernel.signed else (0.5, 2.0)
            d[name] = _random(gpu, tw.shape_of(kernel, name, size, halo), 100 + seed, lo, hi)
        for seed, name in enumerate(kernel.counts):
            d[name] = _big_counts(gpu, size, 200 + seed)
        outs = {name: torch.full(tw.shape_of(kernel, name, size, halo), SENTINEL, dtype=torch.float32, device=gpu) for name in kernel.outputs}
        _check(osg, kernel, _launch(osg, gpu, kernel, d, outs, size, halo, True))
        torch.cuda.synchronize()
        # a
        mv = _bits_of(MASK_VALUE, outs[kernel.outputs[0]])
        for name, out in outs.items():
            _assert_only_the_interior_is_written(out, size, halo)
            top = tw._ints(out)[Hz + Nz - 1, Hy:Hy + Ny, Hx:Hx + Nx]                     # the mask value and the tendency both reach the top level
            assert bool((top[:, :8] == mv).all()) and not bool((top[:, 8:] == mv).all()), name
        # b
        compared = COMPARED[kernel.centred_in_z]
        for which, (a, b) in windows.items():
            levels = tw.levels_that_agree(kernel, a, b, Nz)
            assert levels and levels == compared[which], (which, levels)
            cut, csize = tw.plane_cut(kernel, d, size, halo, a, b)
            wouts = {name: torch.full(tw.shape_of(kernel, name, csize, halo), SENTINEL, dtype=torch.float32, device=gpu) for name in kernel.outputs}
            for name in (*kernel.fields, *kernel.tall, *kernel.planes):                  # on the 16-B grid, as the big call's: the same chunk form
                assert cut[name].is_contiguous() and cut[name].data_ptr() % 16 == 0 and d[name].data_ptr() % 16 == 0, name
            assert all(t.data_ptr() % 16 == 0 for t in (*wouts.values(), *outs.values()))
            assert cut["w"].data_ptr() - d["w"].data_ptr() == (a - 1) * plane * 4
            if which == "bottom":
                assert (b + 1 + 2 * Hz) * plane < TWO30
            if which == "top":
                assert (a - 1 + Hz) * plane > TWO31 and b == Nz          # every interior level of the window lies past 2^31
            _check(osg, kernel, _launch(osg, gpu, kernel, cut, wouts, csize, halo, True))
            torch.cuda.synchronize()
            for name in kernel.outputs:
                for k in levels:
                    assert equal_bits(wouts[name][Hz + k - a], outs[name][Hz + k - 1]), (which, name, k)
            del cut, wouts
        assert k31 + 1 in compared["middle"] and Nz in compared["top"]
        # c
        for which, lo in (("middle", min(max(j31 - 8, 0), Ny - 16)), ("top", Ny - 16)):
            a, b = windows[which]
            window, wsize = tw.plane_cut(kernel, d, size, halo, a, b)
            strip, ssize = tw.row_cut(kernel, window, wsize, halo, lo, 16)
            host = {name: t.contiguous().cpu().numpy() for name, t in strip.items()}
            want = kernel.ref(host, ssize, halo, True)
            for name in kernel.outputs:
                for k in compared[which]:
                    got = outs[name][Hz + k - 1, Hy + lo:Hy + lo + 16, Hx:Hx + Nx].contiguous().cpu().numpy()
                    bad = same_bits(got, want[name][Hz + k - a, Hy:Hy + 16, Hx:Hx + Nx])
                    assert bad == 0, (which, name, k, bad, "cells differ of", got.size)
            assert which != "middle" or lo <= j31 < lo + 16
            del window, strip, host, want
        del d, outs


# ---- B2: latitude bands -----------------------------------------------------------------------------------------------------------------------------
GLOBAL = {k.name: (40, 24, 7 if k.name == "weno_vi" else 3) for k in KERNELS.values()}       # seven levels: every class of weno_vi's z-face orders


def _band_halo(kernel, dtype):
    """Float64 at halo (4, 4, 4), Float32 at (3, 3, 1); the free surface at its own tests' plane halos (Hx, Hy2) = (4, 4) and (5, 2)"""
    if kernel.has_levels:
        return (4, 4, 4) if dtype == F64 else (3, 3, 1)
    return (4, 4, 0) if dtype == F64 else (5, 2, 0)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("layout", ["three", "thin"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=_ids)
@pytest.mark.parametrize("kernel", KERNELS.values(), ids=_ids)
def test_latitude_bands_equal_the_global_field(osg, gpu, kernel, dtype, layout, masked):
    """40 x 24 x 3 (GLOBAL), global parents random in every cell, cut into bands as rows jstart - Hy .. jend + Hy of every array (the count planes,
    which have no halo, by their rows): three bands of 8 rows, and a chain with a band of exactly Hy rows -- one partial tile whose south
    and north stencil arms both leave the band -- beside one of Hy + 1 rows and the rest.  Each band's output equals the matching rows of
    the global DEVICE result, and, as a whole parent, the reference on the cut: the band's own halo rows still hold the sentinel.  (Row 1
    of V of a free-surface band that starts inside the domain is carried: it holds V's input, as the reference on the cut says.)"""
    size, halo = GLOBAL[kernel.name], _band_halo(kernel, dtype)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h, want = _problem(kernel, size, halo, dtype)
    glob = _run(osg, gpu, kernel, h, size, halo, masked)
    _assert_whole(glob, want[masked], "global")
    bands = tw.band_layouts(Ny, Hy)[layout]
    assert sum(rows for _, rows in bands) == Ny and (layout != "thin" or (bands[0][1], bands[1][1]) == (Hy, Hy + 1))
    for lo, rows in bands:
        cut, bsize = tw.row_cut(kernel, h, size, halo, lo, rows)
        got = _run(osg, gpu, kernel, cut, bsize, halo, masked)
        _assert_whole(got, kernel.ref(cut, bsize, halo, masked), ("band parent", lo, rows))
        for name in kernel.outputs:
            g, w = interior(kernel, got[name], bsize, halo), interior(kernel, glob[name], size, halo)[..., lo:lo + rows, :]
            if name == "V_out" and lo > 0:
                assert same_bits(g[0], interior(kernel, h["V"], size, halo)[lo]) == 0
                g, w = g[1:], w[1:]
            assert same_bits(g, w) == 0, ("band against global", name, lo, rows)


# ---- B3: the smallest legal shapes ---------------------------------------------------------------------------------------------------------------------
SMALL = [(k, size, halo, dtype) for k in KERNELS.values() if k.name in tw.SMALLEST for size, halo in tw.SMALLEST[k.name] for dtype in (F64, F32)]


def _small_id(case):
    kernel, size, halo, dtype = case
    return f"{kernel.name}-{'x'.join(map(str, size))}-h{''.join(map(str, halo))}-{_ids(dtype)}"


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("case", SMALL, ids=_small_id)
def test_smallest_shapes_are_bit_exact_and_no_halo_cell_is_written(osg, gpu, case, offset):
    """Nx = 2 (one chunk a row), Ny = 1 (a single row: nr = 1 < JT), Nz = 1, Nx = Hx and Ny = Hy (the WENO arms meet the row's and the
    column's ends), one chunk per row in the SHARE form (lane 0 stores, lane 1 is the chunk past the end): whole parents equal the
    reference's, plain and with the fused mask, with every pointer on the 16-B grid and one element off it.  tendency_windows.walk has
    shown every address of the launch to lie inside its parent (asserted again here, before the launch)"""
    kernel, size, halo, dtype = case
    if kernel.has_levels:
        assert tw.walk(kernel, size, halo, dtype, offset)[0] == []
    h, want = _problem(kernel, size, halo, dtype)
    for masked in (False, True):
        edge = np.ones(want[masked][kernel.outputs[0]].shape, bool)
        interior(kernel, edge, size, halo)[...] = False
        for name in kernel.outputs:                                    # the references themselves: the sentinel exactly on the halo cells
            assert (want[masked][name][edge] == SENTINEL).all() and not (want[masked][name][~edge] == SENTINEL).any()
        _assert_whole(_run(osg, gpu, kernel, h, size, halo, masked, offset), want[masked], ("smallest", masked))


@pytest.mark.parametrize("dtype", [F64, F32], ids=_ids)
def test_free_surface_refuses_a_single_row(osg, gpu, dtype):
    """(2, 1, 1): check_geom admits it, the sub-step does not (row 1 of V is carried, there is no row 2) -- TPG_ERR_UNSUPPORTED, a message,
    the outputs untouched"""
    kernel, size, halo = KERNELS["free_surface"], (2, 1, 1), (1, 1, 0)
    h = tw.draw(kernel, size, halo, dtype)
    d = {k: _dev(a, gpu) for k, a in h.items()}
    outs = _fresh(kernel, size, halo, dtype, gpu)
    assert _launch(osg, gpu, kernel, d, outs, size, halo, False) == UNSUPPORTED
    assert "Ny" in osg._lib.free_surface_lib().tpg_free_surface_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((o == SENTINEL).all()) for o in outs.values())
