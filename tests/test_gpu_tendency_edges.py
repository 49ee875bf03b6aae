"""GPU tests of the six tendency kernels where their addressing can go wrong and no other test looks: element offsets at and past 2^31,
latitude bands, the smallest shapes check_geom admits.  The kernels: the centred, WENO5 x/y and all-WENO tracer tendencies, the
vector-invariant momentum tendency and its WENO5-upwinded form, the free-surface sub-step -- all driven through the C ABI from ONE adapter
table (tests/tendency_windows.py: library, symbol, array list, numpy reference).  Every comparison is bit for bit, on whole arrays, on
integer views; there is no tolerance anywhere in this file.  tests/test_tendency_windows_ref.py holds, on the CPU, every fact these
comparisons rest on: that a cut-out of rows or of planes is a valid stand-in for the whole, on which levels an all-WENO plane window
agrees with the column, that the comparators notice one wrong bit, and that every address of the smallest shapes lies inside its parent.

B1, past 2^31 elements: 8640 x 4320 x 64 at halo (4, 4, 4) in Float32, the geometry of tests/test_gpu_past_2g.py -- a parent has
2 694 855 168 elements (w one plane more), offset 2^31 falls in padded plane 57 (interior level 54), byte offsets cross 2^33.  One test per
3-D tendency.  The free-surface sub-step works on 2-D planes, which cannot reach 2^31 elements (check_geom refuses such a plane): it has
no such test.
B2, latitude bands: all six kernels.  The free-surface sub-step CARRIES row 1 of V (the south wall row): row 1 of a band that starts inside
the domain holds V's input where the global call computed; every other row and array is the global call's.
B3, the smallest shapes: all six kernels.  The free surface refuses Ny = 1; its smallest is (2, 2, 1)."""
import contextlib
import gc
import time

import numpy as np
import pytest
import torch

import tendency_windows as tw
from momentum_ref import METRICS
from tendency_windows import DTAU, F32, F64, GRAVITY, KERNELS, MASK_VALUE, SENTINEL, WITH_LEVELS, equal_bits, interior
from vorticity_ref import same_bits

pytestmark = pytest.mark.gpu

TWO31, TWO30 = 1 << 31, 1 << 30
UNSUPPORTED = -5                                   # TPG_ERR_UNSUPPORTED


@pytest.fixture(autouse=True)
def _free_hbm():
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _ids(v):
    return v.name if isinstance(v, tw.Kernel) else {F32: "f32", F64: "f64"}.get(v)


# ---- the one way into the six entry points -----------------------------------------------------------------------------------------------------
def _ptr(t):
    return None if t is None else t.data_ptr()


def _launch(osg, gpu, kernel, d, outs, size, halo, masked):
    """the status of kernel's entry point on the device arrays d and the outputs outs (both by the names of the adapter table)"""
    fn = getattr(getattr(osg._lib, kernel.library + "_lib")(), kernel.symbol)
    n = [_ptr(d[c]) if masked else None for c in kernel.counts]
    if kernel.counts == ("n_cc",):                                 # the tracer tendencies: tables of one tracer
        args = [osg._lib.ptr_table([d["c"]]), osg._lib.ptr_table([outs["G"]]), 1, *(d[k].data_ptr() for k in ("u", "v", "w", *kernel.planes, "dz_c")),
                *n, MASK_VALUE]
    elif kernel.has_levels:                                        # the momentum tendencies
        args = [*(d[k].data_ptr() for k in ("u", "v", "w")), outs["Gu"].data_ptr(), outs["Gv"].data_ptr(), *(d[k].data_ptr() for k in METRICS),
                d["dz_f"].data_ptr(), *n, MASK_VALUE]
    else:                                                          # the free-surface sub-step, without averaging
        args = [*(outs[k].data_ptr() for k in kernel.outputs), *(d[k].data_ptr() for k in kernel.planes[:5]), None, None, None,
                *(d[k].data_ptr() for k in kernel.planes[5:]), d["depth"].data_ptr(), *n, DTAU, GRAVITY, 0.0]
    if kernel.scheme_arg:
        args.append(0)
    geom = (*size, *halo) if kernel.has_levels else (*size, halo[0], halo[1])
    return fn(*args, *geom, osg._lib.ft_of(outs[kernel.outputs[0]].dtype), osg._lib.current_stream_ptr(gpu))


def _check(osg, kernel, status):
    getattr(osg._lib, "check_" + kernel.library)(status)


def _dev(host, gpu, offset=0):
    """device copy of `host`, `offset` elements past an allocation (element-aligned, off the 16-B grid for offset 1)"""
    host = np.ascontiguousarray(host)
    if not host.flags.writeable:
        host = host.copy()                                         # torch.from_numpy wants a writable array
    t = torch.empty(host.size + offset, dtype=torch.from_numpy(host.reshape(-1)[:1]).dtype, device=gpu)[offset:].view(host.shape)
    t.copy_(torch.from_numpy(host))
    assert offset == 0 or t.data_ptr() % 16 != 0
    return t


def _fresh(kernel, size, halo, dtype, gpu, offset=0):
    return {name: _dev(np.full(tw.shape_of(kernel, name, size, halo), SENTINEL, dtype), gpu, offset) for name in kernel.outputs}


def _run(osg, gpu, kernel, h, size, halo, masked, offset=0):
    """the entry point on device copies of the host problem h into fresh sentinel-filled outputs -> the whole outputs on the host"""
    dtype = h[kernel.planes[0]].dtype.type
    d = {k: _dev(a, gpu, offset) for k, a in h.items()}
    outs = _fresh(kernel, size, halo, dtype, gpu, offset)
    _check(osg, kernel, _launch(osg, gpu, kernel, d, outs, size, halo, masked))
    return {k: o.cpu().numpy() for k, o in outs.items()}


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
BIG, BIG_HALO = (8640, 4320, 64), (4, 4, 4)
# the levels each window is compared on: what tests/test_tendency_windows_ref.py::test_the_all_weno_windows_of_the_gpu_test computed.  An
# all-WENO window of ten leaves out its bottom three levels (unless they are the column's) and its top three (unless they are the column's):
# their faces have another order in the window than in the column
COMPARED = {True: {"bottom": [1, 2, 3, 4], "middle": [53, 54, 55, 56], "top": [61, 62, 63, 64]},
            False: {"bottom": list(range(1, 8)), "middle": [53, 54, 55, 56], "top": list(range(58, 65))}}


@contextlib.contextmanager
def _budget(gpu, what):
    """wall time and peak device memory of the block, printed; the peak stays under half the card"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(gpu)
    print(f"\n[tendency past 2g] {what}: {time.perf_counter() - t0:.1f} s, peak {peak / 2**30:.1f} GiB")
    assert peak < torch.cuda.get_device_properties(gpu).total_memory / 2, peak


def _cell_at(offset, size, halo):
    """the interior cell (k, j, i), 0-based, that holds element `offset` of a padded parent (asserted: it is an interior cell)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    sy, sx = Ny + 2 * Hy, Nx + 2 * Hx
    pk, rem = divmod(offset, sy * sx)
    pj, pi = divmod(rem, sx)
    assert Hz <= pk < Hz + Nz and Hy <= pj < Hy + Ny and Hx <= pi < Hx + Nx
    return pk - Hz, pj - Hy, pi - Hx


def _random(gpu, shape, seed, lo, hi):
    return torch.empty(shape, dtype=torch.float32, device=gpu).uniform_(lo, hi, generator=torch.Generator(device=gpu).manual_seed(seed))


def _big_counts(gpu, size, seed):
    """0 in most columns, drawn from 0 .. Nz in one column of eight, Nz in columns 0 .. 7 of every row: the mask's stores reach the top level
    (past 2^31) there, the tendency's everywhere else"""
    Nx, Ny, Nz = size
    gen = torch.Generator(device=gpu).manual_seed(seed)
    n = torch.randint(0, Nz + 1, (Ny, Nx), dtype=torch.int32, device=gpu, generator=gen)
    keep = torch.randint(0, 8, (Ny, Nx), dtype=torch.int32, device=gpu, generator=gen) == 0
    n = torch.where(keep, n, torch.zeros_like(n))
    n[:, :8] = Nz
    return n


def _bits_of(value, like):
    return tw._ints(torch.full((1,), value, dtype=like.dtype, device=like.device))[0]


def _assert_only_the_interior_is_written(out, size, halo):
    """every halo cell still holds the sentinel, no interior cell does: on the device, by narrow, on integer views"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    I, s = tw._ints(out), _bits_of(SENTINEL, out)
    for dim, x in enumerate((Hz, Hy, Hx)):
        assert bool((I.narrow(dim, 0, x) == s).all()) and bool((I.narrow(dim, I.shape[dim] - x, x) == s).all()), dim
    for k0 in range(0, Nz, 8):
        assert not bool((I[Hz + k0:Hz + min(k0 + 8, Nz), Hy:Hy + Ny, Hx:Hx + Nx] == s).any()), k0


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
GLOBAL = (40, 24, 3)


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
    """40 x 24 x 3, global parents random in every cell, cut into bands as rows jstart - Hy .. jend + Hy of every array (the count planes,
    which have no halo, by their rows): three bands of 8 rows, and a chain with a band of exactly Hy rows -- one partial tile whose south
    and north stencil arms both leave the band -- beside one of Hy + 1 rows and the rest.  Each band's output equals the matching rows of
    the global DEVICE result, and, as a whole parent, the reference on the cut: the band's own halo rows still hold the sentinel.  (Row 1
    of V of a free-surface band that starts inside the domain is carried: it holds V's input, as the reference on the cut says.)"""
    size, halo = GLOBAL, _band_halo(kernel, dtype)
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
SMALL = [(k, size, halo, dtype) for k in KERNELS.values() for size, halo in tw.SMALLEST[k.name] for dtype in (F64, F32)]


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
