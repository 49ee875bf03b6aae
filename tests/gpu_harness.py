"""What the GPU tests of the seven tendency entry points share (tests/test_gpu_advection.py, _weno, _weno_xyz, _momentum, _weno_momentum,
_weno_vi and _tendency_edges), once: the device copies, ONE way into the C entry points built from the adapter table of
tests/tendency_windows.py, the cached draw of a case with its reference outputs, the whole-parent comparisons, the count-plane drawers, the
package-level models, and the device-side helpers of the tests past 2^31 elements.  A plain module, not a conftest: a test file imports the
names it uses -- `_free_hbm` among them, so that the autouse fixture applies to that module.

A case is (size, halo, element type).  Arrays go by the names of the adapter table; a tracer tendency takes a LIST of tracers as "c" and of
outputs as "G" wherever one tensor would do."""
import contextlib
import gc
import time

import numpy as np
import pytest
import torch

import tendency_windows as tw
from immersed_ref import draw_columns, heights_of
from tendency_windows import F32, F64, MASK_VALUE, SENTINEL
from vorticity_ref import same_bits

TWO31, TWO30 = 1 << 31, 1 << 30


@pytest.fixture(autouse=True)
def _free_hbm():
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _id(case):
    size, halo, dtype = case
    return "x".join(map(str, size)) + "-h" + "".join(map(str, halo)) + ("-f64" if dtype == F64 else "-f32")


def _dev(host, gpu, offset=0):
    """device copy of `host`, `offset` elements past an allocation (element-aligned, off the 16-B grid for offset 1)"""
    host = np.ascontiguousarray(host)
    if not host.flags.writeable:
        host = host.copy()                                         # torch.from_numpy wants a writable array
    t = torch.empty(host.size + offset, dtype=torch.from_numpy(host.reshape(-1)[:1]).dtype, device=gpu)[offset:].view(host.shape)
    t.copy_(torch.from_numpy(host))
    assert offset == 0 or t.data_ptr() % 16 != 0
    return t


# ---- the comparisons: whole arrays, bit for bit, NaNs by NaN-ness ------------------------------------------------------------------------------
def _assert_parent(got, want, what):
    bad = same_bits(got, want)
    assert bad == 0, (what, bad, "cells differ of", got.size)


def _assert_pair(got, want, what):
    for name, g, w_ in zip(("Gu", "Gv"), got, want):
        _assert_parent(g, w_, (what, name))


def _assert_inputs_unchanged(d, h, what, names=None):
    """the device arrays `names` of d (None: all of them) still hold what the host problem h holds"""
    for k in d if names is None else names:
        if isinstance(d[k], list):
            for q, c in enumerate(d[k]):
                _assert_parent(c.cpu().numpy(), h[k][q], (what, "input tracer", q))
        else:
            _assert_parent(d[k].cpu().numpy(), h[k], (what, "input", k))


# ---- the one way into the seven entry points --------------------------------------------------------------------------------------------------
def _is_tracer(kernel):
    return "c" in kernel.fields


def _launch(osg, gpu, kernel, d, outs, size, halo, masked=False, counts=None, value=MASK_VALUE, scheme=0, shift=None):
    """the status of kernel's entry point on the device arrays d and the outputs outs (both by the names of the adapter table).  The count
    planes are d's own if `masked`, or `counts`: a tensor or None for each plane of the table.  shift: (name, bytes) moves that input's
    pointer, off its element's grid"""
    lib = osg._lib
    fn = getattr(getattr(lib, kernel.library + "_lib")(), kernel.symbol)
    if counts is None:
        counts = [d[c] if masked else None for c in kernel.counts]
    n = [None if t is None else t.data_ptr() for t in counts]

    def ptrs(*names):
        return [d[k].data_ptr() + (shift[1] if shift and shift[0] == k else 0) for k in names]

    if _is_tracer(kernel):
        tracers, G = ([*x] if isinstance(x, (list, tuple)) else [x] for x in (d["c"], outs["G"]))
        args = [lib.ptr_table(tracers), lib.ptr_table(G), len(tracers), *ptrs("u", "v", "w", *kernel.planes, kernel.column[0]), *n, value]
    elif kernel.has_levels:                                        # the momentum tendencies
        args = [*ptrs("u", "v", "w"), outs["Gu"].data_ptr(), outs["Gv"].data_ptr(), *ptrs(*kernel.planes, kernel.column[0]), *n, value]
    else:                                                          # the free-surface sub-step, without averaging
        args = [*(outs[k].data_ptr() for k in kernel.outputs), *ptrs(*kernel.planes[:5]), None, None, None,
                *ptrs(*kernel.planes[5:], kernel.column[0]), *n, tw.DTAU, tw.GRAVITY, 0.0]
    if kernel.scheme_arg:
        args.append(scheme)
    geom = (*size, *halo) if kernel.has_levels else (*size, halo[0], halo[1])
    return fn(*args, *geom, lib.ft_of(d[kernel.planes[0]].dtype), lib.current_stream_ptr(gpu))


def _check(osg, kernel, status):
    getattr(osg._lib, "check_" + kernel.library)(status)


def _fresh(kernel, size, halo, dtype, gpu, offset=0):
    return {name: _dev(np.full(tw.shape_of(kernel, name, size, halo), SENTINEL, dtype), gpu, offset) for name in kernel.outputs}


def _run(osg, gpu, kernel, h, size, halo, masked, offset=0):
    """the entry point on device copies of the host problem h into fresh sentinel-filled outputs -> the whole outputs on the host"""
    dtype = h[kernel.planes[0]].dtype.type
    d = {k: _dev(a, gpu, offset) for k, a in h.items()}
    outs = _fresh(kernel, size, halo, dtype, gpu, offset)
    _check(osg, kernel, _launch(osg, gpu, kernel, d, outs, size, halo, masked))
    return {k: o.cpu().numpy() for k, o in outs.items()}


def _device(kernel, h, gpu, offset=0):
    """device copies of the inputs of a case"""
    return {k: [_dev(c, gpu, offset) for c in h[k]] if isinstance(h[k], list) else _dev(h[k], gpu, offset) for k in kernel.inputs()}


def _call(osg, gpu, kernel, d, size, halo, which=None, counts=None, value=0.0, offset=0):
    """the entry point on the device arrays d (of a tracer tendency: on the tracers `which`, indices; None: all) into fresh sentinel-filled
    outputs -> the whole parents on the host, a list: one G per tracer, or [Gu, Gv]"""
    if _is_tracer(kernel) and which is not None:
        d = dict(d, c=[d["c"][q] for q in which])
    T = {torch.float64: F64, torch.float32: F32}[d["u"].dtype]
    fresh = [_dev(np.full(tuple(d["u"].shape), SENTINEL, T), gpu, offset) for _ in (d["c"] if _is_tracer(kernel) else kernel.outputs)]
    outs = {"G": fresh} if _is_tracer(kernel) else dict(zip(kernel.outputs, fresh))
    _check(osg, kernel, _launch(osg, gpu, kernel, d, outs, size, halo, counts=counts, value=value))
    return [o.cpu().numpy() for o in fresh]


# ---- a case: its host inputs and reference outputs, drawn once ------------------------------------------------------------------------------------
def _ref(kernel, h, size, halo, counts=(), c=None):
    """the reference parents from sentinel-filled ones: (Gu, Gv); of a tracer tendency G of the tracer c, or the list of them for h["c"].
    With count planes (one for each of the table) the mask is fused, its value MASK_VALUE"""
    if _is_tracer(kernel) and c is None:
        return [_ref(kernel, h, size, halo, counts, c) for c in h["c"]]
    problem = dict(h, **dict(zip(kernel.counts, counts)))
    if _is_tracer(kernel):
        problem["c"] = c
    out = kernel.ref(problem, size, halo, len(counts) > 0)
    return out["G"] if _is_tracer(kernel) else tuple(out[k] for k in kernel.outputs)


_CASES = {}


def _case(kernel, case, ntracers=None):
    """host arrays of a case, random in EVERY cell (halos included) -- u, v, w (and the tracers) in [-1, 1], the metrics and spacings in
    [0.5, 2] --, and under "want" the reference parents from sentinel-filled ones: computed once per kernel and case, shared by the tests,
    never modified (tests copy what they change).  The order of the draws is each operator's own: u, v, w, then the planes and dz_c and
    `ntracers` tracers for a tracer tendency, the per-level vector and the planes for a momentum tendency"""
    key = (kernel.name, case, ntracers)
    if key not in _CASES:
        size, halo, dtype = case
        rng = np.random.default_rng([*size, *halo, np.dtype(dtype).itemsize])
        column = kernel.column[0]
        h = {}
        for name in ("u", "v", "w", *kernel.planes, column) if _is_tracer(kernel) else ("u", "v", "w", column, *kernel.planes):
            lo, hi = (-1, 1) if name in kernel.signed else (0.5, 2)
            h[name] = rng.uniform(lo, hi, tw.shape_of(kernel, name, size, halo)).astype(dtype)
        if _is_tracer(kernel):
            h["c"] = [rng.uniform(-1, 1, tw.shape_of(kernel, "c", size, halo)).astype(dtype) for _ in range(ntracers)]
        h["want"] = _ref(kernel, h, size, halo)
        for a in (*h["want"], *h.get("c", ()), *(h[k] for k in ("u", "v", "w", column, *kernel.planes))):
            a.setflags(write=False)
        _CASES[key] = h
    return _CASES[key]


_PLANES = {}


def _drawn_counts(case, q, varied):
    """count plane q (0, 1) of a case for a drawn bottom with a count above Nz and a negative one planted (a count plane of a deeper grid; a
    column the counts call never writes), computed once per size and halo.  varied: the draw is held to have a land column, an open one
    and, with two levels or more, one between"""
    size, halo, _ = case
    Nx, Ny, Nz = size
    if (size, halo, q) not in _PLANES:
        rng = np.random.default_rng([11 + q, *size, *halo])
        n = draw_columns(rng, Nx, Ny, Nz).astype(np.int32)
        n[Ny - 1 - q, Nx - 1] = Nz + 3
        n[q, 0] = -2
        n.setflags(write=False)
        _PLANES[size, halo, q] = n
    n = _PLANES[size, halo, q]
    assert not varied or (n.shape == (Ny, Nx) and (n == 0).any() and (n == Nz).any() and (Nz < 2 or ((n > 0) & (n < Nz)).any()))
    return n


def _count_plane(case):
    """the (Center, Center) count plane of a tracer tendency"""
    return _drawn_counts(case, 0, True)


def _count_planes(case, varied=True):
    """the (Face, Center) and (Center, Face) count planes of a momentum tendency, of two drawn bottoms"""
    planes = _drawn_counts(case, 0, varied), _drawn_counts(case, 1, varied)
    assert (planes[0] != planes[1]).any()
    return planes


# ---- the package: models on a built grid --------------------------------------------------------------------------------------------------------
def _filled(osg, like, interior, base, boundary_conditions="default"):
    """the parent fill_halo_regions gives a field at `like`'s location and grid that held `base` (a parent) and got that interior"""
    f = osg.Field(like.loc, like.grid, boundary_conditions=boundary_conditions)
    f.data.copy_(torch.from_numpy(np.ascontiguousarray(base)).reshape(f.data.shape))
    f.interior().copy_(torch.from_numpy(np.ascontiguousarray(interior)).reshape(f.interior().shape))
    osg.fill_halo_regions([f])
    return f.data.cpu().numpy()


def _grid(osg, size, halo, tdt, immersed):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo, z=(-1, 0))
    if immersed:
        zc = grid.z_centers[Hz:Hz + Nz].cpu().numpy()
        rng = np.random.default_rng(19)
        grid = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)))
    return grid


def _tracer_model(osg, gpu, size, halo, tdt, immersed, ntracers=2, seed=3):
    """(grid, tracers, u, v, w, G, Gm): filled c, u, v, w from compute_w_from_continuity, random tendencies"""
    grid = _grid(osg, size, halo, tdt, immersed)
    gen = torch.Generator(device=gpu).manual_seed(seed)
    u, v = osg.XFaceField(grid), osg.YFaceField(grid)
    tracers, G, Gm = ([osg.CenterField(grid) for _ in range(ntracers)] for _ in range(3))
    for f in (u, v, *tracers, *G, *Gm):
        f.data.uniform_(-1, 1, generator=gen)
    osg.fill_halo_regions([u, v, *tracers])
    w = osg.compute_w_from_continuity(u, v)
    return grid, tracers, u, v, w, G, Gm


def _velocity_model(osg, gpu, size, halo, tdt, immersed, seed=3):
    """(grid, u, v, w, Gu, Gv, Gum, Gvm): filled u, v, w from compute_w_from_continuity (its horizontal halos filled), random tendencies"""
    grid = _grid(osg, size, halo, tdt, immersed)
    gen = torch.Generator(device=gpu).manual_seed(seed)
    u, Gu, Gum = (osg.XFaceField(grid) for _ in range(3))
    v, Gv, Gvm = (osg.YFaceField(grid) for _ in range(3))
    for f in (u, v, Gu, Gv, Gum, Gvm):
        f.data.uniform_(-1, 1, generator=gen)
    osg.fill_halo_regions([u, v])
    w = osg.compute_w_from_continuity(u, v)
    return grid, u, v, w, Gu, Gv, Gum, Gvm


def _host_model(osg, grid, u, v, w):
    """host copies of u, v, w, the grid's own metric arrays and spacings and the count plane of a tracer tendency"""
    g = getattr(grid, "underlying_grid", grid)
    h = {"u": u.data.cpu().numpy(), "v": v.data.cpu().numpy(), "w": w.data.cpu().numpy()}
    for k in ("dy_fc", "dx_cf", "az_cc"):
        h[k] = g.arrays[k].cpu().numpy()
    h["dz_c"] = osg.z_center_spacings(grid, u.data.dtype).numpy().astype(h["u"].dtype)
    counts = getattr(grid, "column_counts", None)
    h["n_cc"] = None if counts is None else counts["cc"].cpu().numpy()
    return h


def _host_metrics(osg, kernel, grid, dtype):
    """(the metric planes, the per-level spacings of a momentum tendency's table row, (n_fc, n_cf) or (None, None)) of the grid, on the host"""
    g = getattr(grid, "underlying_grid", grid)
    m = {k: g.arrays[k].cpu().numpy() for k in kernel.planes}
    spacings = {"dz_f": osg.z_all_face_spacings, "dz_c": osg.z_center_spacings}[kernel.column[0]]
    dz = spacings(grid, dtype).numpy().astype(m["dx_fc"].dtype)
    counts = getattr(grid, "column_counts", None)
    n = (None, None) if counts is None else (counts["fc"].cpu().numpy(), counts["cf"].cpu().numpy())
    return m, dz, n


# ---- past 2^31 elements: data drawn and compared on the device -----------------------------------------------------------------------------------
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
