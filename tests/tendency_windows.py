"""What tests/test_tendency_windows_ref.py (CPU), tests/gpu_harness.py and the GPU tests of the tendencies share: ONE table of the seven
tendency kernels -- the centred, WENO5 x/y and all-WENO tracer tendencies, the vector-invariant momentum tendency, its form with the
WENO5-upwinded vorticity term and the one upwinded in every term, the free-surface sub-step -- with each one's library, symbol, array list
and numpy reference; the two cut-outs of a problem (rows, planes) with the shifted count planes; the levels of an all-WENO plane window that
agree with the column; the whole-array comparison on integer views; and a host mirror of the index arithmetic of the five 3-D kernels of
one launch (walk; SMALLEST has their smallest shapes and the free surface's).

A problem is a dict of arrays by the names of the table.  Everything here only indexes, so it works alike on numpy arrays and on torch
tensors, on any device: the GPU tests cut the very tensors the big call ran on."""
import numpy as np

import advection_ref
import free_surface_ref
import momentum_ref
import weno_momentum_ref
import weno_ref
import weno_vi_ref
import weno_xyz_ref
from vorticity_ref import same_bits

F32, F64 = np.float32, np.float64
SENTINEL = 12345.0
MASK_VALUE = 0.1                                   # not representable: converted once to the field type
DTAU, GRAVITY = 0.3, 9.80665                       # the free-surface sub-step's scalars; no averaging (weight unused)


class Kernel:
    """One row of the adapter table.  fields: 3-D parents of Nz + 2 Hz planes; tall: of Nz + 1 + 2 Hz; planes: 2-D padded planes; signed:
    the arrays drawn in [-1, 1] (every other one in [0.5, 2]); column: (name, entries beyond Nz) of the per-level vector; counts: the
    (Ny, Nx) int32 planes of the fused mask; outputs: what the call writes (out_rank 3: parents, 2: planes); arm: the halo the rule needs;
    centred_in_z: every level reads k - 1 .. k + 1 only; scheme_arg: the entry point takes a `scheme` after the mask value; jt, share: for
    walk(); ref(h, size, halo, masked) -> {output: whole array from a sentinel-filled one}."""

    def __init__(self, name, library, symbol, fields, tall, planes, signed, column, counts, outputs, out_rank, arm, centred_in_z, scheme_arg,
                 jt, share, ref):
        self.name, self.library, self.symbol = name, library, symbol
        self.fields, self.tall, self.planes, self.signed, self.column, self.counts = fields, tall, planes, signed, column, counts
        self.outputs, self.out_rank, self.arm, self.centred_in_z, self.scheme_arg = outputs, out_rank, arm, centred_in_z, scheme_arg
        self.jt, self.share, self.ref = jt, share, ref

    def __repr__(self):
        return self.name

    @property
    def has_levels(self):
        return bool(self.fields)

    def inputs(self):
        return (*self.fields, *self.tall, *self.planes, self.column[0])


def _sentinel_like(a):
    return np.full(a.shape, SENTINEL, a.dtype)


def _tracer_ref(module):
    def ref(h, size, halo, masked):
        with np.errstate(all="ignore"):
            return {"G": module.tendency(h["c"], h["u"], h["v"], h["w"], _sentinel_like(h["c"]), h["dy_fc"], h["dx_cf"], h["az_cc"], h["dz_c"], size,
                                         halo, h["n_cc"] if masked else None, MASK_VALUE)}
    return ref


def _momentum_ref(module, arrays):
    spacing = arrays["column"][0]                      # dz_f, or dz_c for the tendency upwinded in every term

    def ref(h, size, halo, masked):
        n = (h["n_fc"], h["n_cf"]) if masked else (None, None)
        with np.errstate(all="ignore"):
            Gu, Gv = module.tendencies(h["u"], h["v"], h["w"], _sentinel_like(h["u"]), _sentinel_like(h["u"]),
                                       {k: h[k] for k in momentum_ref.METRICS}, h[spacing], size, halo, *n, MASK_VALUE)
        return {"Gu": Gu, "Gv": Gv}
    return ref


def _free_surface_ref(h, size, halo, masked):
    n = (h["n_fc"], h["n_cf"]) if masked else (None, None)
    outs, _ = free_surface_ref.substep([_sentinel_like(h["eta"])] * 3, (h["eta"], h["U"], h["V"]), (h["GU"], h["GV"]),
                                       {k: h[k] for k in free_surface_ref.METRICS}, h["depth"], size, halo[0], halo[1], DTAU, GRAVITY, *n)
    return dict(zip(("eta_out", "U_out", "V_out"), outs))


_TRACER = dict(fields=("c", "u", "v"), tall=("w",), planes=("dy_fc", "dx_cf", "az_cc"), signed=("c", "u", "v", "w"), column=("dz_c", 0),
               counts=("n_cc",), outputs=("G",), out_rank=3)
_MOMENTUM = dict(fields=("u", "v"), tall=("w",), planes=momentum_ref.METRICS, signed=("u", "v", "w"), column=("dz_f", 1),
                 counts=("n_fc", "n_cf"), outputs=("Gu", "Gv"), out_rank=3)
_UPWINDED = dict(_MOMENTUM, column=("dz_c", 0))        # upwinded in every term: the spacings of the centres
# jt: rows per work item by element size, share: the form with a chunk past the row's end -- the kernels' compile-time defaults, for walk()
KERNELS = {k.name: k for k in (
    Kernel("advection", "advection", "tpg_tracer_advection_tendency", arm=(1, 1, 1), centred_in_z=True, scheme_arg=True, jt={8: 2, 4: 2},
           share=False, ref=_tracer_ref(advection_ref), **_TRACER),
    Kernel("weno", "weno", "tpg_weno_tracer_advection_tendency", arm=(3, 3, 1), centred_in_z=True, scheme_arg=False, jt={8: 2, 4: 2},
           share=True, ref=_tracer_ref(weno_ref), **_TRACER),
    Kernel("weno_xyz", "weno_xyz", "tpg_weno_xyz_tracer_advection_tendency", arm=(3, 3, 1), centred_in_z=False, scheme_arg=False,
           jt={8: 2, 4: 2}, share=True, ref=_tracer_ref(weno_xyz_ref), **_TRACER),
    Kernel("momentum", "momentum", "tpg_momentum_advection_tendency", arm=(1, 1, 1), centred_in_z=True, scheme_arg=True, jt={8: 1, 4: 2},
           share=False, ref=_momentum_ref(momentum_ref, _MOMENTUM), **_MOMENTUM),
    Kernel("weno_momentum", "weno_momentum", "tpg_weno_momentum_advection_tendency", arm=(3, 3, 1), centred_in_z=True, scheme_arg=False,
           jt={8: 2, 4: 2}, share=False, ref=_momentum_ref(weno_momentum_ref, _MOMENTUM), **_MOMENTUM),
    Kernel("weno_vi", "weno_vi", "tpg_weno_vi_momentum_advection_tendency", arm=(3, 3, 1), centred_in_z=False, scheme_arg=False,
           jt={8: 1, 4: 1}, share=False, ref=_momentum_ref(weno_vi_ref, _UPWINDED), **_UPWINDED),
    Kernel("free_surface", "free_surface", "tpg_free_surface_substep", fields=(), tall=(), planes=("eta", "U", "V", "GU", "GV") + free_surface_ref.METRICS,
           signed=("eta", "U", "V", "GU", "GV"), column=("depth", 1), counts=("n_fc", "n_cf"), outputs=("eta_out", "U_out", "V_out"), out_rank=2,
           arm=(1, 1, 0), centred_in_z=True, scheme_arg=False, jt={8: 2, 4: 2}, share=False, ref=_free_surface_ref))}
WITH_LEVELS = tuple(k for k in KERNELS.values() if k.has_levels)


# ---- shapes and drawn problems ---------------------------------------------------------------------------------------------------------------
def shape_of(kernel, name, size, halo):
    """the shape of the array `name` of a problem (size, halo); the free surface's halo is (Hx, Hy2, 0)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    plane = (Ny + 2 * Hy, Nx + 2 * Hx)
    if name in kernel.counts:
        return (Ny, Nx)
    if name == kernel.column[0]:
        return (Nz + kernel.column[1],)
    if name in kernel.tall:
        return (Nz + 1 + 2 * Hz, *plane)
    if name in kernel.fields or (name in kernel.outputs and kernel.out_rank == 3):
        return (Nz + 2 * Hz, *plane)
    assert name in kernel.planes or name in kernel.outputs, name
    return plane


def draw(kernel, size, halo, dtype, seed=0):
    """host arrays random in EVERY cell, halos included: the signed ones in [-1, 1], metrics and spacings in [0.5, 2]; counts in 0 .. Nz with
    a land column, an open one, one above Nz and a negative one planted where the plane has room"""
    Nx, Ny, Nz = size
    rng = np.random.default_rng([seed, *size, *halo, np.dtype(dtype).itemsize, len(kernel.name)])
    h = {}
    for name in kernel.inputs():
        lo, hi = (-1, 1) if name in kernel.signed else (0.5, 2)
        h[name] = rng.uniform(lo, hi, shape_of(kernel, name, size, halo)).astype(dtype)
    for name in kernel.counts:
        n = rng.integers(0, Nz + 1, (Ny, Nx)).astype(np.int32)
        n[0, 0], n[Ny - 1, Nx - 1] = Nz, 0
        if Ny * Nx >= 8:
            n[Ny - 1, 0], n[0, Nx - 1] = Nz + 3, -2
        h[name] = n
    for a in h.values():
        a.setflags(write=False)
    return h


def interior(kernel, a, size, halo):
    """the interior of an output (or of any parent or plane of the problem)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return a[..., Hy:Hy + Ny, Hx:Hx + Nx] if a.ndim == 2 else a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]


# ---- the two cut-outs ------------------------------------------------------------------------------------------------------------------------
def row_cut(kernel, h, size, halo, lo, rows):
    """the problem of the interior rows lo + 1 .. lo + rows (1-based): rows lo .. lo + rows + 2 Hy (0-based padded) of every parent and
    plane, rows lo .. lo + rows of the count planes, the per-level vector whole.  Returns (cut, its size)."""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert 0 <= lo and lo + rows <= Ny and rows >= 1
    cut = {}
    for name, a in h.items():
        if name in kernel.counts:
            cut[name] = a[lo:lo + rows]
        elif name == kernel.column[0]:
            cut[name] = a
        else:
            cut[name] = a[..., lo:lo + rows + 2 * Hy, :]
    return cut, (Nx, rows, Nz)


def shift_counts(n, a, nz):
    """the count plane of the plane window that starts at level `a` (1-based) and has nz levels: level k of the column is level k - (a - 1)
    of the window, masked there iff k - (a - 1) <= clip(n - (a - 1), 0, nz)"""
    return (n - (a - 1)).clip(0, nz)


def plane_cut(kernel, h, size, halo, a, b):
    """the problem of the levels a .. b (1-based) of a 3-D kernel: the contiguous planes a - Hz .. b + Hz of the fields, a - Hz .. b + 1 + Hz
    of w, the entries a .. b of dz_c (the faces a .. b + 1 of dz_f), the 2-D planes whole, the counts shifted.  Returns (cut, its size)."""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert kernel.has_levels and 1 <= a <= b <= Nz
    nz = b - a + 1
    cut = {}
    for name, x in h.items():
        if name in kernel.fields:
            cut[name] = x[a - 1:b + 2 * Hz]
        elif name in kernel.tall:
            cut[name] = x[a - 1:b + 1 + 2 * Hz]
        elif name == kernel.column[0]:
            cut[name] = x[a - 1:b + kernel.column[1]]
        elif name in kernel.counts:
            cut[name] = shift_counts(x, a, nz)
        else:
            cut[name] = x
    return cut, (Nx, Ny, nz)


def levels_that_agree(kernel, a, b, Nz):
    """the levels (1-based, of the column) on which the plane window a .. b gives what the column gives.  A kernel that is centred in z
    reads k - 1 .. k + 1 at level k, all inside the window's planes: every level.  The all-WENO tendency chooses a z-face's order by its
    distance to the nearer WALL, and a window has walls of its own: a level agrees iff its bottom and its top face have the same
    weno_xyz_ref.face_order in the window as in the column (the same order reads the same cells: a centred face is a wall face in both)."""
    if kernel.centred_in_z:
        return list(range(a, b + 1))
    nz = b - a + 1
    same = lambda f: weno_xyz_ref.face_order(f - (a - 1), nz) == weno_xyz_ref.face_order(f, Nz)      # noqa: E731
    return [k for k in range(a, b + 1) if same(k) and same(k + 1)]


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------------
def _ints(t):
    import torch
    return t.view({8: torch.int64, 4: torch.int32}[t.element_size()])


def equal_bits(a, b):
    """whole arrays, bit for bit on integer views: torch tensors on any device by torch.equal (no NaN is equal to another pattern of NaN:
    both sides come from the same kernel), numpy arrays by same_bits (NaNs by NaN-ness: one side is numpy's)"""
    if isinstance(a, np.ndarray):
        return same_bits(a, b) == 0
    assert a.shape == b.shape and a.dtype == b.dtype
    return bool(__import__("torch").equal(_ints(a), _ints(b)))


# ---- a host mirror of the kernels' index arithmetic ---------------------------------------------------------------------------------------------
def chunk_form(size, halo, dtype, offset=0):
    """(W, gen) as chunk_plan chooses them: 16-B chunks, plain where Hx, Nx and every pointer sit on the 16-B grid; Float32 8-B chunks
    where Nx = 2 mod 4"""
    wmax = 16 // np.dtype(dtype).itemsize
    if halo[0] % wmax == 0 and size[0] % wmax == 0 and offset == 0:
        return wmax, False
    return (wmax if size[0] % wmax == 0 else 2), True


def walk(kernel, size, halo, dtype, offset=0):
    """Every address a launch of `kernel` touches, from a mirror of its ro / rc / eo tables, e0, j0 and its clamps (interior-relative
    0-based rows, columns and planes; row -1 is the first south halo row).  Returns (violations, facts): the accesses outside their array
    -- a read outside the padded parent or the count plane, a store outside the interior --, and {"W", "gen", "share", "cpr", "items",
    "stores": how often each interior cell of a level is stored (Ny, Nx)}."""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert kernel.has_levels
    W, gen = chunk_form(size, halo, dtype, offset)
    JT, A = kernel.jt[np.dtype(dtype).itemsize], kernel.arm[0]
    share = kernel.share and Hx >= W
    cpr, tiles = Nx // W, -(-Ny // JT)
    bad, stores = [], np.zeros((Ny, Nx), int)

    def see(what, rows, cols, planes=(0,), top=Nz):
        for r in rows:
            for c in cols:
                for p in planes:
                    if not (-Hy <= r < Ny + Hy and -Hx <= c < Nx + Hx and -Hz <= p < top + Hz):
                        bad.append((what, p, r, c))

    chunk = lambda e0: range(e0, e0 + W)                                                                                        # noqa: E731
    for tile in range(tiles):
        j0 = tile * JT
        nr = min(JT, Ny - j0)
        for ch in range(cpr + (1 if share else 0)):
            past, e0 = ch == cpr, ch * W
            ro = [j0 + min(r, nr) for r in range(0, JT + 1)]                               # the tile's rows and the one north of them
            east = chunk(e0) if share else range(e0, e0 + W + 1)                           # the plain forms read one element east
            if kernel.fields[0] == "c":                                                    # ---- the tracer tendencies
                see("u, dy_fc", ro[:JT], east, range(Nz))
                see("v, dx_cf", ro, chunk(e0), range(Nz))
                see("az_cc", ro[:JT], chunk(e0))
                see("w", ro[:JT], chunk(e0), range(Nz + 1), Nz + 1)
                if A == 1:
                    crows, ccols = [j0 - 1, *ro], range(e0 - 1, e0 + W + 1)
                else:
                    NE = (W if share else W + 1) + 2 - W
                    eo = [0 if past and W + s > 2 else W + s for s in range(NE)]            # past the end: beyond element 2, its own first column
                    crows = [j0 + min(r, nr + 2) for r in range(-3, JT + 3)]
                    ccols = [*range(e0 - 3, e0 + W), *(e0 + x for x in eo)]
                cplanes = {-1, 0, min(1, Nz), min(2, Nz), *(min(k + 3, Nz) for k in range(Nz))} if not kernel.centred_in_z else range(-1, Nz + 1)
                see("c", crows, ccols, cplanes)
            else:                                                                          # ---- the momentum tendencies
                rows = [j0 + min(r, nr + A - 1) for r in range(-A, JT + A)] if A == 3 else [j0 + min(r, nr) for r in range(-1, JT + 1)]
                cols = range(e0 - A, e0 + W + A) if A == 3 else range(e0 - 1, e0 + W + 1)
                see("u, v, the metrics", rows, cols, range(-1, Nz + 1))
                see("w", rows, cols, range(Nz + 1), Nz + 1)
            for r in range(JT):                                                            # the counts: no halo, clamped onto the last row / column 0
                nrow, ncol = j0 + min(r, nr - 1), (0 if past else e0)
                if not (0 <= nrow < Ny and 0 <= ncol and ncol + W <= Nx):
                    bad.append(("counts", 0, nrow, ncol))
            if not past:                                                                   # (lane 63 of a wave of the SHARE form stores nothing: another lane has its chunk)
                for r in range(nr):
                    if 0 <= j0 + r < Ny and 0 <= e0 and e0 + W <= Nx:
                        stores[j0 + r, e0:e0 + W] += 1
                    else:
                        bad.append(("store", 0, j0 + r, e0))
    return bad, {"W": W, "gen": gen, "share": share, "cpr": cpr, "items": tiles * (cpr + (1 if share else 0)), "stores": stores}


# ---- the cases both files use -------------------------------------------------------------------------------------------------------------------
def b1_windows(kernel, Nz, k31):
    """the three plane windows (a, b), 1-based, of the tests past 2^31 elements; k31: the level of the first interior cell at or past 2^31.
    Four levels for the kernels centred in z -- the bottom four, k31 - 1 .. k31 + 2, the top four --; ten for the all-WENO tendency, placed
    so that the middle window's agreeing levels are the same four (tests/test_tendency_windows_ref.py holds that)."""
    n = 4 if kernel.centred_in_z else 10
    first = k31 - 1 if kernel.centred_in_z else k31 - 4
    assert 1 <= first and first + n - 1 <= Nz
    return {"bottom": (1, n), "middle": (first, first + n - 1), "top": (Nz - n + 1, Nz)}


def band_layouts(Ny, Hy):
    """(first interior row 0-based, rows) of the bands of the two layouts: three equal bands; a band of exactly Hy rows (the thinnest
    check_geom admits) beside one of Hy + 1 rows, and the rest"""
    assert Ny % 3 == 0 and 2 * Hy + 1 < Ny
    return {"three": [(b * (Ny // 3), Ny // 3) for b in range(3)], "thin": [(0, Hy), (Hy, Hy + 1), (2 * Hy + 1, Ny - 2 * Hy - 1)]}


_H1 = [((2, 1, 1), (1, 1, 1)), ((2, 2, 2), (1, 1, 1)), ((4, 1, 3), (1, 1, 1))]
_H3 = [((4, 3, 1), (3, 3, 1)), ((4, 3, 2), (3, 3, 1)), ((6, 3, 4), (3, 3, 1)), ((4, 4, 5), (4, 4, 4))]
_XYZ = _H3 + [((nx, ny, nz), halo) for (nx, ny), halo in (((4, 3), (3, 3, 1)), ((6, 3), (3, 3, 1)), ((4, 4), (4, 4, 4))) for nz in (1, 2, 5)
              if ((nx, ny, nz), halo) not in _H3]
# the smallest shapes check_geom admits, per kernel: Nx = 2 = one 8-B / 16-B chunk, one row (nr = 1 < JT), Nx = Hx and Ny = Hy for the WENO
# arms, (4, 4, 5) at halo 4 the SHARE form with one chunk per row in Float32.  The free surface refuses Ny = 1: its smallest is (2, 2, 1).
SMALLEST = {"advection": _H1, "momentum": _H1, "weno": _H3, "weno_momentum": _H3, "weno_xyz": _XYZ, "free_surface": [((2, 2, 1), (1, 1, 0))]}
