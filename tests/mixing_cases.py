"""What the tests of the vertical mixing diffusivities share (tests/test_mixing_ref.py, tests/test_gpu_mixing.py): the draw of a problem of
tests/mixing_ref.py -- every array random in EVERY cell, then NaN in every input cell the header says is not read --, the sentinel-filled
outputs, and the parameters of the two closures."""
import numpy as np

import mixing_ref as R

F32, F64 = np.float32, np.float64
SENTINEL = -777.25
MASK_VALUE = -3.5
CA = dict(background_kappa=0.015625, convective_kappa=1.5, background_nu=0.03125, convective_nu=2.5)
RI = dict(nu0=0.7, kappa0=0.5, kappa_ca=1.7, Ri0=0.1, Ri_delta=0.4, Cav=0.6)


def nan_where_not_read(p):
    """NaN in every cell of b, u, v and the *_prev arrays that the header says p's outputs do not read; dz_f[1] and dz_f[Nz+1] too"""
    read = R.cells_read(p)
    for name in ("b", "u", "v"):
        if p[name] is not None:
            p[name] = np.where(read[name], p[name], np.nan).astype(p[name].dtype)
    if p["prev"] is not None:
        p["prev"] = tuple(np.where(read[n], a, np.nan).astype(a.dtype) for n, a in zip(("kappa_c_prev", "nu_c_prev"), p["prev"]))
    return p


def count_plane(size, which, seed=0):
    """an int32 (Ny, Nx) plane of counts in 0..Nz with, where there is room, a negative one and one above Nz planted"""
    Nx, Ny, Nz = size
    rng = np.random.default_rng([7, "cc fc cf".split().index(which), *size, seed])
    n = rng.integers(0, Nz + 1, (Ny, Nx)).astype(np.int32)
    n[0, 0] = -2
    n[Ny - 1, Nx - 1] = Nz + 3
    if Nx * Ny > 3:
        n[0, 1], n[Ny - 1, Nx - 2] = 0, Nz
    return n


def draw(closure, size, halo, dtype, *, prev=False, counts=(), outputs=R.OUTPUTS, seed=0, params=None, nan_unread=True):
    """(p, into): a problem of mixing_ref with b, u, v in [-1, 1], dz_f in [0.5, 2] (NaN at the faces 1 and Nz + 1), the *_prev arrays in
    [0, 2]; `counts`: the names of the count planes given, of "cc", "fc", "cf"; and the sentinel-filled parents of the outputs"""
    Nx, Ny, Nz = size
    rng = np.random.default_rng([*size, *halo, np.dtype(dtype).itemsize, seed])
    U = lambda lo, hi, s: rng.uniform(lo, hi, s).astype(dtype)     # noqa: E731
    cells, faces = R.cell_shape(size, halo), R.face_shape(size, halo)
    b, u, v = U(-1, 1, cells), U(-1, 1, cells), U(-1, 1, cells)
    dz_f = U(0.5, 2, Nz + 1)
    dz_f[0] = dz_f[Nz] = np.nan
    old = (U(0, 2, faces), U(0, 2, faces))
    ri = closure == "ri"
    p = R.problem(closure, size, halo, b, dz_f, dict(params or (RI if ri else CA)), u=u if ri else None, v=v if ri else None,
                  prev=old if ri and prev else None, counts={k: count_plane(size, k, seed) for k in counts}, mask_value=MASK_VALUE, outputs=outputs)
    into = {name: np.full(faces, SENTINEL, dtype) for name in outputs}
    return (nan_where_not_read(p) if nan_unread else p), into
