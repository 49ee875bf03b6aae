"""The IEEE special-value cases shared by tests/test_special_value_refs.py (CPU: the numpy references against exact rational arithmetic)
and tests/test_gpu_special_values.py (GPU: the kernels against the numpy references).  Everything is a function of the element type.

POOL: 19 values -- +-0, +-smallest subnormal, largest subnormal, +-smallest normal, 0.3 * smallest normal (a subnormal with a rounded
mantissa), +-1, 1.5, 1/3, 1e3, +-max, 0.75 * max, +-Inf, NaN.  The Value / Gradient cases put every ordered (source cell, condition) pair
of POOL x POOL (361) through the rule with each spacing of SPACINGS; the timescale cases are the rows of timescale_rows."""
import numpy as np


def pool(dtype):
    fi = np.finfo(dtype)
    sub, tiny, big = fi.smallest_subnormal, fi.tiny, fi.max
    lsub = np.nextafter(tiny, dtype(0))
    vals = [0.0, -0.0, sub, -sub, lsub, tiny, -tiny, dtype(0.3) * tiny, 1.0, -1.0, 1.5, dtype(1) / dtype(3), 1e3, big, -big,
            dtype(0.75) * big, np.inf, -np.inf, np.nan]
    out = np.array(vals, dtype=dtype)
    assert out.size == 19 and np.signbit(out[1]) and out[2] > 0 and out[4] < tiny and out[7] < tiny
    return out


def spacings(dtype):
    """1; 3e4 (a metric); the smallest subnormal (d / 2 rounds to 0); 4 * the smallest normal; max / 2"""
    fi = np.finfo(dtype)
    return np.array([1.0, 3e4, fi.smallest_subnormal, dtype(4) * fi.tiny, fi.max / dtype(2)], dtype=dtype)


def pairs(dtype):
    """(source, condition): the 361 ordered pairs of the pool, source varying slowest"""
    p = pool(dtype)
    return np.repeat(p, p.size), np.tile(p, p.size)


def tiled(values, shape):
    """`values` repeated in order over an array of `shape` (C order), which must hold them all at least once"""
    n = int(np.prod(shape))
    assert n >= values.size, (n, values.size)
    return np.resize(values, n).reshape(shape).copy()


def timescale_rows(dtype):
    """[(name, cell)]: the operands planted at ONE cell -- u, v, w and the spacings dx, dy of its column and dz of its level; every other
    velocity is +0 and every other spacing 1.  The second half is the first through w and dz."""
    fi = np.finfo(dtype)
    sub, tiny, big = fi.smallest_subnormal, fi.tiny, fi.max
    lsub = np.nextafter(tiny, dtype(0))
    big34 = dtype(0.75) * big
    base = dict(u=0.0, v=0.0, w=0.0, dx=1.0, dy=1.0, dz=1.0)
    horizontal = [("smallest subnormal over 1", dict(u=sub)),
                  ("largest subnormal over 1", dict(u=lsub)),
                  ("0.3 smallest normal over 1", dict(u=dtype(0.3) * tiny)),
                  ("max over smallest normal", dict(u=big, dx=tiny)),
                  ("0 over 0", dict(u=0.0, dx=0.0)),
                  ("Inf over Inf", dict(u=np.inf, dx=np.inf)),
                  ("1 over smallest subnormal", dict(u=1.0, dx=sub))]
    rows = [(name, {**base, **c}) for name, c in horizontal]
    rows.append(("all three -0", {**base, "u": -0.0, "v": -0.0, "w": -0.0}))
    rows.append(("0.75 max + 0.75 max", {**base, "u": big34, "v": big34}))
    for name, c in horizontal:
        moved = {{"u": "w", "dx": "dz"}[k]: x for k, x in c.items()}
        rows.append((name + " (w, dz)", {**base, **moved}))
    rows.append(("0.75 max + 0.75 max (v, w)", {**base, "v": big34, "w": big34}))
    return [(name, {k: dtype(x) for k, x in c.items()}) for name, c in rows]


def timescale_arrays(cell, size, halo, at):
    """the five padded host arrays and dz of one timescale row: u, v (Nz levels), w (Nz + 1), dx, dy (2-D), dz (Nz); `at` = (k, j, i), the
    0-based interior cell that takes the operands"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    dtype = cell["u"].dtype.type
    k, j, i = at
    sy, sx = Ny + 2 * Hy, Nx + 2 * Hx
    u, v = np.zeros((Nz + 2 * Hz, sy, sx), dtype=dtype), np.zeros((Nz + 2 * Hz, sy, sx), dtype=dtype)
    w = np.zeros((Nz + 1 + 2 * Hz, sy, sx), dtype=dtype)
    dx, dy, dz = np.ones((sy, sx), dtype=dtype), np.ones((sy, sx), dtype=dtype), np.ones(Nz, dtype=dtype)
    u[Hz + k, Hy + j, Hx + i], v[Hz + k, Hy + j, Hx + i], w[Hz + k, Hy + j, Hx + i] = cell["u"], cell["v"], cell["w"]
    dx[Hy + j, Hx + i], dy[Hy + j, Hx + i], dz[k] = cell["dx"], cell["dy"], cell["dz"]
    return u, v, w, dx, dy, dz


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def same_bits_or_both_nan(got, want):
    """elementwise: the raw bits agree (signed zeros included), or both are NaN (the payload is free)"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
