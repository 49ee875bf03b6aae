"""Plain high-precision reference of the two geometry utilities, written FROM THE REFERENCE'S JULIA TEXT -- compute_nonorthogonality_angle!
(test/test_tripolar_grid.jl:8-34, the output array of :64, the launch of :70) and convert_to_latlong_frame / convert_to_native_frame
(examples/convert_to_latlong_frame.jl:12-55) -- and not from the oracle's C or the kernels, so that an error the two of them share (a wrong
neighbour, a sign, dx for dy) does not pass.  Whole-array numpy, no tiles, no chunks, no level loop.

Arithmetic: np.longdouble where it is the x87 80-bit format (64-bit significand, nmant = 63); elsewhere mpmath at 40 digits, element by element
(the shapes the tests use are small); with neither, an error.  Inputs are the STORED grid arrays (Float32 or Float64): promoting them is exact,
so the reference answers "what do these stored numbers give", which is what the kernels compute in Float64 (angle) or in the grid's type (frame).

Arrays are the padded parents, A[j + Hy - 1, i + Hx - 1] = the reference's A[i, j] (fields: [k + Hz - 1, j + Hy - 1, i + Hx - 1]).

Tolerances (derived from the arithmetic of a Float64 / element-type evaluation, not from any implementation's output):
  angle   every Cartesian component of a node is a product of two sincosd results, each under 1 ulp: <= about 3 * 2^-53 absolute; a chord
          component (a difference of two) <= about 6.5 * 2^-53; the cosine dot(v1, v2) / (|v1| |v2|) then errs by <= about
          11.3 * 2^-53 * (1/|v1| + 1/|v2|) plus a few ulp; acos magnifies by 1 / sqrt(1 - c^2).  Asserted:
              tol = 16 * 2^-52 * (1/|v1| + 1/|v2|) / sqrt(1 - c^2) * 180/pi + 2 * 2^-52 * 90   degrees   (about 2.8 x the bound)
          on the nodes with |v1| > 0, |v2| > 0 and 1 - c^2 > 1e-6 (`valid`); the forced zeros (i = Nx, j = Ny, immersed) are exact: tol = 0.
  frame   at most about nine roundings reach an output, each relative to |u| + |v| (|d1|, |d2| <= 1):
              |got - want| <= 16 * eps(T) * (|u| + |v|)   per cell   (about 1.8 x the bound)
          where the reference is finite; where it is not (dx_cc = 0: the two pole cells of row Ny when Nx = 2 mod 4) the class must agree."""
import numpy as np

_LD = np.finfo(np.longdouble).nmant >= 63
try:
    import mpmath as _mp
except ImportError:                                      # pragma: no cover
    _mp = None

ANGLE_FACTOR, ANGLE_FLOOR_ULPS, FRAME_FACTOR = 16.0, 2.0, 16.0


class _LongDouble:
    name = "longdouble"
    pi = np.longdouble("3.14159265358979323846264338327950288")

    def __init__(self):
        assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not an extended format on this platform"

    @staticmethod
    def lift(a):
        return np.asarray(a).astype(np.longdouble)       # exact for Float32 / Float64

    sin, cos, sqrt, arccos = staticmethod(np.sin), staticmethod(np.cos), staticmethod(np.sqrt), staticmethod(np.arccos)
    # the grid build's functions (tests/grid_ref.py)
    tan, arctan, arcsin = staticmethod(np.tan), staticmethod(np.arctan), staticmethod(np.arcsin)
    arcsinh, sinh, cosh = staticmethod(np.arcsinh), staticmethod(np.sinh), staticmethod(np.cosh)

    @staticmethod
    def div(a, b):
        with np.errstate(divide="ignore", invalid="ignore"):
            return a / b

    @staticmethod
    def lower(a):
        return a                                          # stays long double


class _MPMath:
    name = "mpmath"

    def __init__(self):
        _mp.mp.dps = 40
        self.pi = +_mp.pi
        f = lambda fn: np.frompyfunc(fn, 1, 1)
        nan_safe = lambda fn: (lambda x: x if _mp.isnan(x) else fn(x))
        self.sin, self.cos = f(_mp.sin), f(_mp.cos)
        self.sqrt = f(nan_safe(lambda x: _mp.sqrt(x) if x >= 0 else _mp.nan))
        self.arccos = f(nan_safe(lambda x: _mp.acos(x) if abs(x) <= 1 else _mp.nan))
        self.tan, self.arctan, self.arcsinh, self.sinh, self.cosh = f(_mp.tan), f(_mp.atan), f(_mp.asinh), f(_mp.sinh), f(_mp.cosh)
        self.arcsin = f(nan_safe(lambda x: _mp.asin(x) if abs(x) <= 1 else _mp.nan))

        def div(a, b):                                    # IEEE classes for x / 0, as the long-double path gives
            if _mp.isnan(a) or _mp.isnan(b):
                return _mp.nan
            if b == 0:
                return _mp.nan if a == 0 else (_mp.inf if a > 0 else -_mp.inf)
            if _mp.isinf(a) and _mp.isinf(b):
                return _mp.nan
            return a / b
        self.div = np.frompyfunc(div, 2, 1)

    @staticmethod
    def lift(a):
        return np.frompyfunc(lambda x: _mp.mpf(float(x)), 1, 1)(np.asarray(a, dtype=np.float64))    # Float32 -> Float64 -> mpf: exact

    @staticmethod
    def lower(a):
        return np.asarray(a, dtype=object).astype(np.float64)


def backend(name=None):
    """the arithmetic: long double where it has a 64-bit significand, else mpmath, else an error (`name` forces one: the tests run both)"""
    if name == "longdouble" or (name is None and _LD):
        return _LongDouble()
    if _mp is not None and name in (None, "mpmath"):
        return _MPMath()
    raise RuntimeError("geometry_ref needs a np.longdouble with a 64-bit significand (x87 extended) or mpmath; this platform has "
                       f"nmant = {np.finfo(np.longdouble).nmant} and no mpmath")


def angle_ref(lambda_ff, phi_ff, size, halo, immersed=None, arith=None):
    """-> (angle, tol, valid), each (Ny, Nx): the angle in degrees between the chords node (i, j) -> (i+1, j) and (i, j) -> (i, j+1),
    minus 90; 0 at i = Nx, at j = Ny (zeros(size(grid)...), launched over (Nx-1, Ny-1)) and where `immersed` is set.  `tol` is the per-node
    tolerance (inf where it does not hold) and `valid` the nodes it holds on (module docstring)."""
    B = backend(arith)
    (Nx, Ny), (Hx, Hy) = size[:2], halo[:2]
    assert lambda_ff.shape == phi_ff.shape == (Ny + 2 * Hy, Nx + 2 * Hx)
    # nodes (1..Nx, 1..Ny): everything the launch over (Nx-1, Ny-1) reads, and no halo cell
    lam = B.lift(lambda_ff[Hy:Hy + Ny, Hx:Hx + Nx]) * B.pi / 180
    phi = B.lift(phi_ff[Hy:Hy + Ny, Hx:Hx + Nx]) * B.pi / 180
    P = (B.cos(lam) * B.cos(phi), B.sin(lam) * B.cos(phi), B.sin(phi))          # lat_lon_to_cartesian(phi, lambda, 1)
    v1 = [c[:-1, 1:] - c[:-1, :-1] for c in P]                                   # (i+1, j) - (i, j)   (:23)
    v2 = [c[1:, :-1] - c[:-1, :-1] for c in P]                                   # (i, j+1) - (i, j)   (:24)
    n1 = B.sqrt(v1[0] * v1[0] + v1[1] * v1[1] + v1[2] * v1[2])
    n2 = B.sqrt(v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2])
    cs = B.div(v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2], n1 * n2)          # :27
    with np.errstate(invalid="ignore"):
        ang = (B.arccos(cs) - B.pi / 2) * 180 / B.pi                             # :29, :32
    n1, n2, cs, ang = (B.lower(a) for a in (n1, n2, cs, ang))
    with np.errstate(divide="ignore", invalid="ignore"):
        s2 = 1 - cs * cs
        ok = (n1 > 0) & (n2 > 0) & (s2 > 1e-6)
        t = (ANGLE_FACTOR * 2.0 ** -52 * (1 / n1 + 1 / n2) / np.sqrt(np.where(ok, s2, 1)) * (180 / np.pi) + ANGLE_FLOOR_ULPS * 2.0 ** -52 * 90)
    angle = np.zeros((Ny, Nx), dtype=ang.dtype)
    tol = np.zeros((Ny, Nx), dtype=np.float64)
    valid = np.ones((Ny, Nx), dtype=bool)
    angle[:-1, :-1], tol[:-1, :-1], valid[:-1, :-1] = ang, np.where(ok, t, np.inf).astype(np.float64), ok
    if immersed is not None:
        m = np.asarray(immersed).astype(bool)
        assert m.shape == (Ny, Nx)
        angle[m], tol[m], valid[m] = 0, 0, True                                  # ifelse(immersed, pi/2, ...) - pi/2  (:29)
    return angle, tol, valid


def frame_ref(grid_arrays, u, v, size, halo, to_native, arith=None):
    """-> (u_out, v_out, scale), each the (Nz, Ny, Nx) interior: the rotation of the example, cell by cell, and scale = |u| + |v|.
    grid_arrays: dict with the padded phi_cf, phi_fc, dy_cc, dx_cc; u, v: padded (Center, Center, Center) parents."""
    B = backend(arith)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    assert Hx >= 1 and Hy >= 1 and u.shape == v.shape == (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    win = lambda name, dj, di: B.lift(grid_arrays[name][Hy + dj:Hy + dj + Ny, Hx + di:Hx + di + Nx])
    ut = B.div((win("phi_cf", 1, 0) - win("phi_cf", 0, 0)) * B.pi / 180, win("dy_cc", 0, 0))       # :14-18
    vt = -B.div((win("phi_fc", 0, 1) - win("phi_fc", 0, 0)) * B.pi / 180, win("dx_cc", 0, 0))      # :20-24
    U = B.sqrt(ut * ut + vt * vt)                                                                   # :26
    d1, d2 = B.div(ut, U), B.div(vt, U)                                                             # :28-29
    uo = B.lift(u[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx])
    vo = B.lift(v[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx])
    if to_native:
        x, y = uo * d1 + vo * d2, uo * d2 - vo * d1                                                 # :54
    else:
        x, y = uo * d1 - vo * d2, uo * d2 + vo * d1                                                 # :31
    return B.lower(x), B.lower(y), B.lower(abs(uo) + abs(vo))


def frame_tolerance(scale, dtype):
    return FRAME_FACTOR * float(np.finfo(dtype).eps) * scale


# ---- the shapes both suites use (tests/test_oracle_geometry.py holds the oracle to this module at them, tests/test_gpu_geometry.py the kernels)
# angle: k_nonorthogonality tiles 64 x 8 nodes = 63 x 7 cells per block: Nx and Ny on both sides of one and of two tile edges, plus two sizes
# with a partial third / fourth / sixth block row
ANGLE_SIZES = [(62, 7), (64, 8), (126, 14), (128, 15), (128, 22), (130, 36)]
ANGLE_HALOS = [(4, 4, 4), (5, 5, 5), (3, 2, 1), (1, 1, 1)]
# frame rotation, ((Nx, Ny), halo): the aligned 16-B form; LOOSE by an odd Hx; Nx = 2 mod 4 (the Float32 scalar kernel, Float64 16-B chunks of 2) at
# an odd and at an element-aligned halo; no z halo; and (Nx / W) * Ny = 450 / 900 threads: more than one block of 256 and a partial last one
FRAME_GEOMS = [((64, 12), (4, 4, 2)), ((64, 12), (5, 5, 5)), ((66, 12), (5, 5, 5)), ((66, 12), (3, 2, 1)), ((62, 9), (5, 5, 5)),
               ((62, 9), (3, 2, 1)), ((130, 20), (1, 1, 0)), ((600, 3), (4, 3, 2))]
FRAME_NZ = [1, 3, 4, 5, 16, 17, 21]            # the 4-level unrolled loop, its tail, and a second group of 16 levels


def frame_levels(geom):
    """the level counts a geometry is run at: all of FRAME_NZ, but 2 only for the partial-block geometry (600, 3, 2)"""
    return [2] if geom[0] == (600, 3) else FRAME_NZ


def frame_inputs(size, halo, dtype):
    """the two padded parents of one case, reproducible: uniform in (-1, 1) times a power of ten per cell (1e-3 .. 1e3), so that the tolerance is
    exercised as a RELATIVE one; halo cells hold data of their own (a kernel that read them would differ from the reference)"""
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng([Nx, Ny, Nz, Hx, Hy, Hz, np.dtype(dtype).itemsize])
    shape = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    u = (rng.uniform(-1, 1, shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(dtype)
    v = (rng.uniform(-1, 1, shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(dtype)
    return u, v


def angle_mask(size):
    """a dense (Ny, Nx) byte plane: about a fifth of the cells set, with values other than 1 among them (the test is `!= 0`), and both sides of
    the first tile edge (columns 62 .. 64, rows 6 .. 8) set in part"""
    Nx, Ny = size[:2]
    rng = np.random.default_rng([Nx, Ny, 77])
    m = np.where(rng.random((Ny, Nx)) < 0.2, rng.choice(np.array([1, 2, 128, 255], dtype=np.uint8), (Ny, Nx)), 0).astype(np.uint8)
    m[min(6, Ny - 1), :Nx:2] = 1
    m[::2, min(62, Nx - 1)] = 255
    return m
