"""A third statement of the TripolarGrid metric precompute, written FROM THE REFERENCE'S JULIA TEXT (src/tripolar_grid.jl,
src/generate_tripolar_coordinates.jl, src/tripolar_grid_utils.jl, src/zipper_boundary_condition.jl, src/distributed_tripolar_grid.jl) and not
from oracle/tpg_oracle.c or the kernels, so that an error the two of them share (a wrong neighbour, a fold index, a sign of zero) does not pass.
Whole-array numpy: no tiles, no tables in LDS, no fused index maps.  The arithmetic is tests/geometry_ref.py's backend: np.longdouble where it
has a 64-bit significand, mpmath at 40 digits otherwise.

Arrays are the padded parents, A[j + Hy - 1, i + Hx - 1] = the reference's A[i, j].

Pieces
  tables       tripolar_grid.jl:90-97.  generate_coordinate(FT, ...) (:90) receives the grid's type, so the LAMBDA tables are ranges of FT: on a
               Float32 grid their elements are the exact rationals -180 + 360 (i-1)/N, -180 + 360 (2i-1)/(2N) rounded once to Float32, and
               sind / cosd of a Float32 return Float32 (the header of k_tables in csrc/tpg_grid.hip restates the same two facts).  The PHI
               tables do not see FT: collect(range(south, 90, length = N)) (:95) is Float64 on every grid, its elements the exact rationals
               rounded once (fractions.Fraction here); phi_f = phi_c .- dphi / 2 (:96-97) is evaluated in Float64.  For an integer `south`
               that is bit-equal to Julia's range; for a non-integer dyadic one (-75.5) Julia's twice-precision range is within 1 ulp of
               the correctly rounded rational, and the coordinate tolerance below allows for that ulp.
  coordinates  generate_tripolar_coordinates.jl:66-87 at the four locations; the arguments (90 - phi) / 2 and (90 - npl) / 2 are formed in
               Float64 as the reference forms them.  sind / cosd carry Julia Base's exact values at the multiples of 90 and its sign of zero
               (sind(-180) = -0.0, sind(0) = +0.0, cosd(+-90) = +0.0): on the two pole meridians x = +-0 and y / x = +-Inf, so the longitude
               is decided by that sign -- stated here as a rule (`zsign`), since neither sin(x pi / 180) in long double nor mpmath has it.
               on_the_north_pole with `i == 1` on the PRE-shift index (:74-77), the hemisphere shift i <= N/2 (:82), first_pole_longitude + 90
               (:86), convert_to_0_360 (:87), then circshift by N / 4 (tripolar_grid.jl:121-130).
  fill         zipper_boundary_condition.jl:70-138 with sign +1, then periodic x over every row (tripolar_grid.jl:147-152).  y-Center fields
               get the row-Ny substitution (:102, :135), the x-Face ones with the self-mapped cell i = N/2 + 1 and the wrap of i = 1.  The
               south halo is not written (south = nothing, :148): zero for the coordinates.
  metrics      tripolar_grid_utils.jl:13-43 from STORED Float64 coordinate interiors (lifted exactly), halo-filled by `fill`: "what do these
               stored numbers give", which is what the kernel and the reference compute.  Distances.haversine, lat_lon_to_cartesian and
               spherical_area_quadrilateral are [recalled] as tests/test_oracle_exact.py states them.
  continuation metric halo fill, then continue_south! (tripolar_grid.jl:287-300, 336-357): rows 1-Hy .. 1 of every padded column (`offsets` are
               negative and size(new_metric) is the padded size, so the loop runs over the x halos too), with the pairings of :292 (dy_ff from
               dy_fc) and :295 (dy_cc from dy_cf) -- one Number on a regular latitude.  The lat-lon formulas are Oceananigans' and not in the
               reference: [recalled], parity unpinned -- restated from the rule of DESIGN / tpg_grid.hip: dlam = 360 / Nx, dphi = (90 - south) / Ny,
               phi_f[j] = south + (j - 1) dphi, phi_c[j] = phi_f[j] + dphi / 2; dx = R rad(dlam) cos(phi) at phi_c (fc, cc) or phi_f (cf, ff);
               dy = R rad(dphi); Az = R^2 rad(dlam) (sin phi_f[j+1] - sin phi_f[j]) (fc, cc) or (sin phi_c[j] - sin phi_c[j-1]) (cf, ff).
  map(FT)      tripolar_grid.jl:308-328: the reference values stay unrounded; the Float32 tolerance carries the rounding.
  bands        rows jstart - Hy .. jend + Hy of the global padded arrays (distributed_tripolar_grid.jl:41-49): Reference.rows().

Tolerances: derived from the arithmetic of a Float64 evaluation of the same formulas (e = 2^-52), never from the oracle's or the kernel's output.
  coordinates  y / x = (cl sh) / (sl ch): sind, cosd < 1 ulp, sinh / cosh correctly rounded, two products each: 5.5 e relative, plus sinh psi = t / a
               (tand twice 2 ulp, one division: 4.5 e) and psi coth psi / 2 <= 2.2 e from the rounding of asinh (psi <= 4.3): about 12 e on
               tan(lambda), i.e. <= 6 e rad = 7.7e-14 degrees through atan (d lambda = rho sin(2 lambda) / 2); atan and the product with 180/pi
               2.6e-14; the additions of :82, :86, :87 round at 1/2 ulp of |l| <= 180, <= 340, <= 720: 1.4e-14 + 2.8e-14 + 5.7e-14.  Sum
               2.1e-13 degrees for lambda at the default parameters (first_pole_longitude = 1000.5 adds 1/2 ulp(1024) = 1.1e-13), 1.3e-13
               for phi (8 e on sqrt(x^2 + y^2), d phi <= (360/pi) rho / 2, atan, 1/2 ulp(90)); a non-integer `south` adds its table ulp,
               1.4e-14.  Asserted: COORD_TOL = 2e-13 degrees, the project's ceiling (tests/test_oracle_exact.py) -- 1.0 x the bound, lambda
               modulo 360.  South halo cells and halo copies: the value 0 exactly / the tolerance of the cell they copy.
  dx, dy       d = 2 R asin(r), r = sqrt(a), a = S1^2 + c1 c2 S2^2, S1 = sin(h_phi), S2 = sin(h_lam), h the half-angles.  Per edge (edge_tolerance):
                 dh_lam = ulp(dlam_deg) pi / 720 + ulp(dlam_rad) / 4 + e |h_lam| / 4        subtraction, product, the deg2rad constant (0.2 e)
                 dh_phi = (ulp(a1) + ulp(a2)) / 4 + ulp(a2 - a1) / 4 + e (|a1| + |a2|) / 8  two rounded radians, their difference
                 dc_k   = e c_k + |sin a_k| (ulp(a_k) / 2 + e |a_k| / 4)                    cos < 1 ulp, its rounded argument
                 tol = R [(2 w2 |cos h_lam| dh_lam + 2 w1 |cos h_phi| dh_phi + (S2^2 / r)(c2 dc1 + c1 dc2) + 5 e r) / sqrt(1 - a) + 4 e asin r]
               with w1 = |S1| / r <= 1 and w2 = c1 c2 |S2| / r <= sqrt(c1 c2) (their limits where r = 0), 5 e r the squares, products, sum and
               sqrt, 4 e asin r the asin and the two products with R.  dh_lam is the explicit half-angle term: where |dlam| > 180 (an edge across
               the 0 / 360 wrap) h_lam sits next to pi and dh_lam grows to 2.9 e = 1.3 ulp(pi), worth up to 5.8 cos(phi) e R; elsewhere the edge
               bound is about 1.3 to 1.5 e R, from dh_phi.  Asserted: 1.0 x this bound.  An edge of length zero has tol = 0.
  Az_fc, Az_cf dy tol(dx) + dx tol(dy) + e dx dy / 2.  Asserted: 1.0 x.
  Az_cc, Az_ff each triangle is 2 atan(N / D), N the triple product, D = 1 + a.b + b.c + a.c; d(2 atan) <= 2 (|D| dN + |N| dD) / (D^2 + N^2).  A
               Cartesian component is a product of two sind / cosd: 2.5 e relative; a term of N three of them and a product more: 8.5 e of at most
               0.19, six terms: dN <= 10 e in the worst case.  Asserted: e R^2 kappa, kappa = (1/2) sum over the four triangles of
               2 (|D| + |N|) / (D^2 + N^2), which is 1.0 for a small cell (D = 4): the project's ceiling e R^2 (tests/test_oracle_exact.py), 0.1 x
               the worst-case bound.  kappa differs from 1 only on the cells of rows j <= 1 that take a vertex from the zero south halo, which
               the continuation overwrites and which survive only as north halo copies where Ny <= Hy.
  rows j <= 1  dx: R rad(dlam) [3.7 cos + 3 |arg sin arg|] e; dy: 1.7 e relative; Az: R^2 rad(dlam) [sum_k (|sin_k| + 3 |arg_k cos_k|) + 3.2 |diff|] e
               (the rounded argument pi phi / 180 with phi itself 2 ulp from the rational: 3 e |arg|; sin, cos < 1 ulp; the prefactors).  1.0 x.
  Float32      half an ulp of Float32 at the reference value plus the Float64 tolerance.  The metrics of a Float32 grid come from Float64
               coordinates that the product does not store, so they are taken from this module's own coordinates rounded to Float64, and the
               tolerance adds what COORD_TOL moves them by: 2 sqrt(2) rad(COORD_TOL) R per edge, the same on both factors of a product area, and
               2 pi sqrt(2) rad(COORD_TOL) R^2 per excess area (a perimeter of at most a great circle).
  coverage     every cell of every padded parent is compared: no class is excluded.  The pole nodes (x = y = 0: two per x-Face array) have the
               finite bounds above (phi = 90 exactly, lambda by the rule of :75); so have the zero-length edges of row Ny.
  halo cells   are copies: check_halo_copies() asserts them bit for bit against `fill` applied to the product's own interior.

Measured (CPU oracle against this module, long double; worst over every case of tests/test_oracle_grid.py, the kernel being bit-identical to
the oracle): MEASURED_RATIOS below are the worst |error| / tolerance per array family on Float64 grids; on Float32 grids every family reaches
1.00 and none exceeds it (half an ulp is what a correct rounding attains).  In absolute terms: coordinates 1.5e-13 degrees at
first_pole_longitude = 1000.5 and 9.3e-14 otherwise; edges away from the wrap 1.01 e R at 360 x 180 (2.3 e R on the 90-degree edges of 4 x 5,
where the relative terms count); wrap-crossing dx edges 2.4 e R at 360 x 180, 2.7 e R over all cases; Az_cc / Az_ff 0.22 to 0.28 e R^2 on small
cells (0.80 kappa e R^2 on the coarsest grids).
"""
from fractions import Fraction

import numpy as np

from geometry_ref import backend

R_EARTH = 6371.0e3
E = 2.0 ** -52
D2R = np.pi / 180
COORD_TOL = 2e-13                # degrees
AREA_CEILING = 1.0               # e R^2 for a small cell
LOCS = {"cc": (0, 0), "fc": (1, 0), "cf": (0, 1), "ff": (1, 1)}
COORDS = tuple(p + "_" + l for p in ("lambda", "phi") for l in LOCS)
METRICS = tuple(p + "_" + l for p in ("dx", "dy", "az") for l in LOCS)
# worst |oracle - reference| / tolerance per array family over tests/test_oracle_grid.py's Float64 cases (rounded up)
MEASURED_RATIOS = {"lambda": 0.76, "lambda, first_pole_longitude within +-360": 0.47, "phi": 0.30, "dx": 0.65, "dy": 0.64, "az_fc_cf": 0.59,
                   "az_cc_ff": 0.81, "rows j <= 1": 0.36}


# ---- small backend helpers -------------------------------------------------------------------------------------------------------------
def _f64(B, a):
    return np.asarray(B.lower(a), dtype=np.float64)


def _lift_scalar(B, x):
    v = B.lift(np.asarray(float(x), dtype=np.float64))
    return v[()] if isinstance(v, np.ndarray) else v


def _mod360(B, x):
    return np.mod(x, 360) if B.name == "longdouble" else np.frompyfunc(lambda v: v % 360, 1, 1)(x)


def _round_f32(B, a):
    """sind(::Float32) returns Float32"""
    return B.lift(_f64(B, a).astype(np.float32))


def _sincosd(B, x):
    """sind, cosd of a Float64 array with Julia Base's exact values at the multiples of 90; the sign of a zero sine is returned apart
    (-1 where Julia gives -0.0: x < 0) because the arithmetic may not carry it"""
    x = np.asarray(x, dtype=np.float64)
    r = B.lift(x) * B.pi / 180
    s, c = B.sin(r) + 0 * r, B.cos(r) + 0 * r
    m180, m90 = np.fmod(x, 180) == 0, np.abs(np.fmod(x, 180)) == 90
    zero, one = _lift_scalar(B, 0), _lift_scalar(B, 1)
    sgn = lambda v: np.where(v < 0, -one, one)
    s = np.where(m180, zero, np.where(m90, sgn(np.sin(x * D2R)), s))
    c = np.where(m90, zero, np.where(m180, sgn(np.cos(x * D2R)), c))
    zsign = np.where(m180 & ((x < 0) | np.signbit(x)), -1, 1)
    return s, c, zsign


# ---- 1-D tables (tripolar_grid.jl:90-97) -----------------------------------------------------------------------------------------------
def _rn(fr, p):
    """the Fraction rounded to the nearest binary float of p significand bits, ties to even -> float"""
    if fr == 0:
        return 0.0
    sign, fr = (-1 if fr < 0 else 1), abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if Fraction(2) ** e > fr:
        e -= 1                                             # 2^e <= fr < 2^(e + 1)
    scale = Fraction(2) ** (p - 1 - e)
    q = fr * scale
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return sign * float(Fraction(n) / scale)


def tables(size, southernmost_latitude=-80, dtype=np.float64):
    """-> lam_f, lam_c (Nx), phi_f, phi_c (Ny), Float64 arrays; on a Float32 grid the lambda elements are Float32 values (module docstring)"""
    Nx, Ny = size[:2]
    p = 53 if np.dtype(dtype) == np.float64 else 24
    lam_f = np.array([_rn(Fraction(-180) + Fraction(360 * (i - 1), Nx), p) for i in range(1, Nx + 1)])
    lam_c = np.array([_rn(Fraction(-180) + Fraction(360 * (2 * i - 1), 2 * Nx), p) for i in range(1, Nx + 1)])
    S = Fraction(float(southernmost_latitude))
    phi_c = np.array([_rn(S + (90 - S) * Fraction(j - 1, Ny - 1), 53) for j in range(1, Ny + 1)])          # :95
    dphi = phi_c[1] - phi_c[0]                                                                              # :96
    phi_f = phi_c - dphi / 2                                                                                # :97
    return lam_f, lam_c, phi_f, phi_c


# ---- coordinates (generate_tripolar_coordinates.jl:66-87, tripolar_grid.jl:121-130) ------------------------------------------------------
def coordinates(size, north_poles_latitude=55, first_pole_longitude=70, southernmost_latitude=-80, dtype=np.float64, arith=None,
                substitute_row_Ny=True):
    """-> dict of the 8 (Ny, Nx) coordinate interiors AFTER the fill's row-Ny substitution (what the grid stores), unrounded;
    substitute_row_Ny=False gives the formula values of :66-87 (what the fill finds)"""
    B = backend(arith)
    Nx, Ny = size[:2]
    f32 = np.dtype(dtype) == np.float32
    lam_f, lam_c, phi_f, phi_c = tables(size, southernmost_latitude, dtype)
    a = B.tan(_lift_scalar(B, (90 - north_poles_latitude) / 2) * B.pi / 180)                               # tripolar_grid.jl:76
    i0 = np.arange(1, Nx + 1)[None, :]                                                                      # the kernel's i: before the shift
    out = {}
    for loc, (xf, yf) in LOCS.items():
        lam1, phi1 = (lam_f if xf else lam_c), (phi_f if yf else phi_c)                                     # :62-63
        psi = B.arcsinh(B.tan(B.lift((90 - phi1) / 2) * B.pi / 180) / a)                                    # :66
        sl, cl, zsign = _sincosd(B, lam1)
        if f32:
            sl, cl = _round_f32(B, sl), _round_f32(B, cl)
        x = (a * sl)[None, :] * B.cosh(psi)[:, None]                                                        # :67
        y = (a * cl)[None, :] * B.sinh(psi)[:, None]                                                        # :68
        xz, yz = np.asarray(x == 0, dtype=bool), np.asarray(y == 0, dtype=bool)
        pole = xz & yz                                                                                      # :74
        ninety = _lift_scalar(B, 90)
        ratio = y / np.where(xz, 1 + 0 * x, x)
        lam = -180 / B.pi * B.arctan(ratio)                                                                 # :77
        plus_inf = np.where(np.asarray(y < 0, dtype=bool), -1, 1) * zsign[None, :] > 0                      # y / +-0 by the sign of the zero
        lam = np.where(xz, np.where(plus_inf, -ninety, ninety), lam)                                        # -180 / pi * atan(+-Inf)
        lam = np.where(pole, np.where(i0 == 1, -ninety, ninety), lam)                                       # :75
        phi = 90 - 360 / B.pi * B.arctan(B.sqrt(y * y + x * x))                                             # :78
        lam = lam + np.where(i0 <= Nx // 2, -ninety, ninety)                                                # :82
        lam = lam + _lift_scalar(B, first_pole_longitude + 90)                                              # :86
        lam = _mod360(B, lam)                                                                               # :87
        out["lambda_" + loc] = np.roll(lam, Nx // 4, axis=1)                                                # tripolar_grid.jl:121-130
        out["phi_" + loc] = np.roll(phi + 0 * lam, Nx // 4, axis=1)
    if substitute_row_Ny:
        for name in out:
            xf, yf = LOCS[name[-2:]]
            P = _pad(out[name], size, (1, 1))
            fill(P, xf, yf, size, (1, 1))
            out[name] = P[1:-1, 1:-1]
    return out


# ---- halo fill of a sign +1 field (zipper_boundary_condition.jl:70-138, then periodic x) ---------------------------------------------------
def _pad(interior, size, halo):
    (Nx, Ny), (Hx, Hy) = size[:2], halo[:2]
    P = np.zeros((Ny + 2 * Hy, Nx + 2 * Hx), dtype=interior.dtype)
    if P.dtype == object:
        P[...] = interior.flat[0] * 0
    P[Hy:Hy + Ny, Hx:Hx + Nx] = interior
    return P


def fill(P, xface, yface, size, halo):
    """in place: the fold of the location over i = 1 .. Nx, then the periodic west / east copy over every row; the south halo is left as it is"""
    (Nx, Ny), (Hx, Hy) = size[:2], halo[:2]
    assert P.shape == (Ny + 2 * Hy, Nx + 2 * Hx) and Hx <= Nx
    i = np.arange(1, Nx + 1)
    if xface:
        ip = Nx - i + 2                                    # :73, :90
        ip = np.where(ip > Nx, ip - Nx, ip)                # :75, :92  (|sign| of +1 is +1: :74, :91)
    else:
        ip = Nx - i + 1                                    # :110, :125
    col, colp = i + Hx - 1, ip + Hx - 1
    for j in range(1, Hy + 1):
        src = Ny - j + 1 if yface else Ny - j              # :80, :115 / :97, :130 (the Ny line is duplicated)
        P[Ny + j + Hy - 1, col] = P[src + Hy - 1, colp]
    if not yface:                                          # :102, :135: the redundant part of the last row
        row = P[Ny + Hy - 1].copy()
        m = i > Nx // 2
        P[Ny + Hy - 1, col[m]] = row[colp[m]]
    P[:, :Hx] = P[:, Nx:Nx + Hx].copy()                    # west <- east interior
    P[:, Nx + Hx:] = P[:, Hx:2 * Hx].copy()                # east <- west interior
    return P


# ---- metrics (tripolar_grid_utils.jl:13-43) -------------------------------------------------------------------------------------------------
def edge_tolerance(l1, p1, l2, p2, R):
    """the per-edge Float64 bound of the module docstring, absolute (the unit of R); Float64 inputs"""
    dl_deg = l2 - l1
    dl = dl_deg * D2R
    a1, a2 = p1 * D2R, p2 * D2R
    hl, hp = dl / 2, (a2 - a1) / 2
    dhl = np.spacing(np.abs(dl_deg)) * np.pi / 720 + np.spacing(np.abs(dl)) / 4 + E * np.abs(hl) / 4
    dhp = (np.spacing(np.abs(a1)) + np.spacing(np.abs(a2))) / 4 + np.spacing(np.abs(a2 - a1)) / 4 + E * (np.abs(a1) + np.abs(a2)) / 8
    same = (dl_deg == 0) & (p1 == p2)
    S1, S2, c1, c2 = np.abs(np.sin(hp)), np.abs(np.sin(hl)), np.abs(np.cos(a1)), np.abs(np.cos(a2))
    a = np.minimum(S1 * S1 + c1 * c2 * S2 * S2, 1.0)
    r = np.sqrt(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        w1 = np.where(r > 0, S1 / r, 1.0)
        w2 = np.where(r > 0, c1 * c2 * S2 / r, np.sqrt(c1 * c2))
        q = np.where(r > 0, S2 * S2 / r, 0.0)
    dc1 = E * c1 + np.abs(np.sin(a1)) * (np.spacing(np.abs(a1)) / 2 + E * np.abs(a1) / 4)
    dc2 = E * c2 + np.abs(np.sin(a2)) * (np.spacing(np.abs(a2)) / 2 + E * np.abs(a2) / 4)
    g = 1 / np.sqrt(np.maximum(1 - a, 1e-30))
    tol = R * ((2 * w2 * np.abs(np.cos(hl)) * dhl + 2 * w1 * np.abs(np.cos(hp)) * dhp + q * (c2 * dc1 + c1 * dc2) + 5 * E * r) * g
               + 4 * E * np.arcsin(r))
    return np.where(same, 0.0, tol)


def _haversine(B, P1, P2, R):
    """Distances.haversine((lam1, phi1), (lam2, phi2), R) [recalled] -> (value, tolerance, |dlam| > 180)"""
    (l1, p1), (l2, p2) = P1, P2
    k = B.pi / 360
    hl, hp = (B.lift(l2) - B.lift(l1)) * k, (B.lift(p2) - B.lift(p1)) * k
    S1, S2 = B.sin(hp), B.sin(hl)
    a = S1 * S1 + B.cos(B.lift(p1) * (2 * k)) * B.cos(B.lift(p2) * (2 * k)) * (S2 * S2)
    r = B.sqrt(a)
    r = np.where(np.asarray(r > 1, dtype=bool), 1 + 0 * r, r)                                              # min(sqrt(a), 1)
    return 2 * (_lift_scalar(B, R) * B.arcsin(r)), edge_tolerance(l1, p1, l2, p2, R), np.abs(l2 - l1) > 180


def _cartesian(B, lam, phi):
    """Oceananigans lat_lon_to_cartesian(phi, lambda, 1) [recalled]: degree functions, exact at the multiples of 90"""
    sl, cl, _ = _sincosd(B, lam)
    sp, cp, _ = _sincosd(B, phi)
    return (cl * cp, sl * cp, sp)


def _triangle(B, a, b, c):
    """spherical_area_triangle (Eriksson 1990) [recalled] -> (area, conditioning 2 (|D| + |N|) / (D^2 + N^2))"""
    dot = lambda u, v: u[0] * v[0] + u[1] * v[1] + u[2] * v[2]
    cross = (b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0])
    N, D = abs(dot(a, cross)), 1 + dot(a, b) + dot(b, c) + dot(a, c)
    Dz = np.asarray(D == 0, dtype=bool)
    area = np.where(Dz, B.pi + 0 * N, 2 * B.arctan(N / np.where(Dz, 1 + 0 * D, D)))
    n, d = _f64(B, N), _f64(B, D)
    with np.errstate(divide="ignore"):
        return area, 2 * (np.abs(d) + n) / (d * d + n * n)


def _quadrilateral(B, a, b, c, d):
    """spherical_area_quadrilateral [recalled] -> (solid angle, kappa)"""
    parts = [_triangle(B, a, b, c), _triangle(B, a, b, d), _triangle(B, a, c, d), _triangle(B, b, c, d)]
    return sum(p[0] for p in parts) / 2, sum(p[1] for p in parts) / 2


def metrics(stored, size, halo, radius=R_EARTH, arith=None):
    """`stored`: the 8 (Ny, Nx) Float64 coordinate interiors.  -> (values, tolerances, wraps): the 12 (Ny, Nx) metric interiors of
    tripolar_grid_utils.jl:13-43 before any fill (unrounded), their absolute Float64 tolerances, and per edge array the mask of the
    edges that cross the 0 / 360 wrap"""
    B = backend(arith)
    (Nx, Ny), (Hx, Hy) = size[:2], halo[:2]
    assert Hx >= 1 and Hy >= 1
    C = {}
    for name in COORDS:
        xf, yf = LOCS[name[-2:]]
        C[name] = fill(_pad(np.asarray(stored[name], dtype=np.float64), size, halo), xf, yf, size, halo)
    pt = lambda loc, di, dj: (C["lambda_" + loc][Hy + dj:Hy + dj + Ny, Hx + di:Hx + di + Nx],
                              C["phi_" + loc][Hy + dj:Hy + dj + Ny, Hx + di:Hx + di + Nx])
    edges = {"dx_cc": (pt("fc", 1, 0), pt("fc", 0, 0)), "dx_fc": (pt("cc", 0, 0), pt("cc", -1, 0)),         # :13-14
             "dx_cf": (pt("ff", 1, 0), pt("ff", 0, 0)), "dx_ff": (pt("cf", 0, 0), pt("cf", -1, 0)),         # :15-16
             "dy_cc": (pt("cf", 0, 1), pt("cf", 0, 0)), "dy_fc": (pt("ff", 0, 1), pt("ff", 0, 0)),         # :18-19
             "dy_cf": (pt("cc", 0, 0), pt("cc", 0, -1)), "dy_ff": (pt("fc", 0, 0), pt("fc", 0, -1))}       # :20-21
    val, tol, wrap = {}, {}, {}
    for name, (P1, P2) in edges.items():
        val[name], tol[name], wrap[name] = _haversine(B, P1, P2, radius)
    R2 = _lift_scalar(B, radius) * _lift_scalar(B, radius)
    cart = lambda loc, di, dj: _cartesian(B, *pt(loc, di, dj))
    for name, quad in (("az_cc", (cart("ff", 0, 0), cart("ff", 1, 0), cart("ff", 1, 1), cart("ff", 0, 1))),          # :23-28
                       ("az_ff", (cart("cc", -1, -1), cart("cc", 0, -1), cart("cc", 0, 0), cart("cc", -1, 0)))):    # :38-43
        omega, kappa = _quadrilateral(B, *quad)
        val[name], tol[name] = omega * R2, AREA_CEILING * E * radius * radius * kappa
    for name in ("az_fc", "az_cf"):                                                                          # :34-35
        dy, dx = "dy" + name[2:], "dx" + name[2:]
        val[name] = val[dy] * val[dx]
        y, x = _f64(B, val[dy]), _f64(B, val[dx])
        tol[name] = y * tol[dx] + x * tol[dy] + E * x * y / 2
    return val, tol, wrap


# ---- continue_south! (tripolar_grid.jl:277-300, 336-357); the lat-lon formulas [recalled], parity unpinned ----------------------------------
def south_rows(size, halo, southernmost_latitude=-80, radius=R_EARTH, arith=None):
    """-> (values, tolerances): per metric name the Hy + 1 values of rows j = 1 - Hy .. 1"""
    B = backend(arith)
    (Nx, Ny), Hy = size[:2], halo[1]
    S = Fraction(float(southernmost_latitude))
    js = range(1 - Hy, 2)
    fr = lambda f: B.lift(np.array([float(v) for v in f], dtype=np.float64)) + B.lift(np.array([float(v - Fraction(float(v))) for v in f]))
    arg = lambda f: fr(f) * B.pi / 180
    dphi = (90 - S) / Ny
    pf, pfn = [S + (j - 1) * dphi for j in js], [S + j * dphi for j in js]
    pc, pcm = [S + (j - 1) * dphi + dphi / 2 for j in js], [S + (j - 2) * dphi + dphi / 2 for j in js]
    R = _lift_scalar(B, radius)
    dlam = 2 * B.pi / Nx
    dlam64 = 2 * np.pi / Nx
    dxc, dxf = R * dlam * B.cos(arg(pc)), R * dlam * B.cos(arg(pf))
    dy = R * (fr([dphi] * len(js)) * B.pi / 180)
    azc = R * R * dlam * (B.sin(arg(pfn)) - B.sin(arg(pf)))
    azf = R * R * dlam * (B.sin(arg(pc)) - B.sin(arg(pcm)))
    f64 = lambda f: np.array([float(v) for v in f]) * D2R
    dx_tol = lambda p: radius * dlam64 * E * (3.7 * np.abs(np.cos(f64(p))) + 3 * np.abs(f64(p) * np.sin(f64(p))))
    az_tol = lambda p, q: radius * radius * dlam64 * E * (np.abs(np.sin(f64(p))) + 3 * np.abs(f64(p) * np.cos(f64(p))) + np.abs(np.sin(f64(q)))
                                                          + 3 * np.abs(f64(q) * np.cos(f64(q))) + 3.2 * np.abs(np.sin(f64(p)) - np.sin(f64(q))))
    dy_tol = 1.7 * E * np.abs(_f64(B, dy))
    val = {"dx_ff": dxf, "dx_fc": dxc, "dx_cf": dxf, "dx_cc": dxc,                                           # :287-290
           "dy_ff": dy, "dy_fc": dy, "dy_cf": dy, "dy_cc": dy,                                               # :292-295: Dy_fc, Dy_fc, Dy_cf, Dy_cf -- one Number
           "az_ff": azf, "az_fc": azc, "az_cf": azf, "az_cc": azc}                                           # :297-300
    tol = {"dx_ff": dx_tol(pf), "dx_fc": dx_tol(pc), "dx_cf": dx_tol(pf), "dx_cc": dx_tol(pc),
           "dy_ff": dy_tol, "dy_fc": dy_tol, "dy_cf": dy_tol, "dy_cc": dy_tol,
           "az_ff": az_tol(pc, pcm), "az_fc": az_tol(pfn, pf), "az_cf": az_tol(pc, pcm), "az_cc": az_tol(pfn, pf)}
    return val, tol


# ---- the whole build ------------------------------------------------------------------------------------------------------------------------
class Reference:
    """values: name -> padded parent (unrounded, the backend's numbers); tol: name -> padded absolute tolerance for the grid's element type;
    wrap: edge name -> padded mask of the wrap-crossing edges; south: the rows j <= 1 of the metrics (a mask over padded rows)"""

    def __init__(self, B, size, halo, dtype, values, tol, wrap):
        self.B, self.size, self.halo, self.dtype, self.values, self.tol, self.wrap = B, size, halo, np.dtype(dtype), values, tol, wrap

    def rows(self, jstart, jend):
        """the latitude band jstart .. jend: rows jstart - Hy .. jend + Hy of the global padded arrays (distributed_tripolar_grid.jl:47-49)"""
        sl = slice(jstart - 1, jend + 2 * self.halo[1])
        cut = lambda d: {n: a[sl] for n, a in d.items()}
        return Reference(self.B, self.size, self.halo, self.dtype, cut(self.values), cut(self.tol), cut(self.wrap))

    def errors(self, got):
        """name -> |got - reference| as Float64 (lambda modulo 360), over the whole padded parent"""
        out = {}
        for name, ref in self.values.items():
            g = np.asarray(got[name])
            assert g.shape == ref.shape and g.dtype == self.dtype, (name, g.shape, ref.shape, g.dtype)
            d = abs(self.B.lift(g) - ref)
            if name.startswith("lambda"):
                d360 = abs(d - 360)
                d = np.where(np.asarray(d360 < d, dtype=bool), d360, d)
            out[name] = _f64(self.B, d)
        return out

    def ratios(self, got):
        """name -> |got - reference| / tolerance per cell (0 where both are 0, inf where only the tolerance is)"""
        out = {}
        for name, d in self.errors(got).items():
            t = self.tol[name]
            with np.errstate(divide="ignore", invalid="ignore"):
                out[name] = np.where(d == 0, 0.0, np.where(t > 0, d / t, np.inf))
            assert not np.isnan(out[name]).any(), name
        return out

    def worst(self, got):
        """the worst ratio per array family, for the figures of the module docstring"""
        r = self.ratios(got)
        fam = {"lambda": max(r[n].max() for n in COORDS[:4]), "phi": max(r[n].max() for n in COORDS[4:]),
               "dx": max(r["dx_" + l].max() for l in LOCS), "dy": max(r["dy_" + l].max() for l in LOCS),
               "az_fc_cf": max(r["az_fc"].max(), r["az_cf"].max()), "az_cc_ff": max(r["az_cc"].max(), r["az_ff"].max())}
        return {k: float(v) for k, v in fam.items()}

    def check(self, got, what=""):
        """every cell of every padded parent within its tolerance"""
        bad = []
        for name, r in self.ratios(got).items():
            if (r > 1.0).any():
                j, i = np.unravel_index(np.argmax(r), r.shape)
                bad.append(f"{name}: {int((r > 1).sum())} cells beyond tolerance, worst {r[j, i]:.3g} x at parent [{j}, {i}] "
                           f"(got {np.asarray(got[name])[j, i]!r}, reference {float(self.values[name][j, i])!r}, tol {self.tol[name][j, i]:.3g})")
        assert not bad, f"{what}: " + "; ".join(bad)


def build(size, halo=(4, 4, 4), southernmost_latitude=-80, north_poles_latitude=55, first_pole_longitude=70, radius=R_EARTH,
          dtype=np.float64, stored=None, arith=None):
    """The reference build.  `stored`: for a Float64 grid the product's own 8 coordinate parents (only their interiors are read) -- the
    metrics then answer "what do these stored numbers give"; None, or a Float32 grid: this module's coordinates rounded to Float64
    (module docstring, Float32)."""
    B = backend(arith)
    dtype = np.dtype(dtype)
    (Nx, Ny), (Hx, Hy) = size[:2], halo[:2]
    f32 = dtype == np.float32
    own = f32 or stored is None
    crd = coordinates(size, north_poles_latitude, first_pole_longitude, southernmost_latitude, dtype, arith, substitute_row_Ny=False)
    values, tol, wrap = {}, {}, {}
    for name in COORDS:
        xf, yf = LOCS[name[-2:]]
        values[name] = fill(_pad(crd[name], size, halo), xf, yf, size, halo)
        tol[name] = fill(_pad(np.full((Ny, Nx), COORD_TOL), size, halo), xf, yf, size, halo)
    if own:
        src = {n: _f64(B, values[n][Hy:Hy + Ny, Hx:Hx + Nx]) for n in COORDS}
        src = {n: (np.mod(a, 360) if n.startswith("lambda") else a) for n, a in src.items()}
    else:
        src = {n: np.asarray(stored[n], dtype=np.float64)[Hy:Hy + Ny, Hx:Hx + Nx] for n in COORDS}
    mval, mtol, mwrap = metrics(src, size, halo, radius, arith)
    sval, stol = south_rows(size, halo, southernmost_latitude, radius, arith)
    moved = 2 * np.sqrt(2) * COORD_TOL * D2R * radius if own else 0.0
    for name in METRICS:
        xf, yf = LOCS[name[-2:]]
        t = mtol[name]
        if own:
            if name[:2] in ("dx", "dy"):
                t = t + moved
            elif name in ("az_fc", "az_cf"):
                t = t + moved * (_f64(B, mval["dx" + name[2:]]) + _f64(B, mval["dy" + name[2:]]) + moved)
            else:
                t = t + np.pi * moved * radius
        V = fill(_pad(mval[name], size, halo), xf, yf, size, halo)                                           # tripolar_grid.jl:230-273
        T = fill(_pad(t, size, halo), xf, yf, size, halo)
        V[:Hy + 1, :] = sval[name][:, None]                                                                  # :287-300: rows 1 - Hy .. 1, every padded column
        T[:Hy + 1, :] = stol[name][:, None]
        values[name], tol[name] = V, T
        if name in mwrap:
            W = fill(_pad(mwrap[name], size, halo), xf, yf, size, halo)
            W[:Hy + 1, :] = False
            wrap[name] = W
    if f32:                                                                                                  # map(FT, .): :308-328
        for name in values:
            v32 = np.abs(_f64(B, values[name])).astype(np.float32)
            tol[name] = tol[name] + np.spacing(v32).astype(np.float64) / 2
    return Reference(B, tuple(size), tuple(halo), dtype, values, tol, wrap)


def check_halo_copies(got, size, halo):
    """Halo cells are copies: every halo cell of the product equals, bit for bit, `fill` applied to the product's own interior (coordinates: the
    whole parent, the zero south halo included; metrics: every row j >= 2, and every north halo row that copies a row j >= 2 -- where Ny <= Hy
    the fold reaches rows j <= 1, which the continuation has since overwritten), and every row j <= 1 of a metric holds one value."""
    (Nx, Ny), (Hx, Hy) = size[:2], halo[:2]
    for name in COORDS + METRICS:
        xf, yf = LOCS[name[-2:]]
        g = np.asarray(got[name])
        want = fill(_pad(g[Hy:Hy + Ny, Hx:Hx + Nx], size, halo), xf, yf, size, halo)
        rows = np.ones(g.shape[0], dtype=bool)
        if name in METRICS:
            rows[:Hy + 1] = False
            for j in range(1, Hy + 1):
                rows[Ny + j + Hy - 1] = (Ny - j + 1 if yf else Ny - j) >= 2
            assert (g[:Hy + 1] == g[:Hy + 1, :1]).all(), f"{name}: rows j <= 1 are not constant along x"
        same = (g[rows].view(np.uint8) == want[rows].view(np.uint8)).all()
        assert same, f"{name}: halo cells differ from the fill of the array's own interior"


# ---- the shapes and parameters both suites use (tests/test_oracle_grid.py holds the oracle to this module at them, tests/test_gpu_grid_reference.py
# the kernels).  k_cells_tile emits 62 columns x 7 cell rows per block: Nx and Ny on both sides of one and of two tile edges, Nx = 0 and 2 mod 4;
# k_south runs as a launch of its own when Ny <= 2 Hy + 2 and is merged otherwise: both paths occur at every halo but (1, 1, 1)
GPU_SIZES = [(62, 7), (64, 8), (124, 14), (126, 15), (128, 22), (130, 36)]
HALOS = [(4, 4, 4), (5, 5, 5), (3, 2, 1), (1, 1, 1)]
PARAMS = {"default": {},
          "npl35-fpl75": dict(north_poles_latitude=35, first_pole_longitude=75),
          "npl60-fpl-35.25": dict(north_poles_latitude=60, first_pole_longitude=-35.25),
          "fpl1000.5": dict(first_pole_longitude=1000.5),                       # |fpl + 90| > 360: the general coord() path on every wave
          "south-75.5-R1": dict(southernmost_latitude=-75.5, radius=1.0),       # the twice-precision phi range
          "south-89-npl80.25": dict(southernmost_latitude=-89, north_poles_latitude=80.25)}
PARAM_SIZES = [(126, 15), (128, 22)]
DTYPES = [np.float64, np.float32]
# ((Nx, Ny), halo, jstart, jend): the two halves and the three thirds of (128, 22) as local_size cuts them, and a band thinner than its halo
BANDS = [((128, 22), (4, 4, 4), 1, 11), ((128, 22), (4, 4, 4), 12, 22), ((128, 22), (4, 4, 4), 8, 14), ((128, 22), (5, 5, 5), 15, 22),
         ((128, 22), (5, 5, 5), 9, 11)]


def gpu_cases():
    """(size, halo, parameter id, dtype): the defaults on every shape and halo, the other parameter sets on PARAM_SIZES"""
    out = [(s, h, "default", dt) for s in GPU_SIZES for h in HALOS for dt in DTYPES]
    out += [(s, (4, 4, 4), p, dt) for s in PARAM_SIZES for p in PARAMS if p != "default" for dt in DTYPES]
    return out


def case_id(c):
    (Nx, Ny), h, p, dt = c
    return f"{Nx}x{Ny}-h{h[0]}{h[1]}{h[2]}-{p}-{np.dtype(dt).name}"
