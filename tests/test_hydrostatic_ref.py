"""tests/hydrostatic_ref.py held to properties (no GPU), so that it is not merely a second copy of the kernel: the column sum against closed
forms, the Coriolis term against exact products, a conservation law and the momentum reference's vorticity term, the cells read against the
header's table by perturbation, and the signs of zero of the ADD / WRITE and dropped-term forms."""
import itertools

import numpy as np
import pytest

import hydrostatic_ref as R
import momentum_ref
from hydrostatic_ref import ADD, ENERGY, ENSTROPHY, WRITE, same_bits

F32, F64 = np.float32, np.float64
TYPES = pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])


def _shapes(size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)


def _random(size, halo, dtype, seed=0):
    rng = np.random.default_rng(seed)
    parent, plane = _shapes(size, halo)
    h = {k: rng.uniform(-1, 1, parent).astype(dtype) for k in ("u", "v", "b", "Gu", "Gv")}
    h["f_ff"] = rng.uniform(-1, 1, plane).astype(dtype)
    h.update({k: rng.uniform(0.5, 2, plane).astype(dtype) for k in R.METRICS})
    h["dz_f"] = rng.uniform(0.5, 2, size[2] + 1).astype(dtype)
    return h


def _unit(size, halo, dtype):
    return {k: np.ones(_shapes(size, halo)[1], dtype) for k in R.METRICS}


@TYPES
def test_uniform_b_gives_the_running_sum_and_no_gradient(dtype):
    """b uniform, halos included.  With b a power of two every product b * dz is exact, so PH[k] is exactly minus b times the running sum of
    dz_f formed top-down in the type; for any b it is the same recurrence on b * dz_f.  Every column is the same sequence, so px = py = +0"""
    size, halo = (6, 5, 7), (2, 1, 1)
    h = _random(size, halo, dtype)
    for value in (dtype(0.5), dtype(-4.0), dtype(0.3)):
        b = np.full_like(h["b"], value)
        PH = R.pressure_columns(b, h["dz_f"], size, halo)
        acc, run = None, dtype(0)
        for k in range(size[2], 0, -1):                            # 1-based level k takes dz_f[k + 1], element k
            run = dtype(run + h["dz_f"][k])
            acc = -(value * h["dz_f"][k]) if acc is None else dtype(acc - value * h["dz_f"][k])
            assert (PH[k - 1] == acc).all()
            if value != dtype(0.3):
                assert (PH[k - 1] == -(value * run)).all()
        px, py, _ = R.pressure_gradient(b, h, h["dz_f"], size, halo)
        assert (px == 0).all() and (py == 0).all() and not np.signbit(px).any() and not np.signbit(py).any()


@TYPES
def test_linear_b_on_uniform_spacing_is_the_quadratic(dtype):
    """b = N2 z on uniform dz: the rule is the trapezoid sum from z_k up to the halo centre z = +dz/2, exact for a linear integrand:
    PH[k] = (N2 / 2) (z_k^2 - dz^2 / 4).  The bound: level k is n = Nz - k + 1 steps.  A step forms x = (0.5 (b_k + b_k+1)) dz from values
    rounded once to the type (u each), one addition (u) and one product (u); the halving is exact: |dx| <= 3u |x| to first order.  Then one
    subtraction: u |PH|.  All x below the top have one sign (the top one is exactly 0), so |PH| grows downwards and the errors add to at most
    3u sum|x| + n u |PH[k]| = (n + 3) u |PH[k]|.  With u = eps / 2 and the Float64 closed form's own few roundings, (n + 6) eps / 2; the
    test allows (n + 6) eps, the factor 2 covering the second-order terms."""
    size, halo = (2, 1, 40), (1, 1, 1)
    Nz, dz, N2 = size[2], 12.5, 1e-5
    zc = (np.arange(0, Nz + 2) - Nz - 0.5) * dz                    # centres k = 0 .. Nz + 1
    b = np.broadcast_to((N2 * zc).astype(dtype)[:, None, None], _shapes(size, halo)[0]).copy()
    PH = R.pressure_columns(b, np.full(Nz + 1, dz, dtype), size, halo)
    eps = np.finfo(dtype).eps
    for k in range(1, Nz + 1):
        exact = 0.5 * N2 * (zc[k] ** 2 - dz ** 2 / 4)
        n = Nz - k + 1
        assert np.abs(PH[k - 1].astype(F64) - exact).max() <= (n + 6) * eps * abs(exact), (k, PH[k - 1].flat[0], exact)
    assert PH[Nz - 1].flat[0] == 0 and PH[0].flat[0] > 0             # the top step is exactly zero; b < 0 below: PH > 0


@TYPES
def test_one_level_is_the_single_top_step(dtype):
    size, halo = (4, 3, 1), (1, 1, 2)
    h = _random(size, halo, dtype, 3)
    PH = R.pressure_columns(h["b"], h["dz_f"], size, halo)
    assert PH.shape[0] == 1 and h["dz_f"].shape == (2,)
    assert same_bits(PH[0], -((dtype(0.5) * (h["b"][2] + h["b"][3])) * h["dz_f"][1])) == 0


@TYPES
@pytest.mark.parametrize("scheme", [ENSTROPHY, ENERGY])
def test_unit_metrics_and_uniform_fields_give_f_times_the_velocity(dtype, scheme):
    size, halo = (6, 5, 2), (1, 1, 1)
    parent, plane = _shapes(size, halo)
    f, u, v = dtype(0.3), dtype(-0.7), dtype(1.1)
    cu, cv = R.coriolis(np.full(parent, u), np.full(parent, v), np.full(plane, f), _unit(size, halo, dtype), size, halo, scheme)
    assert (cu == f * v).all() and (cv == f * u).all()


def test_the_energy_conserving_scheme_does_no_work():
    """unit metrics, doubly periodic data, Float64: sum(u cu - v cv) = sum over the (Face, Face) nodes of f VX UY minus itself.  The bound: N
    = Nx Ny Nz terms t = u cu - v cv; cu, cv carry at most 6 roundings, the two products and the difference 3 more: 9u |t|-sized errors per
    term (against |u cu| + |v cv|), and a float64 summation of N terms adds at most N u sum|t|.  Allowed: (N + 9) eps * sum(|u cu| + |v cv|)"""
    size, halo = (8, 6, 3), (1, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _random(size, halo, F64, 5)

    def wrap(a):
        a = a.copy()
        inner = a[..., Hy:Hy + Ny, Hx:Hx + Nx]
        return np.pad(inner, [(0, 0)] * (a.ndim - 2) + [(Hy, Hy), (Hx, Hx)], mode="wrap")
    u, v, f = wrap(h["u"]), wrap(h["v"]), wrap(h["f_ff"])
    cu, cv = R.coriolis(u, v, f, _unit(size, halo, F64), size, halo, ENERGY)
    ui, vi = momentum_ref._win(u, size, halo), momentum_ref._win(v, size, halo)
    work, scale = float(np.sum(ui * cu - vi * cv)), float(np.sum(np.abs(ui * cu) + np.abs(vi * cv)))
    assert abs(work) <= (Nx * Ny * Nz + 9) * np.finfo(F64).eps * scale, (work, scale)
    assert scale > 1 and abs(float(np.sum(ui * cu))) > 1e-3          # the two halves do not vanish on their own
    ens = R.coriolis(u, v, f, _unit(size, halo, F64), size, halo, ENSTROPHY)
    assert abs(float(np.sum(ui * ens[0] - vi * ens[1]))) > 1e-6      # and the other scheme does work


@TYPES
def test_the_enstrophy_scheme_is_the_momentum_vorticity_term_with_f_for_zeta(dtype):
    """momentum_ref's hu = -((zb vh) / dx_fc), hv = (zb uh) / dy_cf with Z = f: cu = -hu and cv = hv, bit for bit.  Z is made to equal f
    exactly through the arrays the Coriolis term does not read.  For the u equation: dy_cf = 0 and az_ff = 1 leave Z = 0 - (dx_fc u[j] -
    dx_fc u[j-1]); with dx_fc powers of two, f small dyadic numbers and u = -(the running sum of f along j) / dx_fc every product and
    difference is exact and Z = f.  For the v equation likewise with dx_fc = 0, dy_cf powers of two and v = (the running sum of f along
    i) / dy_cf.  v and dx_cf (u and dy_fc) stay random: vh (uh) is general"""
    size, halo = (8, 6, 2), (2, 2, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = _shapes(size, halo)
    rng = np.random.default_rng(11)
    h = _random(size, halo, dtype, 11)
    f = (rng.integers(-8, 9, plane) / 16).astype(dtype)
    pow2 = lambda: (2.0 ** rng.integers(-2, 3, plane)).astype(dtype)                                                           # noqa: E731
    w = np.zeros((parent[0] + 1, *plane), dtype)
    ones = np.ones(plane, dtype)
    # the u equation
    dx_fc = pow2()
    u = np.broadcast_to(-(np.cumsum(f.astype(F64), axis=0) / dx_fc).astype(dtype), parent).copy()
    m = dict(dx_fc=dx_fc, dy_fc=h["dy_fc"], az_fc=ones, dx_cf=h["dx_cf"], dy_cf=np.zeros(plane, dtype), az_cf=ones, az_cc=ones, az_ff=ones)
    assert same_bits(momentum_ref.zeta(u, h["v"], m, size, halo)[0], momentum_ref._win(f, size, halo)) == 0
    with np.errstate(all="ignore"):
        t = momentum_ref.terms(u, h["v"], w, m, h["dz_f"], size, halo)
    cu, _ = R.coriolis(u, h["v"], f, m, size, halo, ENSTROPHY)
    assert same_bits(cu, -t["hu"]) == 0 and np.isfinite(cu).all() and (cu != 0).mean() > 0.9
    # the v equation
    dy_cf = pow2()
    v = np.broadcast_to((np.cumsum(f.astype(F64), axis=1) / dy_cf).astype(dtype), parent).copy()
    m = dict(dx_fc=np.zeros(plane, dtype), dy_fc=h["dy_fc"], az_fc=ones, dx_cf=h["dx_cf"], dy_cf=dy_cf, az_cf=ones, az_cc=ones, az_ff=ones)
    assert same_bits(momentum_ref.zeta(h["u"], v, m, size, halo)[0], momentum_ref._win(f, size, halo)) == 0
    with np.errstate(all="ignore"):
        t = momentum_ref.terms(h["u"], v, w, m, h["dz_f"], size, halo)
        _, cv = R.coriolis(h["u"], v, f, m, size, halo, ENSTROPHY)
    assert same_bits(cv, t["hv"]) == 0 and np.isfinite(cv).all() and (cv != 0).mean() > 0.9


# the header's table: (array, di, dj) a node reads; b at every level k .. Nz + 1
HEADER = {"Gu": {"v": {(-1, 0), (-1, 1), (0, 0), (0, 1)}, "dx_cf": {(-1, 0), (-1, 1), (0, 0), (0, 1)}, "f_ff": {(0, 0), (0, 1)},
                 "b": {(0, 0), (-1, 0)}, "dx_fc": {(0, 0)}},
          "Gv": {"u": {(0, -1), (1, -1), (0, 0), (1, 0)}, "dy_fc": {(0, -1), (1, -1), (0, 0), (1, 0)}, "f_ff": {(0, 0), (1, 0)},
                 "b": {(0, 0), (0, -1)}, "dy_cf": {(0, 0)}}}


@pytest.mark.parametrize("scheme", [ENSTROPHY, ENERGY])
def test_perturbing_every_cell_finds_exactly_the_cells_of_the_header(scheme):
    """every cell of every input is perturbed in turn: the nodes of Gu, Gv that change give the offsets read, which are the header's lists --
    b at the levels k .. Nz + 1 only --, and the cells that change anything are exactly cells_read's.  Plane 0 of b, its corner columns and
    the corners u[0, 0], v[Nx+1, Ny+1] change nothing; the corners v[0, Ny+1] and u[Nx+1, 0] do"""
    size, halo = (4, 3, 2), (1, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _random(size, halo, F64, 2)
    run = lambda x: R.interior_tendencies(x["u"], x["v"], x["b"], x["Gu"], x["Gv"], x["f_ff"], x, x["dz_f"], size, halo, scheme, ADD)[:2]   # noqa: E731
    base = run(h)
    found = {"Gu": {}, "Gv": {}}
    touched = {k: np.zeros(h[k].shape, bool) for k in ("u", "v", "b", "f_ff", *R.METRICS)}
    for name in touched:
        for cell in itertools.product(*(range(n) for n in h[name].shape)):
            x = dict(h, **{name: h[name].copy()})
            x[name][cell] += 0.125
            for out, got, ref in zip(("Gu", "Gv"), run(x), base):
                for k, j, i in zip(*np.nonzero(got != ref)):
                    touched[name][cell] = True
                    found[out].setdefault(name, set()).add((cell[-1] - Hx - i, cell[-2] - Hy - j))
                    if len(cell) == 3:
                        dk = cell[0] - Hz - k
                        assert (0 <= dk <= Nz - k) if name == "b" else dk == 0, (name, cell, out, k)
    assert found == HEADER
    read = R.cells_read(size, halo)
    for name in touched:
        assert (touched[name] == read[name]).all(), name
    assert not touched["b"][0].any() and not touched["b"][:, 0, 0].any() and touched["b"][Hz + Nz].any()
    assert touched["v"][Hz, Hy + Ny, 0] and touched["u"][Hz, 0, Hx + Nx] and not touched["u"][Hz, 0, 0] and not touched["v"][Hz, Hy + Ny, Hx + Nx]
    for which in ("Gu", "Gv"):                                     # and per field
        one = R.cells_read(size, halo, which=which)
        for name in touched:
            assert one[name].any() == (name in HEADER[which]), (which, name)
    assert R.cells_read(size, halo, which="p")["b"].sum() == Nx * Ny * (Nz + 1)


@TYPES
@pytest.mark.parametrize("scheme", [ENSTROPHY, ENERGY])
def test_add_onto_minus_zero_is_write_and_plus_zero_is_not(dtype, scheme):
    """-0 is the additive identity of IEEE arithmetic, +0 is not: (+0) + (-0) = +0.  ADD onto -0 equals WRITE bit for bit in every form; ADD
    onto +0 differs from WRITE exactly in sign where cu = -0 (Coriolis alone, v = 0 under a negative f)"""
    size, halo = (6, 5, 3), (1, 1, 1)
    h = _random(size, halo, dtype, 4)
    mz = np.full_like(h["u"], -0.0)
    for f, b in ((h["f_ff"], h["b"]), (h["f_ff"], None), (None, h["b"])):
        add = R.interior_tendencies(h["u"], h["v"], b, mz, mz, f, h, h["dz_f"], size, halo, scheme, ADD)
        write = R.interior_tendencies(h["u"], h["v"], b, None, None, f, h, h["dz_f"], size, halo, scheme, WRITE)
        assert same_bits(add[0], write[0]) == 0 and same_bits(add[1], write[1]) == 0
    v0, f = np.zeros_like(h["v"]), -np.abs(h["f_ff"])
    write = R.interior_tendencies(h["u"], v0, None, None, None, f, h, h["dz_f"], size, halo, scheme, WRITE)
    assert (write[0] == 0).all() and np.signbit(write[0]).all()      # cu = -0
    pz = np.zeros_like(h["u"])
    add = R.interior_tendencies(h["u"], v0, None, pz, pz, f, h, h["dz_f"], size, halo, scheme, ADD)
    assert (add[0] == 0).all() and not np.signbit(add[0]).any()       # (+0) + (-0) = +0: not WRITE's bits
    add = R.interior_tendencies(h["u"], v0, None, mz, mz, f, h, h["dz_f"], size, halo, scheme, ADD)
    assert same_bits(add[0], write[0]) == 0


@TYPES
@pytest.mark.parametrize("scheme", [ENSTROPHY, ENERGY])
def test_a_dropped_term_is_the_full_form_with_a_zero_input_but_for_signs_of_zero(dtype, scheme):
    """b = +0 (or -0) gives px = py = +0 exactly (PH = -0, -0 - (+0) = -0, (-0) - (-0) = +0), and x - (+0) = x for every x: the form without b
    equals the full form with b = +-0 ALWAYS, in both modes.
    f = +0 gives cu, cv = +-0 (finite velocities).  ADD: (Gu + (+-0)) - px against Gu - px differ only where Gu = -0 and cu = +0 (the sum is
    +0) and then only if px = +0 ((+0) - (+0) = +0 against (-0) - (+0) = -0); likewise Gv = +0 with cv = +0 ... so never on data without
    zeros.  WRITE: (+-0) - px against -px differ exactly where px = +0 with cu = +0 (+0 against -0) or px = -0 with cu = -0 ((-0) - (-0) = +0
    = -(-0): equal) -- that is only (cu, px) = (+0, +0); for Gv, (-cv) - py against -py: only (cv, py) = (-0, +0)"""
    size, halo = (6, 5, 3), (1, 1, 1)
    h = _random(size, halo, dtype, 6)
    args = lambda b, f, G, mode: (h["u"], h["v"], b, G, G, f, h, h["dz_f"], size, halo, scheme, mode)                          # noqa: E731
    for zero in (0.0, -0.0):
        for mode, G in ((ADD, h["Gu"]), (WRITE, None), (ADD, np.full_like(h["u"], -0.0)), (ADD, np.zeros_like(h["u"]))):
            full = R.interior_tendencies(*args(np.full_like(h["b"], zero), h["f_ff"], G, mode))
            drop = R.interior_tendencies(*args(None, h["f_ff"], G, mode))
            assert same_bits(full[0], drop[0]) == 0 and same_bits(full[1], drop[1]) == 0
    f0 = np.zeros_like(h["f_ff"])
    for mode, G in ((ADD, h["Gu"]), (WRITE, None)):                # no zeros in Gu, px, py: identical
        full, drop = R.interior_tendencies(*args(h["b"], f0, G, mode)), R.interior_tendencies(*args(h["b"], None, G, mode))
        assert same_bits(full[0], drop[0]) == 0 and same_bits(full[1], drop[1]) == 0
    # the enumerated exceptions, on uniform b (px = py = +0) with u, v > 0 (cu = cv = +0)
    b1, pos = np.ones_like(h["b"]), np.abs(h["u"]) + dtype(0.5)
    a = lambda f, G, mode: R.interior_tendencies(pos, pos, b1, G, G, f, h, h["dz_f"], size, halo, scheme, mode)                # noqa: E731
    full, drop = a(f0, None, WRITE), a(None, None, WRITE)
    assert (full[0] == 0).all() and (drop[0] == 0).all() and not np.signbit(full[0]).any() and np.signbit(drop[0]).all()       # (+0, +0)
    assert np.signbit(full[1]).all() and np.signbit(drop[1]).all()                                                           # (cv, py) = (+0, +0): equal
    mz = np.full_like(h["u"], -0.0)
    full, drop = a(f0, mz, ADD), a(None, mz, ADD)
    assert not np.signbit(full[0]).any() and np.signbit(drop[0]).all()                                                       # Gu = -0, cu = +0, px = +0
    assert np.signbit(full[1]).all() and np.signbit(drop[1]).all()                                                           # (-0) - (+0) - (+0) = -0 both


def test_the_parents_keep_their_halo_cells_and_the_mask_replaces_in_both_modes():
    size, halo = (6, 5, 3), (2, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _random(size, halo, F32, 8)
    n = np.random.default_rng(1).integers(-1, Nz + 2, (2, Ny, Nx)).astype(np.int32)
    sent = np.full_like(h["u"], 12345.0)
    for mode in (ADD, WRITE):
        Gu, Gv, p = R.tendencies(h["u"], h["v"], h["b"], sent, sent, sent, h["f_ff"], h, h["dz_f"], size, halo, ENERGY, mode, n[0], n[1], 0.1)
        inner = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
        edge = np.ones(sent.shape, bool)
        edge[inner] = False
        k = np.arange(1, Nz + 1)[:, None, None]
        for G, q in ((Gu, 0), (Gv, 1)):
            assert (G[edge] == 12345.0).all() and ((G[inner] == F32(0.1)) == (k <= np.clip(n[q], 0, Nz)[None])).all()
        assert (p[edge] == 12345.0).all() and same_bits(p[inner], R.pressure_gradient(h["b"], h, h["dz_f"], size, halo)[2]) == 0
    alone = R.tendencies(None, None, h["b"], None, None, sent, None, h, h["dz_f"], size, halo)
    assert alone[0] is None and alone[1] is None and same_bits(alone[2], p) == 0
