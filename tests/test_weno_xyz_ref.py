"""The numpy reference of the tracer tendency of `WENO()` (tests/weno_xyz_ref.py) checked on its own, without a GPU, against properties and
not against itself: R3 reproduces constants and linear profiles, has the linear weights -1/6, 5/6, 1/3 on smooth data, converges at third
order, does not overshoot a step and mirrors; the order table equals one written by hand; at Nz = 1 the tendency is weno_ref's bit for bit;
the cells read are found by perturbation; the column sum of the vertical part of V G telescopes."""
import numpy as np
import pytest

import weno_ref
import weno_xyz_ref
from weno_xyz_ref import face_order, face_value3, same_bits

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_face_value3_reproduces_constants_exactly_and_linear_profiles_to_rounding(dtype):
    """On a constant q: b0 = b1 = 0, tau = 0, a0 = K(2,3), a1 = K(1,3), p0 = q exactly, p1 = fl(1.5 q) - 0.5 q.  Where q is zero or a power
    of two every product is an exact scaling, so the numerator is q * fl(a0 + a1), the denominator fl(a0 + a1), and the quotient is q
    EXACTLY: that is what "reproduces a constant exactly" can mean in rounded arithmetic with rounded weights, and it is asserted bit for
    bit.  For any other q the five roundings on the way (1.5 q, p1, the two products, their sum; the quotient is the sixth) each move the
    value by at most half an ulp of q: asserted within 3 ulp of q, measured below."""
    for value in (0.0, 1.0, -4.0, 2.0 ** -40, 2.0 ** 60, -0.5):
        q = np.array([value], dtype)
        assert same_bits(face_value3(q, q, q), q) == 0, value
    worst = 0.0
    for value in (-3.25, 0.1, 1e-30, 7e8, 1 / 3, 0.7, -123.456):
        q = np.array([value], dtype)
        miss = abs(float(face_value3(q, q, q)[0]) - float(q[0])) / float(np.spacing(np.abs(q))[0])
        worst = max(worst, miss)
        assert miss <= 3, (value, miss)
    print("constants off the powers of two: worst miss", worst, "ulp")
    # linear in the index: the face between q1 and q2 lies half a cell past q1.  b0 = b1 exactly for small integers, so the weights are
    # the linear ones and the value is a + 1.5 b to a few ulp of the largest input
    for a, b in ((0, 1), (5, -2), (-7, 3), (4, 0)):
        q = [np.array([a + b * n], dtype) for n in range(3)]
        got = float(face_value3(*q)[0])
        assert abs(got - (a + 1.5 * b)) <= 4 * np.finfo(dtype).eps * max(abs(a) + 2 * abs(b), 1), (a, b, got)


def test_linear_weights_on_smooth_data():
    """where tau / (b + eps) vanishes the weights are 2/3 and 1/3 and R3 is linear in its inputs, with the coefficients -1/6, 5/6, 1/3:
    first from the rule's text by hand, then on the reference with data smooth against eps"""
    # on q = (a, a + b, a + 2 b): R3 = a + 1.5 b.  With weights (w0, w1, w2): w0 a + w1 (a + b) + w2 (a + 2 b), so w0 + w1 + w2 = 1 and
    # w1 + 2 w2 = 1.5.  The third equation comes from the two candidate values, which the rule states: p0 = (q1 + q2) / 2 with weight 2/3,
    # p1 = 1.5 q1 - 0.5 q0 with weight 1/3
    w0, w1, w2 = -0.5 / 3, 0.5 * 2 / 3 + 1.5 / 3, 0.5 * 2 / 3
    assert np.allclose([w0, w1, w2], [-1 / 6, 5 / 6, 1 / 3], rtol=0, atol=1e-15)
    assert abs(w0 + w1 + w2 - 1) < 1e-15 and abs(w1 + 2 * w2 - 1.5) < 1e-15
    # and the reference has them.  Three cells within 2e-7 of one another around a base of size <= 1: b <= 1.6e-13, tau <= b, so
    # r = tau / (b + eps) <= 1.6e-5 and r * r <= 2.6e-10 -- the weights are the linear ones to 2.6e-10 relative, which moves the value by at
    # most 2.6e-10 * |p0 - p1| <= 2.6e-10 * 4e-7 ~ 1e-16; the roundings of the rule and of `want` add a few eps of |q| <= 1, say 16 eps.
    # Other weights would miss by a share of the 2e-7 spread: nine orders above the bound.
    rng = np.random.default_rng(0)
    base = rng.uniform(-1, 1, 200)
    q = [base + 1e-7 * rng.uniform(-1, 1, 200) for _ in range(3)]
    got = face_value3(*q)
    want = -q[0] / 6 + 5 * q[1] / 6 + q[2] / 3
    miss = np.abs(got - want).max()
    print("linear weights: worst miss", miss)
    assert miss <= 1e-16 + 16 * np.finfo(F64).eps
    assert np.abs(got - (q[1] + q[2]) / 2).max() > 1e-9            # and it is not the centred mean


def _errors(N):
    """(max error over all faces, max error over the faces where |cos| >= 0.5) of the left-biased R3 on exact cell averages of sin"""
    h = 2 * np.pi / N
    x = (np.arange(N) + 0.5) * h
    averages = np.sin(x) * (np.sin(h / 2) / (h / 2))               # the exact cell averages of sin
    left = face_value3(np.roll(averages, 1), averages, np.roll(averages, -1))
    miss = np.abs(left - np.sin(x + h / 2))
    return miss.max(), miss[np.abs(np.cos(x + h / 2)) >= 0.5].max()


def test_third_order_convergence_on_smooth_data():
    """exact cell averages of sin, Float64, against the point value at the face.  Third order is what a WENO scheme of order 3 has where
    the first derivative does not vanish: beside a critical point (h f' ~ h^2 f'') the two smoothness indicators differ by a factor of
    order one whatever the resolution, the weights leave the linear ones by order one and the error there is second order -- the known
    behaviour of the scheme, not of this statement of it.  So the max error is taken over the faces where |cos| >= 0.5: its ratio under
    doubling, N = 128 -> 256 -> 512, is >= 7.5 (the asymptote of third order is 8; second order would give 4).  The ratio over ALL faces
    is printed, and is 4."""
    e = [_errors(N) for N in (128, 256, 512)]
    print("max errors (all faces, away from critical points)", e)
    print("ratios", [(a[0] / b[0], a[1] / b[1]) for a, b in zip(e, e[1:])])
    assert e[0][1] / e[1][1] >= 7.5 and e[1][1] / e[2][1] >= 7.5
    assert e[2][1] < 2e-7                                          # measured h^3 / 12 cos: (2 pi / 512)^3 / 12 = 1.5e-7


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_no_overshoot_on_a_step_and_mirror_symmetry(dtype):
    c = np.concatenate([np.ones(20, dtype), np.zeros(20, dtype)])
    f = np.arange(2, 38)                                           # face f lies between the cells f - 1 and f
    left = face_value3(c[f - 2], c[f - 1], c[f])
    right = face_value3(c[f + 1], c[f], c[f - 1])
    tol = 1e-15 if dtype == F64 else 1e-6                          # a few ulp of 1
    for r in (left, right):
        print("step", dtype.__name__, r.min(), r.max())
        assert r.min() >= -tol and r.max() <= 1 + tol
    # the right-biased value at face f of c is the left-biased value at face n - f of the reversed array
    rng = np.random.default_rng(5)
    n = 40
    a = rng.uniform(-1, 1, n).astype(dtype)
    b = a[::-1].copy()
    g = n - f
    assert same_bits(face_value3(a[f + 1], a[f], a[f - 1]), face_value3(b[g - 2], b[g - 1], b[g])) == 0
    assert same_bits(face_value3(a[f + 1], a[f], a[f - 1]), face_value3(a[f - 2], a[f - 1], a[f])) > 0


def test_face_order_equals_a_hand_written_table():
    C = weno_xyz_ref.CENTRED
    table = {1: [C, C],
             2: [C, 1, C],
             3: [C, 1, 1, C],
             4: [C, 1, 3, 1, C],
             5: [C, 1, 3, 3, 1, C],
             6: [C, 1, 3, 5, 3, 1, C],
             7: [C, 1, 3, 5, 5, 3, 1, C],
             8: [C, 1, 3, 5, 5, 5, 3, 1, C]}
    for Nz, want in table.items():
        assert [face_order(f, Nz) for f in range(1, Nz + 2)] == want, Nz


def _random_case(size, halo, dtype, seed=1):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent, plane = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)
    rng = np.random.default_rng(seed)
    h = {k: rng.uniform(-1, 1, parent).astype(dtype) for k in ("c", "u", "v")}
    h["w"] = rng.uniform(-1, 1, (parent[0] + 1,) + plane).astype(dtype)
    for k in ("dy_fc", "dx_cf", "az_cc"):
        h[k] = rng.uniform(0.5, 2, plane).astype(dtype)
    h["dz_c"] = rng.uniform(0.5, 2, Nz).astype(dtype)
    return h


def _G(h, size, halo, module=weno_xyz_ref, **kw):
    a = dict(h)
    a.update(kw)
    return module.interior_tendency(a["c"], a["u"], a["v"], a["w"], a["dy_fc"], a["dx_cf"], a["az_cc"], a["dz_c"], size, halo)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_one_level_is_the_existing_rule_bit_for_bit(dtype):
    size, halo = (12, 10, 1), (3, 4, 2)
    h = _random_case(size, halo, dtype)
    assert same_bits(_G(h, size, halo), _G(h, size, halo, module=weno_ref)) == 0
    size = (12, 10, 2)                                             # and with two levels it is not: face 2 takes the upwind cell
    h = _random_case(size, halo, dtype)
    assert same_bits(_G(h, size, halo), _G(h, size, halo, module=weno_ref)) > 0


@pytest.mark.parametrize("Nz", [1, 2, 4, 7])
def test_cells_read_are_found_by_perturbing_every_cell(Nz):
    """each cell of the parent of c in turn gets +1, under w > 0 and under w < 0 (u, v of both signs as drawn, and negated): the cells whose
    change moves some G are exactly cells_read's, and at Hz = 4 no z-halo plane but 0 and Nz + 1 is among them"""
    size, halo, dtype = (6, 4, Nz), (3, 3, 4), F64
    (Nx, Ny, _), (Hx, Hy, Hz) = size, halo
    h = _random_case(size, halo, dtype, seed=Nz)
    flows = [dict(u=s * h["u"], v=s * h["v"], w=t * np.abs(h["w"])) for s in (1, -1) for t in (1, -1)]
    base = [_G(h, size, halo, **f) for f in flows]
    found = np.zeros(h["c"].shape, bool)
    for idx in np.ndindex(*h["c"].shape):
        c = h["c"].copy()
        c[idx] += 1
        found[idx] = any(same_bits(_G(h, size, halo, c=c, **f), b) > 0 for f, b in zip(flows, base))
    read = weno_xyz_ref.cells_read(size, halo)["c"]
    assert np.array_equal(found, read)
    planes = np.flatnonzero(found.any(axis=(1, 2)))
    assert planes.tolist() == list(range(Hz - 1, Hz + Nz + 1))     # the planes 0 .. Nz + 1 and no other halo plane
    assert not found[:Hz - 1].any() and not found[Hz + Nz + 1:].any()


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_vertical_part_telescopes_over_the_column(dtype):
    """with u = v = 0 the horizontal fluxes are zeros, V G = -(Fz[k+1] - Fz[k]) up to the roundings of 1 / V, of its product and of V G, and
    the column sum is -(Fz[Nz+1] - Fz[1]).  Tolerance: each of the Nz terms V[k] * G[k] carries at most 3 relative roundings on top of the
    exact difference (1 / V, the product with it, the product with V) plus half an ulp for the difference itself, and the sum of Nz terms
    of magnitude <= D = max |Fz[k+1] - Fz[k]| adds at most (Nz - 1) roundings of partial sums <= Nz D: so
    |sum + (Fz[Nz+1] - Fz[1])| <= (4 Nz + Nz (Nz - 1)) eps D, evaluated with the sums in the field type itself."""
    size, halo = (8, 6, 9), (3, 3, 2)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _random_case(size, halo, dtype)
    h["u"], h["v"] = np.zeros_like(h["u"]), np.zeros_like(h["v"])
    _, _, Fz, V = weno_xyz_ref.fluxes(h["c"], h["u"], h["v"], h["w"], h["dy_fc"], h["dx_cf"], h["az_cc"], h["dz_c"], size, halo)
    G = _G(h, size, halo)
    total = np.zeros((Ny, Nx), dtype)
    for k in range(Nz):
        total = total + V[k] * G[k]
    D = np.abs(Fz[1:] - Fz[:-1]).max(axis=0)
    bound = (4 * Nz + Nz * (Nz - 1)) * np.finfo(dtype).eps * D
    miss = np.abs(total.astype(F64) + (Fz[Nz].astype(F64) - Fz[0].astype(F64)))
    print("telescoping", dtype.__name__, "worst miss / bound", (miss / bound).max())
    assert (miss <= bound).all()
    assert (np.abs(total) > 100 * bound).any()                     # the sum is not small by itself


@pytest.mark.parametrize("positive", [True, False], ids=["w+", "w-"])
def test_domain_of_dependence_in_z(positive):
    """w of one sign, u = v = 0: a bump at one level moves G exactly at the levels dependence_window lists, for a level of each order class"""
    size, halo, dtype = (6, 4, 9), (3, 3, 1), F64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _random_case(size, halo, dtype)
    h["u"], h["v"] = np.zeros_like(h["u"]), np.zeros_like(h["v"])
    h["w"] = (np.abs(h["w"]) + 0.1) * (1 if positive else -1)
    base = _G(h, size, halo)
    for level in range(1, Nz + 1):
        c = h["c"].copy()
        c[Hz + level - 1, Hy + 2, Hx + 3] += 1
        moved = base != _G(h, size, halo, c=c)
        assert not moved[:, :2].any() and not moved[:, 3:].any() and not moved[:, 2, :3].any() and not moved[:, 2, 4:].any()
        assert np.array_equal(moved[:, 2, 3], weno_xyz_ref.dependence_window(level, size, positive)), level
    # by hand at Nz = 9 (orders of the faces 1 .. 10: C 1 3 5 5 5 5 3 1 C), level 5.  w > 0: a face of order 5 reads f-3 .. f+1, so the faces
    # 4 .. 8 would read level 5; 4 .. 7 have order 5, face 8 has order 3 and reads 6, 7, 8 -> faces 4 .. 7 -> nodes 3 .. 7.  w < 0: f-2 .. f+2,
    # the faces 3 .. 7; face 3 has order 3 and reads 4, 3, 2 -> faces 4 .. 7 -> nodes 3 .. 7.  Level 2: w > 0 the faces 3 (order 3: 1, 2, 3), 4 (1 .. 5)
    # and 5 (2 .. 6), not 2 (order 1: its upwind cell 1) -> nodes 2 .. 5; w < 0: the faces 2 (order 1: cell 2), 3 (order 3: 4, 3, 2) and
    # 4 (2 .. 6) -> nodes 1 .. 4
    win = lambda level: (np.flatnonzero(weno_xyz_ref.dependence_window(level, size, positive)) + 1).tolist()   # noqa: E731
    assert win(5) == [3, 4, 5, 6, 7]
    assert win(2) == ([2, 3, 4, 5] if positive else [1, 2, 3, 4])
