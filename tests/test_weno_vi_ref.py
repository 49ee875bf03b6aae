"""The numpy statement of the rule of include/tripolar_hip_weno_vi.h (tests/weno_vi_ref.py), held to properties without the kernel: what the
new helpers are (W5F against R, its linear weights, C4 on cubics), what the rule gives on flows whose answer is known (a uniform flow, mirror
images in x and y, the telescoping z-fluxes, a smooth non-divergent flow under refinement, a step in z), and the cells it reads, found by
perturbing every cell and compared with the list the header gives."""
import os

import numpy as np
import pytest

import momentum_ref
import weno_vi_ref as ref
from weno_ref import face_value
from weno_vi_ref import METRICS, same_bits

F32, F64 = np.float32, np.float64
X_FACES = ("u", "dx_fc", "dy_fc", "az_fc", "az_ff")               # what sits on an x-face, and shifts by one under a mirror in x
Y_FACES = ("v", "dx_cf", "dy_cf", "az_cf", "az_ff")


def _shapes(size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    return (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Nz + 1 + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx), (Ny + 2 * Hy, Nx + 2 * Hx)


def _random(size, halo, dtype, seed=0, unit=False):
    parent, wparent, plane = _shapes(size, halo)
    rng = np.random.default_rng([seed, *size, *halo])
    h = {"u": rng.uniform(-1, 1, parent).astype(dtype), "v": rng.uniform(-1, 1, parent).astype(dtype),
         "w": rng.uniform(-1, 1, wparent).astype(dtype), "dz_c": rng.uniform(0.5, 2, size[2]).astype(dtype)}
    h.update({k: rng.uniform(0.5, 2, plane).astype(dtype) for k in METRICS})
    if unit:
        h["dz_c"][:] = 1
        for k in METRICS:
            h[k][:] = 1
    return h


def _terms(h, size, halo):
    return ref.terms(h["u"], h["v"], h["w"], {k: h[k] for k in METRICS}, h["dz_c"], size, halo)


# ---- the helpers ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_w5f_of_a_function_on_itself_is_r(dtype):
    rng = np.random.default_rng(1)
    q = [rng.uniform(-2, 2, 4096).astype(dtype) for _ in range(5)]
    q[0][:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-30, 3.0e38 if dtype == F32 else 1e308, 1.0]
    assert same_bits(ref.face_value_fs(q, q), face_value(*q)) == 0
    other = [rng.uniform(-2, 2, 4096).astype(dtype) for _ in range(5)]
    assert same_bits(ref.face_value_fs(q, other), face_value(*q)) > 4000       # the smoothness function matters


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_w5f_with_constant_smoothness_has_the_linear_weights(dtype):
    """s constant: b0 = b1 = b2 = 0, tau = 0, the weights are 3/10, 6/10, 1/10 exactly as computed (their sum rounds to 1), and the value
    is the fifth-order upwind interpolant (2 q0 - 13 q1 + 47 q2 + 27 q3 - 3 q4) / 60 to a few roundings of the candidates"""
    rng = np.random.default_rng(2)
    q = [rng.uniform(-2, 2, 1000).astype(dtype) for _ in range(5)]
    s = [np.full(1000, 1.75, dtype)] * 5
    T = dtype
    K = lambda n, d: T(n) / T(d)                                   # noqa: E731
    p2 = (K(1, 3) * q[0] - K(7, 6) * q[1]) + K(11, 6) * q[2]
    p1 = (K(5, 6) * q[2] - K(1, 6) * q[1]) + K(1, 3) * q[3]
    p0 = (K(1, 3) * q[2] + K(5, 6) * q[3]) - K(1, 6) * q[4]
    a0, a1, a2 = K(3, 10) * T(1), K(3, 5) * T(1), K(1, 10) * T(1)
    want = ((a0 * p0 + a1 * p1) + a2 * p2) / ((a0 + a1) + a2)
    got = ref.face_value_fs(q, s)
    assert same_bits(got, want) == 0
    q64 = [x.astype(F64) for x in q]
    linear = (2 * q64[0] - 13 * q64[1] + 47 * q64[2] + 27 * q64[3] - 3 * q64[4]) / 60
    assert np.abs(got - linear).max() <= 32 * np.finfo(dtype).eps           # |q| <= 2, coefficients sum below 4: a handful of roundings


def test_c4_is_exact_on_cubics():
    """the cell averages of a cubic over four unit cells give its value on the face between the middle two"""
    rng = np.random.default_rng(3)
    c = rng.integers(-8, 9, (4, 500)).astype(F64)                  # p(x) = c0 + c1 x + c2 x^2 + c3 x^3
    anti = lambda x: c[0] * x + c[1] * x ** 2 / 2 + c[2] * x ** 3 / 3 + c[3] * x ** 4 / 4     # noqa: E731
    avg = [anti(x + 1.0) - anti(x) for x in (-2.0, -1.0, 0.0, 1.0)]
    assert np.abs(ref.c4(*avg) - c[0]).max() <= 1e-12
    quartic = [np.array([(b ** 5 - a ** 5) / 5]) for a, b in ((-2, -1), (-1, 0), (0, 1), (1, 2))]
    assert abs(ref.c4(*quartic)[0]) > 1e-3                         # not exact on x^4: order four, no more


# ---- flows whose answer is known -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("speed", [0.75, -0.75])
def test_a_uniform_u_gives_zero_tendencies(dtype, speed):
    size, halo = (6, 5, 7), (3, 3, 1)
    h = _random(size, halo, dtype, unit=True)
    h["u"][:], h["v"][:], h["w"][:] = speed, 0, 0
    t = _terms(h, size, halo)
    assert (t["Gu"] == 0).all() and (t["Gv"] == 0).all()           # +0 or -0 on every node


def _mirror(h, axis):
    """the mirror image of the arrays in x (axis -1) or y (axis -2): a centre cell p of a parent goes to n - 1 - p, a face to n - p (the
    face p = 0 has no image; with a halo of 4 nothing reads it), the velocity normal to the mirror changes its sign"""
    faces, normal = (X_FACES, "u") if axis == -1 else (Y_FACES, "v")
    out = {}
    for k, a in h.items():
        if k == "dz_c":
            out[k] = a
            continue
        b = np.flip(a, axis)
        if k in faces:
            b = np.roll(b, 1, axis)
        out[k] = -b if k == normal else b
    return out


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("axis", [-1, -2], ids=["x", "y"])
def test_mirror_symmetry(dtype, axis):
    """the rule applied to the mirror image of a flow is the mirror image of the rule's result, bit for bit: every sum of the rule that the
    mirror reorders is a sum of two, and every upwind window goes over into the other one"""
    size, halo = (8, 7, 7), (4, 4, 4)
    (Nx, Ny, Nz) = size
    h = _random(size, halo, dtype, seed=4)
    t, tm = _terms(h, size, halo), _terms(_mirror(h, axis), size, halo)
    if axis == -1:      # Gu'[i] = -Gu[Nx + 2 - i] for i = 2..Nx; Gv'[i] = Gv[Nx + 1 - i]
        assert same_bits(tm["Gu"][:, :, 1:], -t["Gu"][:, :, :0:-1]) == 0
        assert same_bits(tm["Gv"], t["Gv"][:, :, ::-1]) == 0
    else:
        assert same_bits(tm["Gv"][:, 1:, :], -t["Gv"][:, :0:-1, :]) == 0
        assert same_bits(tm["Gu"], t["Gu"][:, ::-1, :]) == 0


def test_the_z_fluxes_telescope_to_the_wall_faces():
    size, halo = (6, 5, 9), (3, 3, 2)
    t = _terms(_random(size, halo, F64, seed=5), size, halo)
    for F in (t["FZu"], t["FZv"]):
        total = (F[1:] - F[:-1]).sum(axis=0)
        assert np.abs(total - (F[-1] - F[0])).max() <= 1e-13 * np.abs(F).max() * size[2]
        assert np.abs(F[-1] - F[0]).max() > 0.01


def _smooth(N, dtype=F64):
    """a smooth, discretely non-divergent flow on the unit square with N x N cells of width h = 1/N and one level: u = -dpsi/dy, v = dpsi/dx
    of a streamfunction on the (Face, Face) nodes, w = 0; every halo cell holds the analytic value"""
    size, halo = (N, N, 1), (3, 3, 1)
    parent, wparent, plane = _shapes(size, halo)
    hh = 1.0 / N
    xf = (np.arange(plane[1] + 1) - 3) * hh                        # x of the faces i = -2 ..
    yf = (np.arange(plane[0] + 1) - 3) * hh
    psi = (np.sin(2 * np.pi * xf)[None, :] * np.cos(2 * np.pi * yf)[:, None] + 0.3 * np.cos(4 * np.pi * xf)[None, :] * np.sin(2 * np.pi * yf)[:, None]) / (2 * np.pi)
    u2 = -(psi[1:, :-1] - psi[:-1, :-1]) / hh
    v2 = (psi[:-1, 1:] - psi[:-1, :-1]) / hh
    h = {"u": np.broadcast_to(u2, parent).astype(dtype), "v": np.broadcast_to(v2, parent).astype(dtype), "w": np.zeros(wparent, dtype),
         "dz_c": np.ones(1, dtype)}
    for k in METRICS:
        h[k] = np.full(plane, hh * hh if k.startswith("az") else hh, dtype)
    return h, size, halo


def test_convergence_towards_the_centred_rule_on_a_smooth_flow():
    """Both rules are consistent discretisations of -(U . grad) u; the centred one (tests/momentum_ref.py) is of second order, so the
    difference of the two shrinks at second order or better under refinement.  With a difference a h^2 + b h^3 + .. the observed order
    between h and h/2 is 2 + O(h): it approaches 2 from either side and its distance from 2 halves with h.  So the test asks that every
    halving of h shrinks the difference at least 3.5 times, and that the order between the two finest grids is 2 to within 0.01.
    Observed with N = 16, 32, 64, 128, 256 (maximum norm, relative): orders Gu 1.892, 1.972, 2.006, 1.997 and Gv 2.174, 2.036, 2.007,
    2.002."""
    diffs = []
    for N in (16, 32, 64, 128, 256):
        h, size, halo = _smooth(N)
        m = {k: h[k] for k in METRICS}
        new = ref.terms(h["u"], h["v"], h["w"], m, h["dz_c"], size, halo)
        old = momentum_ref.terms(h["u"], h["v"], h["w"], m, np.ones(2), size, halo)
        div = (h["u"][:, :-1, 1:] - h["u"][:, :-1, :-1]) + (h["v"][:, 1:, :-1] - h["v"][:, :-1, :-1])
        assert np.abs(div).max() < 1e-12 * N                       # discretely non-divergent: DS is rounding
        diffs.append([np.abs(new[G] - old[G]).max() / np.abs(old[G]).max() for G in ("Gu", "Gv")])
    orders = np.log2(np.array(diffs[:-1]) / np.array(diffs[1:]))
    print("relative differences", diffs, "orders", orders.tolist())
    assert (np.array(diffs[:-1]) >= 3.5 * np.array(diffs[1:])).all(), orders
    assert (orders[-1] >= 1.99).all(), orders


@pytest.mark.parametrize("sign", [1.0, -1.0, -0.0])
def test_zf_does_not_overshoot_on_a_step(sign):
    size, halo = (4, 3, 9), (3, 3, 1)
    parent, wparent, plane = _shapes(size, halo)
    for at in range(0, 12):
        x = np.zeros(parent)
        x[at:] = 1.0
        M = np.full((size[2] + 1, size[1], size[0]), sign)
        C = ref.z_face_values(x, M, size, halo)
        assert C.min() >= -1e-12 and C.max() <= 1 + 1e-12, (at, C[:, 0, 0])


# ---- the cells read ---------------------------------------------------------------------------------------------------------------------------
def _reached(h, size, halo, name, base):
    """the cells of the parent `name` whose perturbation moves a bit of Gu or Gv"""
    hit = np.zeros(h[name].shape, bool)
    for cell in np.ndindex(*h[name].shape):
        b = dict(h)
        b[name] = h[name].copy()
        b[name][cell] *= 1.25
        t = _terms(b, size, halo)
        hit[cell] = same_bits(t["Gu"], base["Gu"]) + same_bits(t["Gv"], base["Gv"]) > 0
    return hit


def test_cells_read_found_by_perturbation_are_the_headers():
    """every cell of u, v and w scaled by 1.25 in turn, in a flow where u, v, w are positive everywhere and in one where they are
    negative (so every window is taken once to each side): the cells that move a bit of Gu or Gv are EXACTLY cells_read's, which is the
    list of the header.  (4, 3, 2) at halo (3, 3, 1) is the smallest shape served: every arm ends on the last halo cell."""
    size, halo = (4, 3, 2), (3, 3, 1)
    read = ref.cells_read(size, halo)
    found = {k: np.zeros(read[k].shape, bool) for k in ("u", "v", "w")}
    for sgn in (1, -1):
        h = _random(size, halo, F64, seed=6)
        for k in ("u", "v", "w"):
            h[k] = sgn * (np.abs(h[k]) + 0.25)
        base = _terms(h, size, halo)
        for k in found:
            found[k] |= _reached(h, size, halo, k, base)
    for k in found:
        assert np.array_equal(found[k], read[k]), (k, np.argwhere(found[k] != read[k])[:10])
    # the header's list, spelt out: rows and columns of the crosses relative to a node
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    want = {"u": [(di, 0) for di in range(-3, 4)] + [(di, -1) for di in range(-2, 4)] + [(0, dj) for dj in range(-3, 4)] + [(1, dj) for dj in range(-3, 3)],
            "v": [(0, dj) for dj in range(-3, 4)] + [(-1, dj) for dj in range(-2, 4)] + [(di, 0) for di in range(-3, 4)] + [(di, 1) for di in range(-3, 3)],
            "w": [(di, 0) for di in range(-2, 2)] + [(0, dj) for dj in range(-2, 2)],
            "dx_fc": [(0, dj) for dj in range(-3, 4)] + [(di, dj) for di in range(-2, 4) for dj in (-1, 0)],
            "dy_cf": [(di, dj) for di in (-1, 0) for dj in range(-2, 4)] + [(di, 0) for di in range(-3, 4)],
            "az_ff": [(0, dj) for dj in range(-2, 4)] + [(di, 0) for di in range(-2, 4)],
            "dy_fc": [(di, 0) for di in range(-3, 4)] + [(di, dj) for di in (0, 1) for dj in range(-3, 3)],
            "dx_cf": [(0, dj) for dj in range(-3, 4)] + [(di, dj) for di in range(-3, 3) for dj in (0, 1)],
            "az_cc": [(di, 0) for di in range(-2, 2)] + [(0, dj) for dj in range(-2, 2)], "az_fc": [(0, 0)], "az_cf": [(0, 0)]}
    for k, cells in want.items():
        assert {(di, dj) for name, di, dj, dk in ref.STENCIL if name == k} == set(cells), k
    assert {dk for name, di, dj, dk in ref.STENCIL if name == "w"} == {0, 1}
    assert ref.z_planes_read(size, halo).tolist() == [True] * (Nz + 2)         # Hz = 1: the planes 0 .. Nz + 1, all of them


def test_the_z_arm_follows_the_order_table():
    """Nz = 9, a halo of 3 in z: whatever the sign of w, no plane beyond 0 and Nz + 1 moves anything, and a level moves exactly the nodes
    whose two faces read it by the order table"""
    size, halo = (4, 3, 9), (3, 3, 3)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    for sgn in (1, -1):
        h = _random(size, halo, F64, seed=7)
        h["w"] = sgn * (np.abs(h["w"]) + 0.25)
        base = _terms(h, size, halo)
        assert ((base["Wu"] >= 0) == (sgn > 0)).all()
        for plane in range(Nz + 2 * Hz):
            b = dict(h)
            b["u"] = h["u"].copy()
            b["u"][plane, Hy + 1, Hx + 2] *= 1.25                  # node (3, 2), level plane - Hz + 1
            t = _terms(b, size, halo)
            moved = t["Gu"][:, 1, 2].view(np.uint64) != base["Gu"][:, 1, 2].view(np.uint64)
            level = plane - Hz + 1
            faces = []
            for f in range(1, Nz + 2):
                order = ref.face_order(f, Nz)
                cells = {2: (f - 1, f), 1: (f - 1,) if sgn > 0 else (f,), 3: (f - 2, f - 1, f) if sgn > 0 else (f + 1, f, f - 1),
                         5: tuple(range(f - 3, f + 2)) if sgn > 0 else tuple(range(f - 2, f + 3))}[order]
                faces.append(level in cells)
            want = np.array([faces[k - 1] or faces[k] or k == level for k in range(1, Nz + 1)])
            assert np.array_equal(moved, want), (sgn, level, moved, want)
            if level < 0 or level > Nz + 1:
                assert not moved.any()


@pytest.mark.parametrize("positive", [True, False], ids=["positive", "negative"])
def test_dependence_window_is_what_moves(positive):
    """u, v, w of one sign; one cell of u or v scaled by 1.25: the nodes of Gu, Gv whose bits move are exactly dependence_window's, for a
    cell in the middle, one in the west halo, one in the Zipper rows and one below the column's first level"""
    size, halo = (12, 9, 9), (3, 3, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _random(size, halo, F64, seed=8)
    for k in ("u", "v", "w"):
        h[k] = (1 if positive else -1) * (np.abs(h[k]) * 0.5 + 0.5)
    base = _terms(h, size, halo)
    for name in ("u", "v"):
        for cell in ((Hz + 4, Hy + 4, Hx + 5), (Hz + 1, Hy + 3, Hx - 2), (Hz + 7, Hy + Ny + 1, Hx + 6), (0, Hy + 2, Hx + 3)):
            b = dict(h)
            b[name] = h[name].copy()
            b[name][cell] *= 1.25
            changed = np.zeros(h[name].shape, bool)
            changed[cell] = True
            window = ref.dependence_window(name, changed, size, halo, positive, positive, positive)
            t = _terms(b, size, halo)
            for q, G in enumerate(("Gu", "Gv")):
                moved = t[G].view(np.uint64) != base[G].view(np.uint64)
                assert np.array_equal(moved, window[q]), (name, cell, G, np.argwhere(moved != window[q])[:8])


def test_the_header_states_the_rule_the_reference_states():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "tripolar_hip_weno_vi.h")).read()
    for piece in ("C4(a, b, c, d) = (T(7)/T(12)) * (b + c) - (T(1)/T(12)) * (a + d)", "W5F(q; q) is R(q), the same bits",
                  "vu  = (uu * (dvs + dur) + (FZu[i,j,k+1] - FZu[i,j,k])) / (az_fc[i,j] * dz_c[k])", "bu  = (kur + kus) / dx_fc[i,j]",
                  "Gu[i,j,k] = -((hu + vu) + bu)", "Gv[i,j,k] = -((hv + vvert) + bv)", "true for -0 and false for NaN", "A zero divisor divides",
                  "u at (-3..+3, 0), (-2..+3, -1), (0, -3..+3) and", "w at the faces k, k+1 at (-2..+1, 0) and (0, -2..+1)",
                  "Hx >= 3, Hy >= 3, Hz >= 1", "has one definition"):
        assert piece in text, piece
