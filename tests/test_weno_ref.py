"""The numpy reference of the WENO5 tracer tendency (tests/weno_ref.py) checked on its own, without a GPU: the face value R is fifth-order
on smooth data, does not overshoot a step, is the linear fifth-order upwind value where the smoothness indicators agree, its mirrored
selection is the reversed array's result reversed, the tendency degenerates to the centred one with u = v = 0, reads exactly its stencil,
and a changed cell reaches exactly the nodes the rule says."""
import numpy as np
import pytest

import advection_ref
import weno_ref
from weno_ref import face_value, same_bits, upwind_face_value

F32, F64 = np.float32, np.float64


def _left_biased(c):
    """R at the faces i + 1/2 of a periodic row of cell values, biased to the left: q2 = c[i] is the upwind cell"""
    return face_value(*(np.roll(c, -o) for o in range(-2, 3)))


def _max_error(N):
    h = 2 * np.pi / N
    x = (np.arange(N) + 0.5) * h
    averages = np.sin(x) * (np.sin(h / 2) / (h / 2))               # the exact cell averages of sin
    return np.abs(_left_biased(averages) - np.sin(x + h / 2)).max()


def test_fifth_order_convergence_on_smooth_data():
    """exact cell averages of sin on a uniform periodic grid, Float64, against the point value at the face: the max-error ratio for
    N = 32 -> 64 and 64 -> 128 is >= 30 (the asymptote is 32)"""
    e32, e64, e128 = _max_error(32), _max_error(64), _max_error(128)
    print("max errors", e32, e64, e128, "ratios", e32 / e64, e64 / e128)
    assert e32 / e64 >= 30 and e64 / e128 >= 30
    assert e128 < 1e-8


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_no_overshoot_on_a_step(dtype):
    """twenty ones followed by twenty zeros: every reconstructed value, of either bias, stays in [-1e-15, 1 + 1e-15] in Float64"""
    c = np.concatenate([np.ones(20, dtype), np.zeros(20, dtype)])
    x = [c[o:o + 35] for o in range(6)]                            # the six cells around the faces 3 .. 37
    left = upwind_face_value(np.ones(35, dtype), x)
    right = upwind_face_value(-np.ones(35, dtype), x)
    tol = 1e-15 if dtype == F64 else 1e-6                          # Float32: a few ulp of 1, the same property in the narrower type
    for r in (left, right):
        print("step", dtype.__name__, r.min(), r.max())
        assert r.min() >= -tol and r.max() <= 1 + tol
    assert (left[:14] == 1).all() and (left[-14:] == 0).all()      # away from the step the data are constant


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_linear_data_gives_the_linear_upwind_value(dtype):
    """on data linear in the index (small integers) b0 = b1 = b2, tau = 0 and the weights are the linear ones:
    R = (2 q0 - 13 q1 + 47 q2 + 27 q3 - 3 q4) / 60 to a few ulp"""
    for a, b in ((0, 1), (5, -2), (-7, 3), (4, 0)):
        q = [np.array([a + b * n], dtype) for n in range(5)]
        exact = (2 * (a + 0 * b) - 13 * (a + b) + 47 * (a + 2 * b) + 27 * (a + 3 * b) - 3 * (a + 4 * b)) / 60
        got = face_value(*q)[0]
        scale = max(abs(a) + 4 * abs(b), 1)
        assert abs(float(got) - exact) <= 4 * np.finfo(dtype).eps * scale, (a, b, got, exact)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_mirrored_selection_is_the_reversed_arrays_result_reversed(dtype):
    rng = np.random.default_rng(5)
    n = 40
    c = rng.uniform(-1, 1, n).astype(dtype)
    faces = np.arange(3, n - 2)                                    # face f lies between the cells f - 1 and f
    cells = lambda a: [a[faces + o] for o in range(-3, 3)]         # noqa: E731
    right = upwind_face_value(-np.ones(faces.size, dtype), cells(c))             # R(c[f+2], c[f+1], c[f], c[f-1], c[f-2])
    left_of_reversed = upwind_face_value(np.ones(faces.size, dtype), cells(c[::-1].copy()))
    # face f of c is face n - f of the reversed array
    assert np.array_equal(n - faces[::-1], faces)
    assert same_bits(right, left_of_reversed[::-1]) == 0
    assert same_bits(right, upwind_face_value(np.ones(faces.size, dtype), cells(c))) > 0
    # -0 selects as +0 does, NaN as a negative flow does
    assert same_bits(upwind_face_value(np.full(faces.size, -0.0, dtype), cells(c)), upwind_face_value(np.ones(faces.size, dtype), cells(c))) == 0
    assert same_bits(upwind_face_value(np.full(faces.size, np.nan, dtype), cells(c)), right) == 0


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


def _G(h, size, halo, **kw):
    a = dict(h)
    a.update(kw)
    return weno_ref.interior_tendency(a["c"], a["u"], a["v"], a["w"], a["dy_fc"], a["dx_cf"], a["az_cc"], a["dz_c"], size, halo)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_degenerates_to_the_centred_tendency_without_horizontal_flow(dtype):
    """u = v = 0, zeros of either sign: the x / y fluxes are zeros of either sign, and adding them changes no bits of the vertical
    divergence for finite c -- G equals advection_ref's centred G with the same w, bit for bit"""
    size, halo = (12, 10, 4), (3, 4, 2)
    h = _random_case(size, halo, dtype)
    rng = np.random.default_rng(2)
    zeros = lambda: np.where(rng.random(h["u"].shape) < 0.5, dtype(0.0), dtype(-0.0)).astype(dtype)     # noqa: E731
    h["u"], h["v"] = zeros(), zeros()
    assert np.signbit(h["u"]).any() and not np.signbit(h["u"]).all()
    # the sign-of-zero cases first: the fluxes are +-0 of both signs; (+-0) + (+-0) is a zero, and x + (+-0) = x for x != 0
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    Mx = (h["dy_fc"][None, Hy:Hy + Ny, Hx:Hx + Nx + 1] * h["dz_c"][:, None, None]) * h["u"][Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx + 1]
    Fx = Mx * upwind_face_value(Mx, [h["c"][Hz:Hz + Nz, Hy:Hy + Ny, Hx + o:Hx + o + Nx + 1] for o in range(-3, 3)])
    assert (Fx == 0).all() and np.signbit(Fx).any() and not np.signbit(Fx).all()
    G = _G(h, size, halo)
    centred = advection_ref.interior_tendency(h["c"], h["u"], h["v"], h["w"], h["dy_fc"], h["dx_cf"], h["az_cc"], h["dz_c"], size, halo)
    assert np.isfinite(G).all() and (G != 0).all()
    assert same_bits(G, centred) == 0
    flowing = _G(_random_case(size, halo, dtype), size, halo)
    assert same_bits(flowing, centred) > 0.9 * G.size


def test_reads_exactly_its_stencil():
    """every cell outside cells_read is NaN: G has no NaN and the same bits; and the cells of c inside it matter: a NaN in one reaches some
    node under a flow of one sign or the other (the selection leaves the far cell of the downwind side unread)"""
    size, halo, dtype = (10, 8, 2), (4, 3, 1), F64
    h = _random_case(size, halo, dtype)
    read = weno_ref.cells_read(size, halo)
    want = _G(h, size, halo)
    poisoned = {k: np.where(read[k], h[k], np.nan) for k in read}
    assert all(np.isnan(poisoned[k]).any() for k in read)
    assert same_bits(_G(h, size, halo, **poisoned), want) == 0
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    corners = read["c"][Hz, :Hy, :Hx]
    assert not corners.any()                                       # a plus-shaped stencil: no corner halo cell
    assert read["c"][Hz, Hy, 0] == (Hx == 3) and read["c"][Hz, Hy, Hx - 3] and read["c"][Hz, Hy, Hx + Nx + 2] and read["c"][Hz, Hy - 3, Hx]
    rng = np.random.default_rng(3)
    cells = np.argwhere(read["c"])
    for k, j, i in cells[rng.choice(len(cells), 60, replace=False)]:
        c = h["c"].copy()
        c[k, j, i] = np.nan
        up, vp = np.abs(h["u"]), np.abs(h["v"])
        assert np.isnan(_G(h, size, halo, c=c, u=up, v=vp)).any() or np.isnan(_G(h, size, halo, c=c, u=-up, v=-vp)).any(), (k, j, i)


@pytest.mark.parametrize("axis,positive", [("x", True), ("x", False), ("y", True), ("y", False)], ids=["u+", "u-", "v+", "v-"])
def test_domain_of_dependence(axis, positive):
    """one-signed flow along one axis, the other velocities zero: adding 1 to c at one interior cell n* changes G at n* + 3 (flow > 0) or
    n* - 3 (flow < 0) and nowhere outside n* - 2 .. n* + 3 (n* - 3 .. n* + 2) of that row and level"""
    size, halo, dtype = (16, 14, 3), (3, 3, 1), F64
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _random_case(size, halo, dtype)
    flow = np.abs(h["u" if axis == "x" else "v"]) + dtype(0.1)
    h["u"], h["v"], h["w"] = np.zeros_like(h["u"]), np.zeros_like(h["v"]), np.zeros_like(h["w"])
    h["u" if axis == "x" else "v"] = flow if positive else -flow
    k, j, i = 1, 6, 7                                              # 0-based interior cell
    c = h["c"].copy()
    c[Hz + k, Hy + j, Hx + i] += 1
    changed = weno_ref.same_bits(_G(h, size, halo), _G(h, size, halo, c=c))
    moved = _G(h, size, halo) != _G(h, size, halo, c=c)
    assert changed == moved.sum()
    window = weno_ref.dependence_window(c != h["c"], size, halo, axis, positive)
    lo, hi = (-2, 3) if positive else (-3, 2)
    expect = np.zeros((Nz, Ny, Nx), bool)
    if axis == "x":
        expect[k, j, i + lo:i + hi + 1] = True
        far = (k, j, i + (3 if positive else -3))
    else:
        expect[k, j + lo:j + hi + 1, i] = True
        far = (k, j + (3 if positive else -3), i)
    assert np.array_equal(window, expect)
    assert not (moved & ~window).any() and moved[far] and moved.sum() == 6
