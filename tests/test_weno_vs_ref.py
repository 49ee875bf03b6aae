"""The numpy statement of the rule of include/tripolar_hip_weno_vs.h (tests/weno_vs_ref.py), held to properties without the kernel: what
W5V is (R where the three functions are one, the linear fifth-order value where the velocities are constant, whatever the vorticity does),
what the rule gives on a flow whose answer is known (constant u and v over drawn metrics), the cells it reads, found by perturbing every
cell and compared with weno_vi_ref.cells_read, the mirror image in x, and -- on the very cases tests/test_gpu_weno_vs.py draws -- that hu
and hv differ in bits from the DefaultStencil ones, so that a call which launched the DefaultStencil form could not pass there."""
import os

import numpy as np
import pytest

import weno_momentum_ref
import weno_vi_ref
import weno_vs_ref as ref
from test_weno_vi_ref import _mirror, _random           # the drawn problems and the mirror of the rule this one extends
from weno_ref import face_value
from weno_vs_ref import METRICS, same_bits

F32, F64 = np.float32, np.float64


def _terms(h, size, halo):
    return ref.terms(h["u"], h["v"], h["w"], {k: h[k] for k in METRICS}, h["dz_c"], size, halo)


# ---- W5V -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_w5v_of_one_function_is_r(dtype):
    """W5V(q; q; q) is R(q) bit for bit on values drawn in [-1, 1]: bA = bB, x + x and T(0.5) * (2x) are exact (no indicator overflows
    or goes subnormal there; a zero indicator stays zero).  Another smoothness function gives other bits"""
    rng = np.random.default_rng(1)
    q = [rng.uniform(-1, 1, 8192).astype(dtype) for _ in range(5)]
    for n in range(5):
        q[n][:4] = [0.0, -0.0, 1.0, -1.0]                          # and a constant window: every indicator 0
    assert same_bits(ref.face_value_vs(q, q, q), face_value(*q)) == 0
    other = [rng.uniform(-1, 1, 8192).astype(dtype) for _ in range(5)]
    assert same_bits(ref.face_value_vs(q, other, q), face_value(*q)) > 8000
    assert same_bits(ref.face_value_vs(q, q, other), face_value(*q)) > 8000
    assert same_bits(ref.face_value_vs(q, other, other), weno_vi_ref.face_value_fs(q, other)) == 0     # and W5F where a = b


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_w5v_of_constant_velocities_is_the_linear_value_whatever_q_does(dtype):
    """a, b constant: every indicator is 0, tau = 0, the weights are K(3,10), K(3,5), K(1,10) exactly, and the value is
    ((K(3,10) p0 + K(3,5) p1) + K(1,10) p2) / ((K(3,10) + K(3,5)) + K(1,10)) bit for bit -- for a random q and for a step in q, where R
    itself falls back onto one candidate: the weights of a smooth velocity ignore a rough vorticity"""
    rng = np.random.default_rng(2)
    a, b = [np.full(1000, 1.75, dtype)] * 5, [np.full(1000, -0.375, dtype)] * 5
    q = [rng.uniform(-2, 2, 1000).astype(dtype) for _ in range(5)]
    assert same_bits(ref.face_value_vs(q, a, b), ref.linear5(*q)) == 0
    for at in range(1, 5):
        step = [np.full(1000, 0.0 if n < at else 1.0, dtype) for n in range(5)]
        got = ref.face_value_vs(step, a, b)
        assert same_bits(got, ref.linear5(*step)) == 0
        assert np.abs(face_value(*step) - got).max() > 1e-3        # R does not give the linear value on a step
    q64 = [x.astype(F64) for x in q]
    linear = (2 * q64[0] - 13 * q64[1] + 47 * q64[2] + 27 * q64[3] - 3 * q64[4]) / 60
    assert np.abs(ref.face_value_vs(q, a, b) - linear).max() <= 32 * np.finfo(dtype).eps


# ---- a flow whose answer is known ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("speeds", [(0.75, 0.5), (-0.75, -0.5), (0.25, -1.0)])
def test_constant_velocities_over_drawn_metrics_give_the_linear_flux(dtype, speeds):
    """u and v constant, the metrics drawn in [0.5, 2]: UB and VB are constant, Z is rough (it carries the metrics), and
    hu = -(vhat * linear5(Z window)), hv = uhat * linear5(Z window) bit for bit, with the windows chosen by the signs"""
    size, halo = (8, 7, 2), (3, 3, 1)
    h = _random(size, halo, dtype, seed=3)
    h["u"][:], h["v"][:] = speeds
    t = _terms(h, size, halo)
    m = {k: h[k] for k in METRICS}
    Z = lambda di, dj: weno_momentum_ref.zeta_at(h["u"], h["v"], m, size, halo, di, dj)      # noqa: E731
    assert ((t["vhat"] >= 0) == (speeds[1] >= 0)).all() and ((t["uhat"] >= 0) == (speeds[0] >= 0)).all()
    rows = range(-2, 3) if speeds[1] >= 0 else range(3, -2, -1)
    cols = range(-2, 3) if speeds[0] >= 0 else range(3, -2, -1)
    with np.errstate(all="ignore"):
        hu = -(t["vhat"] * ref.linear5(*(Z(0, dj) for dj in rows)))
        hv = t["uhat"] * ref.linear5(*(Z(di, 0) for di in cols))
    assert same_bits(t["hu"], hu) == 0 and same_bits(t["hv"], hv) == 0
    old = weno_vi_ref.terms(h["u"], h["v"], h["w"], m, h["dz_c"], size, halo)
    assert same_bits(t["hu"], old["hu"]) > 0.9 * hu.size and same_bits(t["hv"], old["hv"]) > 0.9 * hv.size    # DefaultStencil sees the rough Z


# ---- the cells read ---------------------------------------------------------------------------------------------------------------------------
def test_cells_read_found_by_perturbation_are_weno_vis():
    """every cell of u, v, w and of the eight metric planes scaled by 1.25 in turn, in a flow where u, v, w are positive everywhere and in
    one where they are negative (so every window is taken once to each side): the cells that move a bit of Gu or Gv are EXACTLY
    weno_vi_ref.cells_read's -- the smoothness inputs read no cell the built rule does not read.  (4, 3, 2) at halo (3, 3, 1) is the
    smallest shape served: every arm ends on the last halo cell"""
    size, halo = (4, 3, 2), (3, 3, 1)
    assert ref.cells_read is weno_vi_ref.cells_read
    read = ref.cells_read(size, halo)
    found = {k: np.zeros(read[k].shape, bool) for k in read}
    for sgn in (1, -1):
        h = _random(size, halo, F64, seed=6)
        for k in ("u", "v", "w"):
            h[k] = sgn * (np.abs(h[k]) + 0.25)
        base = _terms(h, size, halo)
        for name in found:
            for cell in np.ndindex(*h[name].shape):
                b = dict(h)
                b[name] = h[name].copy()
                b[name][cell] *= 1.25
                t = _terms(b, size, halo)
                found[name][cell] |= same_bits(t["Gu"], base["Gu"]) + same_bits(t["Gv"], base["Gv"]) > 0
    for k in found:
        assert np.array_equal(found[k], read[k]), (k, np.argwhere(found[k] != read[k])[:10])


def test_the_smoothness_inputs_alone_read_the_cells_the_header_lists():
    """UB[i, j-2..j+3] reads u at (0, -3..+3), VB[i, j-2..j+3] v at (-1..0, -2..+3), UB[i-2..i+3, j] u at (-2..+3, -1..0) and
    VB[i-2..i+3, j] v at (-3..+3, 0): found by perturbation of ub and vb themselves, and all inside weno_vi_ref.STENCIL"""
    size, halo = (4, 3, 1), (3, 3, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    h = _random(size, halo, F64, seed=9)
    windows = {"uy": [(0, dj) for dj in range(-2, 4)], "ux": [(di, 0) for di in range(-2, 4)]}
    want = {("u", "uy"): {(0, dj) for dj in range(-3, 4)}, ("v", "uy"): {(di, dj) for di in (-1, 0) for dj in range(-2, 4)},
            ("u", "ux"): {(di, dj) for di in range(-2, 4) for dj in (-1, 0)}, ("v", "ux"): {(di, 0) for di in range(-3, 4)}}
    for (name, win), cells in want.items():
        f = ref.ub if name == "u" else ref.vb
        base = [f(h[name], size, halo, di, dj) for di, dj in windows[win]]
        found = set()
        node = (0, 1, 1)                                           # the node (i, j) = (2, 2) of level 1
        for cell in np.ndindex(*h[name].shape):
            b = h[name].copy()
            b[cell] *= 1.25
            if any(x[node] != y[node] for x, y in zip(base, (f(b, size, halo, di, dj) for di, dj in windows[win]))):
                found.add((cell[2] - Hx - 1, cell[1] - Hy - 1))
        assert found == cells, (name, win, sorted(found))
        assert cells <= {(di, dj) for n, di, dj, dk in weno_vi_ref.STENCIL if n == name}


# ---- symmetry ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_mirror_symmetry_in_x(dtype):
    """the rule applied to the mirror image of a flow in x is the mirror image of the rule's result, bit for bit: UB goes over into UB of
    the mirrored node, VB = T(0.5) * (v[i-1] + v[i]) is a sum of two, and every upwind window goes over into the other one"""
    size, halo = (8, 7, 3), (4, 4, 4)
    h = _random(size, halo, dtype, seed=4)
    t, tm = _terms(h, size, halo), _terms(_mirror(h, -1), size, halo)
    assert same_bits(tm["Gu"][:, :, 1:], -t["Gu"][:, :, :0:-1]) == 0
    assert same_bits(tm["Gv"], t["Gv"][:, :, ::-1]) == 0
    assert same_bits(tm["hu"][:, :, 1:], -t["hu"][:, :, :0:-1]) == 0 and same_bits(tm["hv"], t["hv"][:, :, ::-1]) == 0


# ---- the GPU file's cases ---------------------------------------------------------------------------------------------------------------------------
def test_on_every_case_of_the_gpu_file_the_stencil_shows_in_the_bits():
    """On every case tests/test_gpu_weno_vs.py draws (its ALL, BIGGER, SELECT and the band problem), hu and hv of this rule differ in bits
    from weno_vi_ref's, and so do the reference outputs Gu, Gv: a call that launched the DefaultStencil form fails there.  Observed on
    the CPU: the least share of interior nodes on which one of hu, hv, Gu, Gv differs, over all the cases, is 0.99994 (uniform draws: the
    velocities' indicators do not equal the vorticity's).  Asserted: more than 0.9 on every case and quantity"""
    import tendency_windows as tw
    import test_gpu_weno_vs as G
    cases = [c for c, _, _ in G.ALL + G.BIGGER] + list(G.SELECT)
    problems = [(G._case(c), c[0], c[1]) for c in cases]
    problems += [(tw.draw(G.KERNEL, G.BANDS[0], G.BANDS[1][dtype], dtype), G.BANDS[0], G.BANDS[1][dtype]) for dtype in (F64, F32)]
    shares = []
    for h, size, halo in problems:
        m = {k: h[k] for k in METRICS}
        new = ref.terms(h["u"], h["v"], h["w"], m, h["dz_c"], size, halo)
        old = weno_vi_ref.terms(h["u"], h["v"], h["w"], m, h["dz_c"], size, halo)
        for k in ("hu", "hv", "Gu", "Gv"):
            shares.append(same_bits(new[k], old[k]) / new[k].size)
            assert shares[-1] > 0.9, (size, halo, k, shares[-1])
        for k in ("vu", "bu", "vv", "bv"):
            assert same_bits(new[k], old[k]) == 0                  # everything else is weno_vi's, bit for bit
    print("least share of differing nodes", min(shares))


def test_the_header_states_the_rule_the_reference_states():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = " ".join(open(os.path.join(root, "include", "tripolar_hip_weno_vs.h")).read().replace("\n *", " ").split())   # line breaks do not count
    for piece in ("UB[i,j,k] = T(0.5) * (u[i,j-1,k] + u[i,j,k])", "VB[i,j,k] = T(0.5) * (v[i-1,j,k] + v[i,j,k])",
                  "b_s = T(0.5) * (bA_s + bB_s)", "W5V(Z[i, j-2..j+2]; UB[i, j-2..j+2]; VB[i, j-2..j+2])",
                  "W5V(Z[i+3..i-1, j]; UB[i+3..i-1, j]; VB[i+3..i-1, j])", "hu = -(vhat * zr)", "hv = uhat * zr",
                  "true for -0 and", "W5V(q; q; q) is R(q) bit for bit", "UB[i, j-2..j+3] reads u at (0, -3..+3)",
                  "VB[i-2..i+3, j] reads v at (-3..+3, 0)", "halo (3, 3, 1)", "via tau = |b0 - b2|", "one definition",
                  "[recalled: Oceananigans' biased WENO weights for VelocityStencil"):
        assert piece in text, piece
