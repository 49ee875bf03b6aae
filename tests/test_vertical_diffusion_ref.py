"""tests/vertical_diffusion_ref.py, the numpy statement of the rule of tpg_vertical_implicit_diffusion, held to properties (no GPU): the
dense solve of the same matrix in long double, the maximum principle, the identities, the decay of a cosine mode, the agreement of the three
kappa forms and of the two statements of the rule, the masked column, the elided division and the cells read."""
import numpy as np
import pytest

import vertical_diffusion_ref as R

TYPES = [np.float64, np.float32]
IDS = ["f64", "f32"]
LD = np.longdouble


def _column(rng, Nz, T, kappa_hi=2.0):
    f = rng.uniform(-1, 1, Nz).astype(T)
    kappa = rng.uniform(0, kappa_hi, Nz + 1).astype(T)
    dz_c, dz_f = rng.uniform(0.5, 2, Nz).astype(T), rng.uniform(0.5, 2, Nz + 1).astype(T)
    return f, kappa, dz_c, dz_f


def _dense(kappa, dz_c, dz_f, dt, k0=1):
    """the matrix of the wet levels k0..Nz (1-based) in long double, its coefficients evaluated in long double from the same inputs"""
    Nz = len(dz_c)
    n = Nz - k0 + 1
    A = np.zeros((n, n), LD)
    kap, dzc, dzf = (np.concatenate([[0], np.asarray(a, LD)]) for a in (kappa, dz_c, dz_f))       # 1-based
    for k in range(k0, Nz + 1):
        A[k - k0, k - k0] = 1
    for k in range(k0 + 1, Nz + 1):                                # face k between the cells k - 1 and k
        up = -(LD(dt) * kap[k] / dzc[k - 1] / dzf[k])
        lo = -(LD(dt) * kap[k] / dzc[k] / dzf[k])
        A[k - 1 - k0, k - k0] = up
        A[k - 1 - k0, k - 1 - k0] -= up
        A[k - k0, k - 1 - k0] = lo
        A[k - k0, k - k0] -= lo
    return A


def _gauss(A, b):
    """dense elimination with partial pivoting in long double"""
    A, b = A.copy(), np.asarray(b, LD).copy()
    n = len(b)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, p]], b[[c, p]] = A[[p, c]], b[[p, c]]
        for r in range(c + 1, n):
            m = A[r, c] / A[c, c]
            A[r, c:] -= m * A[c, c:]
            b[r] -= m * b[c]
    x = np.zeros(n, LD)
    for r in range(n - 1, -1, -1):
        x[r] = (b[r] - A[r, r + 1:] @ x[r + 1:]) / A[r, r]
    return x


@pytest.mark.parametrize("T", TYPES, ids=IDS)
def test_agrees_with_a_dense_long_double_solve(T):
    """|phi - x| <= 16 eps(T) ||A||inf max|f|: A is row-diagonally dominant with unit row sums, so ||A^-1||inf <= 1; the Thomas sweep is
    componentwise backward stable with a factor of about 4 eps, and each coefficient carries three more roundings.  Derived, not tuned; the
    largest ratio seen is printed (DESIGN.md 6 records it)"""
    assert np.finfo(LD).eps < np.finfo(np.float64).eps / 100
    rng = np.random.default_rng(11)
    eps, worst = np.finfo(T).eps, 0.0
    for trial in range(120):
        Nz = int(rng.integers(1, 25))
        f, kappa, dz_c, dz_f = _column(rng, Nz, T, kappa_hi=(2.0, 50.0)[trial % 2])
        count = None if trial % 3 else int(rng.integers(0, Nz))
        dt = float(T(rng.uniform(0.1, 3)))
        k0 = R.first_wet(count, Nz)
        phi = R.solve_column(f, kappa, dz_c, dz_f, dt, count)
        A = _dense(kappa, dz_c, dz_f, dt, k0)
        x = _gauss(A, f[k0 - 1:])
        assert np.allclose(np.asarray(A.sum(axis=1), np.float64), 1.0, atol=1e-14)              # unit row sums
        bound = 16 * eps * float(np.abs(A).sum(axis=1).max()) * float(np.abs(f[k0 - 1:]).max())
        err = float(np.abs(np.asarray(phi[k0 - 1:], LD) - x).max())
        assert err <= bound, (trial, err, bound)
        worst = max(worst, err / bound)
    print(f"\n[vertical diffusion ref] {np.dtype(T).name}: largest error / bound over 120 columns = {worst:.3f}")


@pytest.mark.parametrize("T", TYPES, ids=IDS)
def test_maximum_principle(T):
    """min f <= phi <= max f for kappa >= 0, to within 4 eps(T) max|f|; the largest excess seen is printed"""
    rng = np.random.default_rng(12)
    eps, worst = float(np.finfo(T).eps), 0.0
    for trial in range(20):                                        # 20 draws of 100 columns: 2000 columns
        Nz, cols = int(rng.integers(1, 30)), 100
        f = rng.uniform(-1, 1, (Nz, cols)).astype(T)
        kappa = rng.uniform(0, 2, (Nz + 1, cols)).astype(T)
        dz_c, dz_f = rng.uniform(0.5, 2, Nz).astype(T), rng.uniform(0.5, 2, Nz + 1).astype(T)
        phi = R.solve_columns(f, kappa, dz_c, dz_f, float(rng.uniform(0, 5)))
        scale = np.abs(f).max(axis=0).astype(np.float64)
        over = np.maximum(phi.max(axis=0).astype(np.float64) - f.max(axis=0), f.min(axis=0).astype(np.float64) - phi.min(axis=0))
        excess = float((np.maximum(over, 0) / (eps * scale)).max())
        assert excess <= 4, (trial, excess)
        worst = max(worst, excess)
    print(f"\n[vertical diffusion ref] {np.dtype(T).name}: largest excess over [min f, max f] on 2000 columns = {worst:.2f} eps")


@pytest.mark.parametrize("T", TYPES, ids=IDS)
def test_identities(T):
    """kappa = 0 or dt = 0 returns f bit for bit; so does Nz = 1 with any kappa"""
    rng = np.random.default_rng(13)
    for Nz in (1, 2, 7):
        f, kappa, dz_c, dz_f = _column(rng, Nz, T)
        assert (f != 0).all()
        assert np.array_equal(R.solve_column(f, np.zeros(Nz + 1, T), dz_c, dz_f, 0.7), f)
        assert np.array_equal(R.solve_column(f, kappa, dz_c, dz_f, 0.0), f)
        assert np.array_equal(R.solve_columns(f[:, None], kappa, dz_c, dz_f, 0.0)[:, 0], f)
    f, kappa, dz_c, dz_f = _column(rng, 1, T)
    assert np.array_equal(R.solve_column(f, kappa, dz_c, dz_f, 3.0), f)


def _mode(Nz, m=1, H=1.0):
    z = (np.arange(Nz) + 0.5) * (H / Nz)
    return np.cos(np.pi * m * z / H)


def _decay_rate(Nz, dt, kappa=1.0, H=1.0):
    """-lambda_h estimated from ONE step on the cosine mode: phi = f / (1 + dt kappa |lambda_h|) on a uniform grid with no-flux ends"""
    dz = H / Nz
    f = _mode(Nz)
    phi = R.solve_column(f, np.full(Nz + 1, kappa), np.full(Nz, dz), np.full(Nz + 1, dz), dt)
    ratio = f / phi
    assert np.ptp(ratio) < 1e-9 * abs(ratio[0])                    # the mode is an eigenvector of the discrete operator
    return (float(ratio.mean()) - 1) / (dt * kappa)


def test_cosine_mode_decays_at_second_order_in_dz_and_first_in_dt():
    exact = np.pi ** 2
    errs = [abs(_decay_rate(Nz, 1e-2) - exact) for Nz in (16, 32, 64)]
    for coarse, fine in zip(errs, errs[1:]):
        assert 3.8 < coarse / fine < 4.2, errs                     # second order in dz
    # first order in dt: n steps to the time 0.1 against the semi-discrete decay exp(-lambda_h t), lambda_h = (4 / dz^2) sin^2(pi dz / 2)
    Nz, t_end = 32, 0.1
    dz = 1.0 / Nz
    lam = 4 / dz ** 2 * np.sin(np.pi * dz / 2) ** 2
    out = []
    for n in (20, 40, 80):
        phi = _mode(Nz)
        for _ in range(n):
            phi = R.solve_column(phi, np.ones(Nz + 1), np.full(Nz, dz), np.full(Nz + 1, dz), t_end / n)
        out.append(abs(phi[0] / _mode(Nz)[0] - np.exp(-lam * t_end)))
    for coarse, fine in zip(out, out[1:]):
        assert 1.9 < coarse / fine < 2.1, out


@pytest.mark.parametrize("T", TYPES, ids=IDS)
def test_the_two_statements_and_the_three_forms_agree_bit_for_bit(T):
    rng = np.random.default_rng(14)
    for trial in range(200):
        Nz, cols = int(rng.integers(1, 12)), 5
        f = rng.uniform(-1, 1, (Nz, cols)).astype(T)
        kap = rng.uniform(-0.5, 2, (Nz + 1, cols)).astype(T)
        dz_c, dz_f = rng.uniform(0.5, 2, Nz).astype(T), rng.uniform(0.5, 2, Nz + 1).astype(T)
        counts = rng.integers(-2, Nz + 3, cols) if trial % 3 else None
        many = R.solve_columns(f, kap, dz_c, dz_f, 0.7, counts, 0.0)
        for c in range(cols):
            one = R.solve_column(f[:, c], kap[:, c], dz_c, dz_f, 0.7, None if counts is None else counts[c], 0.0)
            assert np.array_equal(many[:, c], one) and np.array_equal(np.signbit(many[:, c]), np.signbit(one)), (trial, c)
    size, halo = (6, 3, 5), (2, 1, 1)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    parent = rng.uniform(-1, 1, (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)).astype(T)
    dz_c, dz_f = rng.uniform(0.5, 2, Nz).astype(T), rng.uniform(0.5, 2, Nz + 1).astype(T)
    counts = rng.integers(-1, Nz + 2, (Ny, Nx))
    value = 0.37
    forms = [R.reference([parent], value, R.CONSTANT, dz_c, dz_f, 0.7, size, halo, counts)[0],
             R.reference([parent], np.full(Nz + 1, T(value), T), R.PROFILE, dz_c, dz_f, 0.7, size, halo, counts)[0],
             R.reference([parent], np.full(parent.shape, T(value), T), R.FIELD, dz_c, dz_f, 0.7, size, halo, counts)[0]]
    assert np.array_equal(forms[0], forms[1]) and np.array_equal(forms[0], forms[2]) and not np.array_equal(forms[0], parent)
    inner = (slice(Hz, Hz + Nz), slice(Hy, Hy + Ny), slice(Hx, Hx + Nx))
    halo_mask = np.ones(parent.shape, bool)
    halo_mask[inner] = False
    assert np.array_equal(forms[0][halo_mask], parent[halo_mask])    # the halos are as they were


@pytest.mark.parametrize("T", TYPES, ids=IDS)
def test_a_masked_column_is_the_unmasked_solve_of_its_wet_levels(T):
    rng = np.random.default_rng(15)
    Nz = 9
    f, kappa, dz_c, dz_f = _column(rng, Nz, T)
    for count in (-3, 0, 1, 4, Nz - 1, Nz, Nz + 2):
        m = min(max(count, 0), Nz)
        got = R.solve_column(f, kappa, dz_c, dz_f, 0.7, count, mask_value=-5.0)
        assert np.array_equal(got[:m], np.full(m, -5, T))
        if m < Nz:
            assert np.array_equal(got[m:], R.solve_column(f[m:], kappa[m:], dz_c[m:], dz_f[m:], 0.7))
    assert np.array_equal(R.solve_column(f, kappa, dz_c, dz_f, 0.7, Nz), np.zeros(Nz, T))                # a column that is all mask


@pytest.mark.parametrize("T", TYPES, ids=IDS)
def test_the_elided_division(T):
    """kappa = -0.5, dz = 1, dt = 1, Nz = 2, f = (3, 7): beta is exactly 0 at level 2 and the select takes its second arm: (-1, 7)"""
    f, ones = np.array([3, 7], T), np.ones(3, T)
    got = R.solve_column(f, np.full(3, -0.5, T), ones[:2], ones, 1.0)
    assert np.array_equal(got, np.array([-1, 7], T))
    assert np.array_equal(R.solve_columns(f[:, None], np.full(3, -0.5, T), ones[:2], ones, 1.0)[:, 0], got)
    A = _dense(np.full(3, -0.5), ones[:2], ones, 1.0)
    assert float(A[0, 0]) == 0.5 and float(A[1, 0]) == 0.5         # the matrix of the case: singular after the first elimination


@pytest.mark.parametrize("count", [None, 0, 3, 5, 6])
def test_the_cells_read_are_found_by_perturbing_every_cell(count):
    """every entry of f, kappa, dz_c, dz_f changed in turn: the result changes exactly where the header says the entry is read -- f and dz_c
    at the wet levels k0..Nz (dz_c not at all where one level is wet), kappa and dz_f at the faces k0+1..Nz.  (A NaN is no probe: a NaN
    beta takes the select's second arm and can be swallowed there)"""
    T, Nz = np.float64, 6
    rng = np.random.default_rng(17)
    f, kappa, dz_c, dz_f = _column(rng, Nz, T)
    base = R.solve_column(f, kappa, dz_c, dz_f, 0.7, count)
    k0 = R.first_wet(count, Nz)
    wet = set(range(k0, Nz + 1))
    faces = set(range(k0 + 1, Nz + 1))
    read = {"f": wet, "kappa": faces, "dz_c": wet if faces else set(), "dz_f": faces}
    arrays = {"f": f, "kappa": kappa, "dz_c": dz_c, "dz_f": dz_f}
    for name, a in arrays.items():
        for q in range(len(a)):                                    # entry q is level / face q + 1
            moved = {k: v.copy() for k, v in arrays.items()}
            moved[name][q] = a[q] * 1.5 + 0.25
            changed = not np.array_equal(R.solve_column(moved["f"], moved["kappa"], moved["dz_c"], moved["dz_f"], 0.7, count), base)
            assert changed == ((q + 1) in read[name]), (name, q + 1, changed)
