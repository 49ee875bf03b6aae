"""GPU tests of the vertical mixing diffusivities (tpg_convective_adjustment_diffusivities, tpg_ri_based_diffusivities,
libtripolar_hip_mixing.so): bit for bit against tests/mixing_ref.py on WHOLE parents -- no tolerance anywhere.  The outputs start as a
sentinel, so their halo cells must come back as they were; the inputs must come back unchanged.  NaN sits in every input cell the header
says is not read for the outputs of the call: the z-halo planes, the halo cells beyond the first, the corners, the west column without
kappa_u, the south row without kappa_v, the faces 1 and Nz + 1 and every other halo cell of the *_prev arrays, dz_f[1] and dz_f[Nz+1].

The shapes are the smallest at which each path can go wrong (SHAPES): no evaluated face, one evaluated face, Nx = Hx, Ny = Hy, an odd Hx,
Float32 rows that do not split into 16-B chunks, pointers one element off the 16-B grid, a row wider than one wave of chunks; and one
Float32 case past 2^31 elements, where an offset held in 32 bits would wrap."""
import itertools

import numpy as np
import pytest
import torch

import mixing_ref as R
import special_values as sv
from gpu_harness import _assert_parent, _dev, _free_hbm, _id  # noqa: F401
from mixing_cases import F32, F64, MASK_VALUE, RI, SENTINEL, draw, nan_where_not_read

pytestmark = pytest.mark.gpu

MAIN = ((40, 24, 7), (4, 4, 4))
SHAPES = [((2, 1, 1), (1, 1, 1)), ((2, 1, 2), (1, 1, 1)),          # no evaluated face; one evaluated face
          ((4, 6, 3), (4, 2, 1)),                                  # Nx = Hx
          ((8, 3, 2), (2, 3, 2)),                                  # Ny = Hy
          MAIN, ((40, 24, 7), (5, 5, 5)), ((40, 24, 7), (3, 2, 1)),    # the default halo, the model halo (odd Hx: element-aligned chunks), a mixed one
          ((42, 5, 3), (4, 4, 4)),                                 # Nx = 2 mod 4: 8-B chunks in Float32
          ((260, 4, 3), (4, 4, 4))]                                # 130 Float64 chunks per row: a wave's edge and the periodic seam inside a row
SUBSETS = [s for n in range(1, 5) for s in itertools.combinations(R.OUTPUTS, n)]
COUNTS = [(), ("cc",), ("fc", "cf"), ("cc", "fc", "cf")]


def _run(osg, gpu, p, into, offset=0):
    """the status-checked entry point on device copies of the problem p into device copies of `into` -> {name: whole parent on the host};
    the inputs must be unchanged"""
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    L = osg._lib
    dev = lambda a: None if a is None else _dev(a, gpu, offset)    # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()            # noqa: E731
    ins = {k: dev(p[k]) for k in ("b", "u", "v")}
    prev = (None, None) if p["prev"] is None else tuple(dev(a) for a in p["prev"])
    outs = {k: dev(into[k]) if k in p["outputs"] else None for k in R.OUTPUTS}
    dz_f = dev(p["dz_f"])
    planes = [None if p["counts"][k] is None else _dev(np.ascontiguousarray(p["counts"][k], dtype=np.int32), gpu) for k in ("cc", "fc", "cf")]
    tail = (ptr(dz_f), *(ptr(t) for t in planes), p["mask_value"], *p["size"], *p["halo"], L.ft_of(ins["b"].dtype), L.current_stream_ptr(gpu))
    lib = M.mixing_lib()
    if p["closure"] == "ca":
        status = lib.tpg_convective_adjustment_diffusivities(ptr(ins["b"]), *(ptr(outs[k]) for k in R.OUTPUTS), *(p["params"][k] for k in R.CA_PARAMS), *tail)
    else:
        status = lib.tpg_ri_based_diffusivities(ptr(ins["b"]), ptr(ins["u"]), ptr(ins["v"]), ptr(prev[0]), ptr(prev[1]), *(ptr(outs[k]) for k in R.OUTPUTS),
                                                *(p["params"][k] for k in R.RI_PARAMS), *tail)
    M.check_mixing(status)
    torch.cuda.synchronize()
    for k, t in ins.items():
        if t is not None:
            _assert_parent(t.cpu().numpy(), p[k], ("input unchanged", k))
    for t, a in zip(prev, p["prev"] or ()):
        _assert_parent(t.cpu().numpy(), a, "prev unchanged")
    return {k: outs[k].cpu().numpy() for k in p["outputs"]}


def _check(osg, gpu, p, into, what, offset=0):
    want = R.reference(p, into)
    got = _run(osg, gpu, p, into, offset)
    for name in p["outputs"]:
        _assert_parent(got[name], want[name], (what, name))


# ---- the table: every shape in both types and alignments, the outputs, the time average and the count planes crossed in rotation ---------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: _id((*c, F64))[:-4])
@pytest.mark.parametrize("offset", [0, 1], ids=["16B", "one-element-off"])
@pytest.mark.parametrize("closure", ["ca", "ri"])
def test_whole_parents_are_the_reference_bit_for_bit(osg, gpu, closure, case, dtype, offset):
    size, halo = case
    every = list(itertools.product(SUBSETS, (False, True), COUNTS))
    start = (SHAPES.index(case) * 37 + offset * 11 + (dtype is F32) * 5) % len(every)
    for n in range(8):                                             # eight combinations per closure, shape, type and alignment; all four outputs first
        outputs, prev, counts = (R.OUTPUTS, n % 2 == 1, COUNTS[3]) if n < 2 else every[(start + 29 * n) % len(every)]
        p, into = draw(closure, size, halo, dtype, prev=prev, counts=counts, outputs=outputs, seed=n)
        _check(osg, gpu, p, into, (outputs, prev, counts), offset)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("closure,prev", [("ca", False), ("ri", False), ("ri", True)], ids=["ca", "ri", "ri-prev"])
def test_every_output_subset_with_all_some_and_no_count_planes(osg, gpu, closure, prev, dtype):
    size, halo = MAIN
    for n, outputs in enumerate(SUBSETS):
        for counts in COUNTS:
            p, into = draw(closure, size, halo, dtype, prev=prev, counts=counts, outputs=outputs, seed=n)
            _check(osg, gpu, p, into, (outputs, counts))


def test_the_drawn_problems_reach_every_branch():
    """no GPU: the main case has stable and unstable faces, all three zones of the taper, and masked and open faces at every location"""
    p, into = draw("ri", *MAIN, F64, prev=True, counts=COUNTS[3], nan_unread=False)
    N2, S2, Ri = R.richardson_of(p)
    tau = R.taper(Ri, RI["Ri0"], RI["Ri_delta"])
    assert (N2 < 0).any() and (N2 > 0).any() and (tau == 1).any() and (tau == 0).any() and ((tau > 0) & (tau < 1)).any()
    out = R.reference(p, into)
    Nz = MAIN[0][2]
    for name in R.OUTPUTS:
        n = p["counts"][R.COUNT_OF[name]]
        assert (n < 0).any() and (n > Nz).any() and (n == 0).any() and ((n > 0) & (n < Nz)).any()
        assert (out[name] == F64(MASK_VALUE)).any() and (out[name] == 0).any() and (out[name] == SENTINEL).any()


# ---- special values ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("closure,prev", [("ca", False), ("ri", False), ("ri", True)], ids=["ca", "ri", "ri-prev"])
def test_special_values(osg, gpu, closure, prev, dtype):
    """the pool of IEEE special values (signed zeros, subnormals, the extremes, infinities, NaN) in every cell of b, u and v, rolled so that
    every pair meets in a difference; then planted columns: N2 = +0 and -0, S2 = 0 with N2 > 0 and N2 < 0, Inf / Inf, and differences that
    are Float32 subnormals"""
    size, halo = MAIN
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    pool = sv.pool(dtype)
    p, into = draw(closure, size, halo, dtype, prev=prev, counts=("cc",), nan_unread=False)
    shape = p["b"].shape
    p["b"] = sv.tiled(pool, shape)
    if closure == "ri":
        p["u"], p["v"] = sv.tiled(np.roll(pool, 5), shape), sv.tiled(np.roll(pool, 11), shape)
        if prev:
            p["prev"] = tuple(np.where(np.arange(a.size).reshape(a.shape) % 7 == q, sv.tiled(np.roll(pool, 3 + q), a.shape), a) for q, a in enumerate(p["prev"]))
    tiny = np.finfo(dtype).tiny
    col = lambda a, i, values: a.__setitem__((slice(Hz, Hz + Nz), Hy + 2, Hx + i), np.asarray(values, dtype))       # noqa: E731
    col(p["b"], 0, [1, 1, 1.5, 1.5, -2, -2, 0.0])                  # N2 = +0, > 0, +0, < 0, +0, > 0
    col(p["b"], 1, [1, 1, 0.5, 0.5, 2, 2, 2])
    col(p["b"], 2, [tiny, 1.5 * tiny, tiny, 0.5 * tiny, 0, -0.0, np.finfo(dtype).smallest_subnormal])      # subnormal differences
    col(p["b"], 3, [-0.0, 0.0, -0.0, np.inf, np.inf, -np.inf, 1])
    if closure == "ri":
        for a in (p["u"], p["v"]):                                 # no shear around the columns 1..2: S2 = 0 with N2 of either sign
            a[Hz:Hz + Nz, Hy + 2:Hy + 4, Hx - 1:Hx + 3] = dtype(0.25)
        col(p["u"], 3, [np.inf] * Nz)                              # Inf - Inf in du
        col(p["v"], 2, [tiny, 2 * tiny, tiny, 0, tiny, 0.5 * tiny, 0])
    p = nan_where_not_read(p)
    want = R.reference(p, into)
    inner = want["kappa_c"][Hz + 1:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx]
    assert np.isfinite(inner).any() and (closure != "ri" or not prev or np.isnan(inner).any())
    got = _run(osg, gpu, p, into)
    for name in R.OUTPUTS:
        _assert_parent(got[name], want[name], name)


# ---- latitude bands ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closure", ["ca", "ri"])
@pytest.mark.parametrize("rows", [(8, 8, 8), (4, 5)], ids=["three-of-8", "Hy-beside-Hy+1"])
def test_latitude_bands_give_the_rows_of_the_global_call(osg, gpu, closure, rows):
    """through the C ABI: each band is the padded rows of the global arrays -- its seam halos hold what an exchange would deliver; the
    kernel has no fold index map, so the last band's row Ny + 1 is the global one"""
    Hy = 4
    size, halo = (20, sum(rows), 4), (4, Hy, 2)
    p, into = draw(closure, size, halo, F64, prev=True, counts=("cc", "fc", "cf"), nan_unread=False)
    whole = R.reference(p, into)
    got = _run(osg, gpu, p, into)
    for name in R.OUTPUTS:
        _assert_parent(got[name], whole[name], ("global", name))
    j0 = 0
    for band, ny in enumerate(rows):
        sl = slice(j0, j0 + ny + 2 * Hy)
        cut = lambda a: None if a is None else np.ascontiguousarray(a[:, sl])          # noqa: E731
        b = dict(p, size=(size[0], ny, size[2]), b=cut(p["b"]), u=cut(p["u"]), v=cut(p["v"]),
                 prev=None if p["prev"] is None else tuple(cut(a) for a in p["prev"]),
                 counts={k: np.ascontiguousarray(n[j0:j0 + ny]) for k, n in p["counts"].items()})
        got = _run(osg, gpu, b, {k: cut(a) for k, a in into.items()})
        for name in R.OUTPUTS:
            _assert_parent(got[name][:, Hy:Hy + ny], whole[name][:, Hy + j0:Hy + j0 + ny], (band, name))
        j0 += ny


# ---- the package ---------------------------------------------------------------------------------------------------------------------------------------------------
def _host_problem(osg, grid, closure, kind, b, u, v, prev, outputs, tdt):
    np_t = F64 if tdt == torch.float64 else F32
    host = lambda f: None if f is None else f.data.cpu().numpy()   # noqa: E731
    dz_f = osg.z_all_face_spacings(grid, tdt).numpy().astype(np_t)
    counts = {k: n.cpu().numpy() for k, n in grid.column_counts.items() if k in ("cc", "fc", "cf")}
    size, halo = (b.Nx, b.Ny, b.Nz), (b.Hx, b.Hy, b.Hz)
    if kind == "ca":
        params = dict(background_kappa=closure.background_kappa_z, convective_kappa=closure.convective_kappa_z, background_nu=closure.background_nu_z,
                      convective_nu=closure.convective_nu_z)
    else:
        params = {k: getattr(closure, k) for k in R.RI_PARAMS}
    return R.problem(kind, size, halo, host(b), dz_f, params, u=host(u) if kind == "ri" else None, v=host(v) if kind == "ri" else None, prev=prev,
                     counts=counts, mask_value=0.0, outputs=outputs)


@pytest.mark.parametrize("kind", ["ca", "ri", "ri-averaged"])
@pytest.mark.parametrize("size,halo,tdt", [((48, 40, 6), (5, 5, 5), torch.float64), ((50, 40, 4), (4, 4, 4), torch.float32)],
                         ids=["48x40x6-h5-f64", "50x40x4-h4-f32"])
def test_the_step_plan_equals_the_references_and_replays_in_a_graph(osg, gpu, size, halo, tdt, kind):
    """on a built immersed grid with its own spacings and counts: the diffusivities of mixed_implicit_step_plan are mixing_ref's, the
    stepped fields are vertical_diffusion_ref's with those diffusivities, the plan allocates nothing when called, and a captured graph
    replays the eager bits -- with the time average, two calls in a row, the second of which reads the first one's filled halos"""
    import vertical_diffusion_ref as V
    from gpu_harness import _grid
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    np_t = F64 if tdt == torch.float64 else F32
    grid = _grid(osg, size, halo, tdt, True)
    gen = torch.Generator(device=gpu).manual_seed(7)
    u, v, T, S = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid), osg.CenterField(grid)
    for f in (u, v, T, S):
        f.data.uniform_(-1, 1, generator=gen)
    osg.fill_halo_regions([u, v, T, S])
    start = [f.data.clone() for f in (u, v, T, S)]
    linear = osg.PiecewiseLinearRiDependentTapering()
    closure = {"ca": osg.ConvectiveAdjustmentVerticalDiffusivity(convective_kappa_z=1.5, convective_nu_z=2.5, background_kappa_z=0.015625, background_nu_z=0.03125),
               "ri": osg.RiBasedVerticalDiffusivity(Ri_dependent_tapering=linear, Cen=0, Cav=0),
               "ri-averaged": osg.RiBasedVerticalDiffusivity(Ri_dependent_tapering=linear, Cen=0)}[kind]
    dt, calls = 0.37, 2 if kind == "ri-averaged" else 1
    step = osg.mixed_implicit_step_plan(closure, u, v, {"T": T, "S": S}, T, dt, fill_halos=True)
    outputs = tuple(k for k in R.OUTPUTS if step.mixing.outputs[k] is not None)
    assert outputs == (R.OUTPUTS if kind != "ca" else ("kappa_c", "kappa_u", "kappa_v"))

    def run():
        for _ in range(calls):
            step()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(gpu)
    run()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(gpu) == before              # the plans allocate nothing when called
    eager = [f.data.cpu().numpy() for f in (u, v, T, S)]
    eager_kappa = {k: step.mixing.outputs[k].data.cpu().numpy() for k in outputs}
    # the references, call by call: the fields are stepped in place and their halos refilled, so the second call sees the first one's fields
    fields = [osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid), osg.CenterField(grid)]
    for f, t in zip(fields, start):
        f.data.copy_(t)
    dz_c = osg.z_center_spacings(grid, tdt).numpy().astype(np_t)
    dz_f = osg.z_all_face_spacings(grid, tdt).numpy().astype(np_t)
    faces = R.face_shape(size, halo)
    prev = (np.zeros(faces, np_t), np.zeros(faces, np_t)) if kind == "ri-averaged" else None
    for _ in range(calls):
        p = _host_problem(osg, grid, closure, kind[:2], fields[2], fields[0], fields[1], prev, outputs, tdt)
        kappa = R.reference(p, {k: np.zeros(faces, np_t) for k in outputs})      # the plan's fields start as zeros
        for f, key, loc in zip(fields, ("kappa_u", "kappa_v", "kappa_c", "kappa_c"), ("fc", "cf", "cc", "cc")):
            new = V.reference([f.data.cpu().numpy()], kappa[key], 2, dz_c, dz_f, np_t(dt), size, halo, counts=grid.column_counts[loc].cpu().numpy())[0]
            f.data.copy_(torch.from_numpy(new))
        osg.fill_halo_regions(fields)
        if prev is not None:                                       # the next call's previous values: this call's, with their halos filled
            held = [osg.ZFaceField(grid), osg.ZFaceField(grid)]
            for f, k in zip(held, ("kappa_c", "nu_c")):
                f.data.copy_(torch.from_numpy(kappa[k]))
            osg.fill_halo_regions(held)
            prev = tuple(f.data.cpu().numpy() for f in held)
    for k in outputs:                                              # the interior: the halos of kappa_c and nu_c were filled by the plan
        got, want = (a[:, Hy:Hy + Ny, Hx:Hx + Nx] for a in (eager_kappa[k], kappa[k]))
        _assert_parent(np.ascontiguousarray(got), np.ascontiguousarray(want), ("diffusivity", k))
    for f, got, what in zip(fields, eager, "uvTS"):
        _assert_parent(got, f.data.cpu().numpy(), ("stepped", what))
    # the same calls as one captured graph, from the same start
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            run()
    torch.cuda.current_stream().wait_stream(side)
    for f, t in zip((u, v, T, S), start):
        f.data.copy_(t)
    for f in step.mixing.outputs.values():
        if f is not None:
            f.data.zero_()
    for t in step.mixing.twins or ():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for f, want, what in zip((u, v, T, S), eager, "uvTS"):
        _assert_parent(f.data.cpu().numpy(), want, ("replay", what))
    for k in outputs:
        _assert_parent(step.mixing.outputs[k].data.cpu().numpy(), eager_kappa[k], ("replay", k))
    again = step.with_dt(2 * dt)
    assert again.dt == 2 * dt and again.mixing is step.mixing


def test_the_one_shot_form_on_a_bare_grid(osg, gpu):
    size, halo = (48, 40, 6), (4, 4, 4)
    grid = osg.TripolarGrid(osg.GPU(0), torch.float64, size=size, halo=halo, z=(-1, 0))
    gen = torch.Generator(device=gpu).manual_seed(11)
    b, u, v = osg.CenterField(grid), osg.XFaceField(grid), osg.YFaceField(grid)
    for f in (b, u, v):
        f.data.uniform_(-1, 1, generator=gen)
    osg.fill_halo_regions([b, u, v])
    closure = osg.RiBasedVerticalDiffusivity(Ri_dependent_tapering=osg.PiecewiseLinearRiDependentTapering(), Cen=0, Cav=0)
    out = osg.vertical_mixing_diffusivities(closure, b, u, v, kappa_c=None)
    assert sorted(out) == ["kappa_u", "kappa_v", "nu_c"]
    dz_f = osg.z_all_face_spacings(grid, torch.float64).numpy()
    p = R.problem("ri", size, halo, b.data.cpu().numpy(), dz_f, {k: getattr(closure, k) for k in R.RI_PARAMS}, u=u.data.cpu().numpy(),
                  v=v.data.cpu().numpy(), outputs=tuple(sorted(out)))
    want = R.reference(p, {k: np.zeros(R.face_shape(size, halo)) for k in out})
    for k in ("kappa_u", "kappa_v"):                               # only nu_c has its halos filled
        _assert_parent(out[k].data.cpu().numpy(), want[k], k)
    inner = (slice(None), slice(4, 44), slice(4, 52))
    _assert_parent(np.ascontiguousarray(out["nu_c"].data.cpu().numpy()[inner]), np.ascontiguousarray(want["nu_c"][inner]), "nu_c")
    filled = out["nu_c"].data.cpu().numpy()
    assert np.array_equal(filled[:, 4:44, :4], filled[:, 4:44, 48:52]) and np.array_equal(filled[:, 4:44, 52:], filled[:, 4:44, 4:8])      # periodic in x


def test_the_example_steps_agree_eagerly_and_as_a_graph():
    """examples/mixed_model_step.py asserts that its eager and replayed steps agree bit for bit"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "mixed_model_step.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# ---- past 2^31 elements -----------------------------------------------------------------------------------------------------------------------------------
def test_float32_past_2g_elements(osg, gpu):
    """8640 x 4320 x 64, halo 4, Float32: a parent of cells has 2 694 855 168 elements, offset 2^31 falls in padded plane 57 (cell 54, face
    54).  The Ri rule without the time average into kappa_c (with the count plane), kappa_u and kappa_v; data drawn on the device, the
    outputs sentinel-filled.
    a. every halo cell of the outputs still holds the sentinel, no interior cell of the planes of the faces 1..Nz+1 does, and the mask value
       and the diffusivity both reach the top faces;
    b. the same entry point on three plane windows -- contiguous plane slices of the SAME tensors, fresh small outputs, dz_f and the counts
       shifted -- equals the big output on the faces strictly inside the window (its own faces 1 and n + 1 are closed).  The bottom window
       lies below 2^30, the middle one holds the first interior cell at or past 2^31, the top one ends at the highest addresses.  The
       small-shape tests hold that form of the kernel to the reference;
    c. numpy anchor: the reference on a strip of 16 rows around the row that holds offset 2^31, all levels, equals the big output on the
       faces of the middle and the top window (NaNs by NaN-ness).
    Prints its wall time and peak device memory; skipped where the card holds less than twice the 70 GiB it needs."""
    import tendency_windows as tw
    from gpu_harness import BIG, BIG_HALO, TWO30, TWO31, _assert_only_the_interior_is_written, _big_counts, _bits_of, _budget, _cell_at, _random
    from orthogonalsphericalshellgrids.jl_amd import mixing as M
    from vorticity_ref import same_bits
    if torch.cuda.get_device_properties(gpu).total_memory < 140 * 2**30:
        pytest.skip("needs 70 GiB of device memory, under half the card")
    size, halo = BIG, BIG_HALO
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    sy, sx = Ny + 2 * Hy, Nx + 2 * Hx
    plane = sy * sx
    cells, faces = (Nz + 2 * Hz, sy, sx), (Nz + 1 + 2 * Hz, sy, sx)
    assert np.prod(cells, dtype=np.int64) == 2694855168 and TWO31 // plane == 57
    k31, j31, _ = _cell_at(TWO31, size, halo)
    assert k31 + 1 == 54
    windows = {"bottom": (1, 5), "middle": (52, 57), "top": (60, 64)}                  # cells a..b, 1-based
    compared = {"bottom": [2, 3, 4, 5], "middle": [53, 54, 55, 56, 57], "top": [61, 62, 63, 64]}       # faces a+1..b
    L = osg._lib
    lib = M.mixing_lib()
    q = [RI[k] for k in R.RI_PARAMS]
    NAMES = ("kappa_c", "kappa_u", "kappa_v")

    def call(b, u, v, outs, dz_f, counts, n):
        M.check_mixing(lib.tpg_ri_based_diffusivities(b.data_ptr(), u.data_ptr(), v.data_ptr(), None, None, outs[0].data_ptr(), None, outs[1].data_ptr(),
                                                      outs[2].data_ptr(), *q, dz_f.data_ptr(), counts.data_ptr(), None, None, MASK_VALUE, Nx, Ny, n, Hx, Hy, Hz,
                                                      L.TPG_F32, L.current_stream_ptr(gpu)))

    with _budget(gpu, "mixing diffusivities"):
        b, u, v = (_random(gpu, cells, 300 + n, -1.0, 1.0) for n in range(3))
        dz_f = _random(gpu, (Nz + 1,), 310, 0.5, 2.0)
        counts = _big_counts(gpu, size, 311)
        outs = [torch.full(faces, tw.SENTINEL, dtype=torch.float32, device=gpu) for _ in NAMES]
        call(b, u, v, outs, dz_f, counts, Nz)
        torch.cuda.synchronize()
        # a
        for o in outs:
            _assert_only_the_interior_is_written(o, (Nx, Ny, Nz + 1), halo)
        mv = _bits_of(MASK_VALUE, outs[0])
        top = tw._ints(outs[0])[Hz + Nz - 1, Hy:Hy + Ny, Hx:Hx + Nx]                     # the face Nz, the last evaluated one
        assert bool((top[:, :8] == mv).all()) and not bool((top[:, 8:] == mv).all())
        # b
        for which, (a, z) in windows.items():
            n = z - a + 1
            cut = [t[a - 1:a - 1 + n + 2 * Hz] for t in (b, u, v)]
            small = [torch.full((n + 1 + 2 * Hz, sy, sx), tw.SENTINEL, dtype=torch.float32, device=gpu) for _ in NAMES]
            assert all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (*cut, *small))
            assert cut[0].data_ptr() - b.data_ptr() == (a - 1) * plane * 4
            if which == "bottom":
                assert (z + 1 + 2 * Hz) * plane < TWO30
            if which == "top":
                assert (a - 1 + Hz) * plane > TWO31 and z == Nz    # every interior plane of the window lies past 2^31
            call(*cut, small, dz_f[a - 1:z + 1], (counts - (a - 1)).contiguous(), n)
            torch.cuda.synchronize()
            for k in compared[which]:
                assert a < k <= z
                for name, w_, o in zip(NAMES, small, outs):
                    assert tw.equal_bits(w_[Hz + k - a], o[Hz + k - 1]), (which, k, name)
            del cut, small
        # c
        lo = min(max(j31 - 8, 1), Ny - 17)
        assert lo <= j31 < lo + 16
        rows = slice(lo, lo + 16 + 2 * Hy)                          # the strip's padded rows: its y-halos are rows of the big interior
        host = lambda t: t[..., rows, :].contiguous().cpu().numpy()    # noqa: E731
        p = R.problem("ri", (Nx, 16, Nz), halo, host(b), dz_f.cpu().numpy(), RI, u=host(u), v=host(v), counts={"cc": counts[lo:lo + 16].cpu().numpy()},
                      mask_value=MASK_VALUE, outputs=NAMES)
        want = R.reference(p, {k: np.full((Nz + 1 + 2 * Hz, 16 + 2 * Hy, sx), tw.SENTINEL, F32) for k in NAMES})
        for k in compared["middle"] + compared["top"]:
            for name, o in zip(NAMES, outs):
                got = o[Hz + k - 1, Hy + lo:Hy + lo + 16, Hx:Hx + Nx].contiguous().cpu().numpy()
                bad = same_bits(got, np.ascontiguousarray(want[name][Hz + k - 1, Hy:Hy + 16, Hx:Hx + Nx]))
                assert bad == 0, (k, name, bad, "cells differ of", got.size)
        del b, u, v, outs, counts, p, want
