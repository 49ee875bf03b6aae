"""GPU tests of the Value / Gradient south / bottom / top halo fill (tpg_fill_value_gradient_halos and HaloFillPlan's use of it): bit-exact
against the host sequence of tests/value_gradient_ref.py (C oracle + numpy) for every valid combination of {none, Flux, Value, Gradient} per
side with scalar and tensor conditions, sentinels beyond the first halo point, the headline size through the plan, latitude bands through the
loop-back transport, the production RCCL branch's marshalling, and graph capture with a tensor condition updated in place."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest
import torch

from bounded_ref import random_field
from value_gradient_ref import GRADIENT, VALUE, extrapolate, post_pass_sequence

pytestmark = pytest.mark.gpu
LOCS = [(0, 0), (1, 0), (0, 1), (1, 1)]
SENTINEL = 12345.0


@pytest.fixture(autouse=True)
def _free_hbm():
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _loc(osg, xl, yl):
    return (osg.Face if xl else osg.Center, osg.Face if yl else osg.Center, osg.Center)


def _dev(host, gpu, offset):
    """device copy of `host`, `offset` elements past an allocation (element-aligned, off the 16-B grid for offset 1)"""
    t = torch.empty(host.size + offset, dtype=torch.from_numpy(host.reshape(-1)[:1]).dtype, device=gpu)[offset:].view(host.shape)
    t.copy_(torch.from_numpy(host))
    return t


def _side(osg, spec, gpu, offset):
    """(BoundaryCondition, reference spec, tensor or None) from a (kind name, host condition) pair"""
    if spec is None:
        return None, None, None
    kind, host = spec
    if kind == "flux":
        return osg.NoFluxBoundaryCondition(), "flux", None
    ctor = osg.ValueBoundaryCondition if kind == "value" else osg.GradientBoundaryCondition
    k = VALUE if kind == "value" else GRADIENT
    if np.ndim(host) == 0:
        return ctor(float(host)), (k, np.asarray(host, dtype=host.dtype)), None
    t = _dev(host, gpu, offset)
    return ctor(t), (k, host), t


def _make(osg, rng, grid, kinds, xl, yl, tensor, dtype, gpu, offset):
    """a field with sides `kinds` = (south, bottom, top) names, its reference specs and the host copy of its data"""
    size, halo = grid.size, grid.halo_size
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rows = {"south": Nz, "bottom": Ny + 2 * Hy, "top": Ny + 2 * Hy}
    specs, bcs, keep = {}, {}, []
    for side, k in zip(("south", "bottom", "top"), kinds):
        if k is None or k == "flux":
            spec = None if k is None else ("flux", None)
        else:
            host = rng.uniform(-1, 1, (rows[side], Nx + 2 * Hx)).astype(dtype) if tensor else dtype(rng.uniform(-1, 1))
            spec = (k, host)
        bcs[side], specs[side], t = _side(osg, spec, gpu, offset)
        keep.append(t)
    per = osg.PeriodicBoundaryCondition
    host = random_field(rng, size, halo, dtype)
    # sentinels beyond the first halo point: rows j <= -1 and planes k <= -1, k >= Nz+2
    host[:Hz - 1] = SENTINEL
    host[Hz + Nz + 1:] = SENTINEL
    host[:, :Hy - 1] = SENTINEL
    f = osg.Field(_loc(osg, xl, yl), grid, data=_dev(host, gpu, offset),
                  boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **bcs))
    return f, specs, host, keep


def _reference(oracle, xl, yl, f, specs, host, grid, dtype):
    from orthogonalsphericalshellgrids.jl_amd.grids import boundary_z_spacings
    sg = f.boundary_conditions.north.condition
    dy_row = grid.dy_cf[grid.Hy].cpu().numpy().astype(dtype)
    dz = boundary_z_spacings(grid, f.data.dtype)
    return post_pass_sequence(oracle, host, xl, yl, sg, grid.size, grid.halo_size, specs["south"], specs["bottom"], specs["top"],
                              dy_row, tuple(dtype(d) for d in dz))


@pytest.mark.parametrize("halo", [(4, 4, 2), (5, 5, 3), (3, 2, 1), (2, 5, 3)], ids=["h442", "h553", "h321", "h253"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
def test_bit_exact_every_location_and_side_combination(osg, oracle, gpu, halo, dtype, offset):
    """48 x 40 x 3: every location x every valid {none, Flux, Value, Gradient} per side, scalar and tensor conditions alternating --
    160 fields in ONE plan (one group: batches of 16 in each C call); sentinels beyond the first halo point stay unless a Flux mirror
    copies them"""
    size = (48, 40, 3)
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo)
    rng = np.random.default_rng(hash((halo, offset, np.dtype(dtype).str)) % 2**32)
    kinds = [None, "flux", "value", "gradient"]
    fields, n = [], 0
    for (xl, yl) in LOCS:
        for ks, kb, kt in itertools.product(kinds if yl == 0 else [None], kinds, kinds):
            fields.append((xl, yl, (ks, kb, kt), *_make(osg, rng, grid, (ks, kb, kt), xl, yl, n % 2 == 1, dtype, gpu, offset)))
            n += 1
    assert len(fields) == 160
    osg.halo_fill_plan([f for *_, f, _, _, _ in fields])()
    torch.cuda.synchronize()
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    for xl, yl, ks, f, specs, host, _ in fields:
        got = f.data.cpu().numpy()
        want = _reference(oracle, xl, yl, f, specs, host, grid, dtype)
        assert np.array_equal(got, want), (xl, yl, ks)
        if "flux" not in ks:
            assert (got[:Hz - 1] == SENTINEL).all() and (got[Hz + Nz + 1:] == SENTINEL).all()       # planes k <= -1, k >= Nz+2
            assert (got[Hz:Hz + Nz, :Hy - 1] == SENTINEL).all()                                       # rows j <= -1 of every level


def test_rows_shorter_than_one_chunk_and_no_halo_sides(osg, gpu):
    """Float32 rows of 2 elements (8-B chunks) and of 6, offset pointers; Hz = 0 / Hy = 0 make those sides no-ops"""
    lib = osg._lib.lib()
    for size, halo in (((2, 6, 2), (0, 2, 1)), ((4, 6, 2), (1, 2, 2)), ((6, 5, 2), (2, 2, 0)), ((6, 5, 2), (2, 0, 1))):
        (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
        sx, sy = Nx + 2 * Hx, Ny + 2 * Hy
        rng = np.random.default_rng(7)
        host = random_field(rng, size, halo, np.float32)
        cb = rng.uniform(-1, 1, (sy, sx)).astype(np.float32)
        cs = rng.uniform(-1, 1, (Nz, sx)).astype(np.float32)
        dy = rng.uniform(1, 2, (sy, sx)).astype(np.float32)
        t, tb, ts, tdy = _dev(host, gpu, 1), _dev(cb, gpu, 1), _dev(cs, gpu, 1), _dev(dy, gpu, 1)
        kinds = (C.c_uint8 * 3)(VALUE, GRADIENT, VALUE)
        vals = (C.c_double * 3)(0.0, 0.0, float(np.float32(0.3)))
        conds = (C.c_void_p * 3)(ts.data_ptr(), tb.data_ptr(), None)
        dz = (float(np.float32(0.7)), float(np.float32(1.3)))
        for pss in (osg._lib.TPG_SIDE_SOUTH, osg._lib.TPG_SIDE_BOTTOM | osg._lib.TPG_SIDE_TOP):
            osg._lib.check(lib.tpg_fill_value_gradient_halos(osg._lib.ptr_table([t]), 1, pss, kinds, vals, conds, tdy.data_ptr(), *dz,
                                                             *size, *halo, osg._lib.TPG_F32, None))
        torch.cuda.synchronize()
        from value_gradient_ref import south_vg, z_vg
        south_vg(host, size, halo, VALUE, cs, dy[Hy])
        z_vg(host, size, halo, (GRADIENT, cb), (VALUE, np.float32(0.3)), tuple(np.float32(d) for d in dz))
        assert np.array_equal(t.cpu().numpy(), host), (size, halo)


def _headline_fields(osg, grid, gpu, tdt, offset):
    """c, u, v, zeta, T, S at the headline size, with Value / Gradient sides that no Flux mirror reads (so that everything but the
    first halo points equals the same fill without them)"""
    Nx, Ny, Nz = grid.size
    Hx, Hy, Hz = grid.halo_size
    sx, sy = Nx + 2 * Hx, Ny + 2 * Hy
    V, G, nf = osg.ValueBoundaryCondition, osg.GradientBoundaryCondition, osg.NoFluxBoundaryCondition
    gen = torch.Generator(device=gpu).manual_seed(77)

    def cond(rows):
        t = torch.empty(rows * sx + offset, dtype=tdt, device=gpu)[offset:].view(rows, sx)
        return t.uniform_(-1, 1, generator=gen)

    C_, Fc = osg.Center, osg.Face
    specs = [("c", (C_, C_), dict(south=G(cond(Nz)), bottom=V(1.5), top=G(-2e-3))),
             ("u", (Fc, C_), dict(south=V(0.25))),
             ("v", (C_, Fc), dict(bottom=nf(), top=V(cond(sy)))),
             ("zeta", (Fc, Fc), dict(bottom=G(cond(sy)), top=nf())),
             ("T", (C_, C_), dict(bottom=G(1e-4), top=V(20.0))),
             ("S", (C_, C_), dict(south=nf(), bottom=nf(), top=V(cond(sy))))]
    per = osg.PeriodicBoundaryCondition
    shape = (Nz + 2 * Hz, sy, sx)
    out = []
    for k, (name, (LX, LY), sides) in enumerate(specs):
        data = torch.empty(int(np.prod(shape)) + offset, dtype=tdt, device=gpu)[offset:].view(shape)
        data.uniform_(-1, 1, generator=gen)
        out.append((name, data, sides, osg.Field((LX, LY, osg.Center), grid, data=data,
                                                 boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **sides))))
    return out


@pytest.mark.parametrize("tdt", [torch.float64, torch.float32])
def test_headline_size_through_the_plan(osg, gpu, tdt):
    """3600 x 1800 x 75 at halo (5, 5, 5): c / u / v / zeta / T / S through Field + HaloFillPlan.  The first halo points equal the host
    rule applied to the filled source rows / planes; every other cell equals the same fill of a device clone without the Value / Gradient
    sides.  Float32: 3610-element rows and fields one element past their allocation (GEN)."""
    from orthogonalsphericalshellgrids.jl_amd.grids import boundary_z_spacings
    size, halo = (3600, 1800, 75), (5, 5, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    offset = 1 if tdt == torch.float32 else 0
    dtype = np.float64 if tdt == torch.float64 else np.float32
    grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo)
    fs = _headline_fields(osg, grid, gpu, tdt, offset)
    per = osg.PeriodicBoundaryCondition
    clones = []
    for name, data, sides, f in fs:
        keep = {s: b for s, b in sides.items() if osg.is_flux(b)}
        clones.append(osg.Field(f.loc, grid, data=data.clone(), boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **keep)))
    osg.halo_fill_plan([f for *_, f in fs])()
    osg.halo_fill_plan(clones)()
    torch.cuda.synchronize()
    dy_row = grid.dy_cf[Hy].cpu().numpy()
    dz = boundary_z_spacings(grid, tdt)

    def host(c):
        return c if not torch.is_tensor(c) else c.cpu().numpy()

    for (name, data, sides, f), cl in zip(fs, clones):
        written = torch.zeros(data.shape, dtype=torch.bool, device=gpu)
        for side, bc in sides.items():
            if osg.is_flux(bc):
                continue
            kind = VALUE if osg.is_value(bc) else GRADIENT
            cond = host(bc.condition) if torch.is_tensor(bc.condition) else np.asarray(bc.condition, dtype=dtype)
            if side == "south":
                got, src, d = data[Hz:Hz + Nz, Hy - 1], data[Hz:Hz + Nz, Hy], dy_row[None, :]
                written[Hz:Hz + Nz, Hy - 1] = True
            elif side == "bottom":
                got, src, d = data[Hz - 1], data[Hz], dtype(dz[0])
                written[Hz - 1] = True
            else:
                got, src, d = data[Hz + Nz], data[Hz + Nz - 1], dtype(dz[1])
                written[Hz + Nz] = True
            want = extrapolate(kind, src.cpu().numpy(), cond, d, side == "top")
            assert np.array_equal(got.cpu().numpy(), want), (name, side)
        assert torch.equal(torch.where(written, cl.data, data), cl.data), name
        del written
    del fs, clones, grid


@pytest.mark.parametrize("stage", [0, 2])
@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("halo", [(4, 4, 2), (5, 5, 5)], ids=["halo442", "halo5"])
def test_bands_with_loopback_transport(osg, gpu, R, stage, halo):
    """every rank's padded slab == the matching rows of the serial fill; only rank 0 fills its south side; the bottom / top condition
    tensors are the band's rows of the global ones"""
    size = (48, 40, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    sx = Nx + 2 * Hx
    rng = np.random.default_rng(23)
    V, G, nf = osg.ValueBoundaryCondition, osg.GradientBoundaryCondition, osg.NoFluxBoundaryCondition
    top_g = torch.from_numpy(rng.uniform(-1, 1, (Ny + 2 * Hy, sx))).to(gpu)
    bot_g = torch.from_numpy(rng.uniform(-1, 1, (Ny + 2 * Hy, sx))).to(gpu)
    south_c = torch.from_numpy(rng.uniform(-1, 1, (Nz, sx))).to(gpu)
    locs = [(0, 0), (1, 0), (0, 1), (1, 1)]

    def sides(yl, top, bot):
        return [dict(south=G(south_c) if yl == 0 else None, bottom=V(bot), top=nf()),
                dict(south=V(0.5) if yl == 0 else None, bottom=nf(), top=G(top)),
                dict(south=nf() if yl == 0 else None, bottom=G(-1e-2), top=V(top))]

    per = osg.PeriodicBoundaryCondition
    specs = [(xl, yl, k) for xl, yl in locs for k in range(3)]
    grid = osg.TripolarGrid(osg.GPU(0), torch.float64, size=size, halo=halo)
    globs = [torch.from_numpy(random_field(rng, size, halo, np.float64)).to(gpu) for _ in specs]
    serial = [osg.Field(_loc(osg, xl, yl), grid, data=g.clone(),
                        boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **sides(yl, top_g, bot_g)[k]))
              for (xl, yl, k), g in zip(specs, globs)]
    osg.halo_fill_plan(serial)()
    ranks = []
    for r in range(R):
        arch = osg.Distributed(osg.GPU(0), osg.Partition(y=R), local_rank=r)
        bg = osg.TripolarGrid(arch, torch.float64, size=size, halo=halo)
        jstart, jend = bg.jrange
        rows = slice(jstart - 1, jend + 2 * Hy)
        top_l, bot_l = top_g[rows].contiguous(), bot_g[rows].contiguous()
        fs = []
        for (xl, yl, k), g in zip(specs, globs):
            f = osg.Field(_loc(osg, xl, yl), bg, data=g[:, rows].contiguous(),
                          boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **sides(yl, top_l, bot_l)[k]))
            assert (f.boundary_conditions.south is not None and not isinstance(f.boundary_conditions.south.classification,
                                                                              osg.boundary_conditions.HaloCommunication)) == (yl == 0 and r == 0)
            fs.append(f)
        ranks.append((bg, fs, top_l, bot_l))
    mailbox = osg.LoopbackMailbox()
    plans = [osg.halo_fill_plan(fs, exchange=mailbox.endpoint(r), fields_per_stage=stage) for r, (_, fs, *_) in enumerate(ranks)]
    for plan in plans:
        plan.begin()
    for plan in plans:
        plan.finish()
    torch.cuda.synchronize()
    for r, (bg, fs, *_) in enumerate(ranks):
        jstart, jend = bg.jrange
        for f, s, spec in zip(fs, serial, specs):
            assert torch.equal(f.data, s.data[:, jstart - 1:jend + 2 * Hy]), (r, spec)


@pytest.mark.parametrize("pipelined", [False, True])
def test_rccl_branch_runs_the_passes_after_the_one_call_fill(osg, gpu, monkeypatch, pipelined):
    """production branch (an RcclComm on the architecture): per plan call, the one distributed C call, then the Value / Gradient south
    pass (rank 0 only), the no-flux mirror and the bottom / top pass, all on the caller's stream; the distributed call is replaced by a
    recorder that runs the local fill (no second RCCL rank here)"""
    from orthogonalsphericalshellgrids.jl_amd.distributed import RcclComm
    lib = osg._lib.lib()
    size, halo, R = (32, 24, 4), (4, 4, 2), 3
    order = []
    real_bounded, real_vg = lib.tpg_fill_bounded_halos, lib.tpg_fill_value_gradient_halos

    def distributed(comm, rank, nranks, fields, nfields, xl, yl, sg, ss, sn, rs, rn, Nx, Ny, Nz, Hx, Hy, Hz, ft, stream, *pipe):
        order.append(("fill", stream.value))
        return lib.tpg_fill_halo_regions(fields, nfields, xl, yl, sg, Nx, Ny, Nz, Hx, Hy, Hz, 1 if rank == nranks - 1 else 0, ft, stream)

    def bounded(fields, nfields, sides, *rest):
        order.append(("bounded", rest[-1].value))
        return real_bounded(fields, nfields, sides, *rest)

    def vg(fields, nfields, pss, *rest):
        order.append(("vg", pss, rest[-1].value))
        return real_vg(fields, nfields, pss, *rest)

    name = "tpg_fill_halo_regions_distributed_pipelined" if pipelined else "tpg_fill_halo_regions_distributed"
    monkeypatch.setattr(lib, name, distributed, raising=True)
    monkeypatch.setattr(lib, "tpg_fill_bounded_halos", bounded, raising=True)
    monkeypatch.setattr(lib, "tpg_fill_value_gradient_halos", vg, raising=True)
    side = torch.cuda.Stream()
    per = osg.PeriodicBoundaryCondition
    for r in range(R):
        arch = osg.Distributed(osg.GPU(0), osg.Partition(y=R), local_rank=r, rccl_comm=RcclComm(C.c_void_p(0xC0FFEE), r, R))
        grid = osg.TripolarGrid(arch, torch.float64, size=size, halo=halo)
        fs = [osg.CenterField(grid, boundary_conditions=osg.FieldBoundaryConditions(
                  west=per(), east=per(), south=osg.GradientBoundaryCondition(0.1), bottom=osg.NoFluxBoundaryCondition(),
                  top=osg.ValueBoundaryCondition(3.0))),
              osg.YFaceField(grid, boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(),
                                                                                   bottom=osg.GradientBoundaryCondition(1.0)))]
        for f in fs:
            f.data.copy_(torch.rand_like(f.data))
        plan = osg.halo_fill_plan(fs, fields_per_stage=1 if pipelined else 0)
        order.clear()
        with torch.cuda.stream(side):
            plan()
        torch.cuda.synchronize()
        s = side.cuda_stream
        want = [("fill", s)] + ([("vg", 1, s)] if r == 0 else []) + [("bounded", s), ("vg", 6, s)]
        assert order == want, r
        Hz = halo[2]
        d = fs[1].data
        from orthogonalsphericalshellgrids.jl_amd.grids import boundary_z_spacings
        dzb, _ = boundary_z_spacings(grid)
        assert torch.equal(d[Hz - 1], d[Hz] + 1.0 * (-dzb))                         # the bottom pass ran on the device


def test_graph_capture_reads_tensor_conditions_at_replay(osg, gpu):
    """a captured serial plan with a tensor top condition: updating the tensor in place changes what a replay writes"""
    from orthogonalsphericalshellgrids.jl_amd.grids import boundary_z_spacings
    size, halo = (128, 48, 6), (5, 5, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    grid = osg.TripolarGrid(osg.GPU(0), torch.float64, size=size, halo=halo)
    per = osg.PeriodicBoundaryCondition
    top = torch.rand(Ny + 2 * Hy, Nx + 2 * Hx, dtype=torch.float64, device=gpu)
    south = torch.rand(Nz, Nx + 2 * Hx, dtype=torch.float64, device=gpu)
    c = osg.CenterField(grid, boundary_conditions=osg.FieldBoundaryConditions(
        west=per(), east=per(), south=osg.GradientBoundaryCondition(south), bottom=osg.NoFluxBoundaryCondition(),
        top=osg.ValueBoundaryCondition(top)))
    c.data.copy_(torch.rand_like(c.data) * 2 - 1)
    pristine = c.data.clone()
    plan = osg.halo_fill_plan([c])
    graph = plan.graph()                     # graph() runs the plan once eagerly before it captures
    dz = boundary_z_spacings(grid)[1]
    dy = grid.dy_cf[Hy]
    for step in range(2):
        top.copy_(torch.rand_like(top) + step)
        south.copy_(torch.rand_like(south) - step)
        c.data.copy_(pristine)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got_top = c.data[Hz + Nz].cpu().numpy()
        want_top = extrapolate(VALUE, c.data[Hz + Nz - 1].cpu().numpy(), top.cpu().numpy(), np.float64(dz), True)
        assert np.array_equal(got_top, want_top), step
        got_s = c.data[Hz:Hz + Nz, Hy - 1].cpu().numpy()
        want_s = extrapolate(GRADIENT, c.data[Hz:Hz + Nz, Hy].cpu().numpy(), south.cpu().numpy(), dy.cpu().numpy()[None, :], False)
        assert np.array_equal(got_s, want_s), step
