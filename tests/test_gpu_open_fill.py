"""GPU tests of the Open (impenetrable) south / bottom / top face write (tpg_fill_open_faces and HaloFillPlan's use of it): bit-exact on the
whole parent against the host sequence of tests/open_ref.py (C oracle + numpy) for v and w with every class the other sides admit, scalar and
tensor conditions, aligned and offset pointers, sentinels in every halo cell; the direct C call; a model's (u, v, w, T, S) at 3600 x 1800 x
75 through the plan; latitude bands through the loop-back transport; the production RCCL branch's marshalling; graph replay with a tensor
condition updated in place."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest
import torch

from bounded_ref import random_field
from open_ref import OPEN, library_sequence_open, open_faces
from value_gradient_ref import GRADIENT, VALUE

pytestmark = pytest.mark.gpu
SENTINEL = 12345.0
SOUTH, BOTTOM, TOP = 1, 2, 4


@pytest.fixture(autouse=True)
def _free_hbm():
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _dev(host, gpu, offset):
    """device copy of `host`, `offset` elements past an allocation (element-aligned, off the 16-B grid for offset 1)"""
    t = torch.empty(host.size + offset, dtype=torch.from_numpy(host.reshape(-1)[:1]).dtype, device=gpu)[offset:].view(host.shape)
    t.copy_(torch.from_numpy(host))
    return t


def _sentinel_halos(a, size, halo):
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    keep = a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx].copy()
    a[...] = SENTINEL
    a[Hz:Hz + Nz, Hy:Hy + Ny, Hx:Hx + Nx] = keep
    return a


def _side(osg, kind, rng, rows, sx, tensor, dtype, gpu, offset):
    """(BoundaryCondition, reference spec, tensor or None) of one side"""
    if kind is None:
        return None, None, None
    if kind == "flux":
        return osg.NoFluxBoundaryCondition(), "flux", None
    ctor, k = {"value": (osg.ValueBoundaryCondition, VALUE), "gradient": (osg.GradientBoundaryCondition, GRADIENT),
               "open": (osg.OpenBoundaryCondition, OPEN), "impenetrable": (osg.OpenBoundaryCondition, OPEN)}[kind]
    if kind == "impenetrable":
        return osg.ImpenetrableBoundaryCondition(), (OPEN, np.asarray(0, dtype=dtype)), None
    if not tensor:
        host = dtype(rng.uniform(-1, 1))
        return ctor(float(host)), (k, np.asarray(host, dtype=dtype)), None
    host = rng.uniform(-1, 1, (rows, sx)).astype(dtype)
    t = _dev(host, gpu, offset)
    return ctor(t), (k, host), t


def _make(osg, rng, grid, loc, kinds, sg, tensor, dtype, gpu, offset):
    """a field at loc = (xl, yl, zl) with sides `kinds` = (south, bottom, top) names and zipper sign sg: (field, specs, host data, tensors)"""
    (Nx, Ny, Nz), halo = grid.size, grid.halo_size
    Hx, Hy, Hz = halo
    xl, yl, zl = loc
    size = (Nx, Ny, Nz + zl)
    rows = {"south": Nz + zl, "bottom": Ny + 2 * Hy, "top": Ny + 2 * Hy}
    bcs, specs, keep = {}, {}, []
    for side, k in zip(("south", "bottom", "top"), kinds):
        bcs[side], specs[side], t = _side(osg, k, rng, rows[side], Nx + 2 * Hx, tensor, dtype, gpu, offset)
        keep.append(t)
    host = _sentinel_halos(random_field(rng, size, halo, dtype), size, halo)
    per = osg.PeriodicBoundaryCondition
    L = lambda b: osg.Face if b else osg.Center
    f = osg.Field((L(xl), L(yl), L(zl)), grid, data=_dev(host, gpu, offset),
                  boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), north=osg.ZipperBoundaryCondition(sg), **bcs))
    return f, specs, host, size, keep


@pytest.mark.parametrize("size,halo", [((48, 40, 3), (4, 4, 4)), ((48, 40, 3), (5, 5, 5)), ((48, 40, 3), (3, 2, 1)), ((48, 40, 6), (5, 5, 5))],
                         ids=["nz3-h444", "nz3-h555", "nz3-h321", "nz6-h555"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
def test_bit_exact_v_and_w_with_every_class_on_the_other_sides(osg, oracle, gpu, size, halo, dtype, offset):
    """48 x 40 x 3 (and x 6, where Nz >= Hz lets the no-flux mirror of a z side run at halo 5; with Nz < Hz that class is left out): v (south Open; {none, Flux, Value, Gradient} on bottom and on top) and w (bottom and / or top Open; every such class on
    south), signs +1 / -1, scalar / impenetrable / tensor conditions, and fields without an Open side between them -- 160 fields in ONE plan
    (two geometry groups, batches of 16 in each C call); every halo cell a sentinel beforehand; the whole parent is compared"""
    from orthogonalsphericalshellgrids.jl_amd.grids import boundary_z_spacings
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo)
    rng = np.random.default_rng(hash((size, halo, offset, np.dtype(dtype).str)) % 2**32)
    other = [None, "flux", "value", "gradient"]
    zother = other if size[2] >= halo[2] else [None, None, "value", "gradient"]      # tpg_fill_bounded_halos: a z mirror needs Nz >= Hz
    cases = []
    for n, (kb, kt, sg, tensor) in enumerate(itertools.product(zother, zother, (1, -1), (False, True))):
        cases.append(((0, 1, 0), ("impenetrable" if n % 5 == 0 else "open", kb, kt), sg, tensor))
        if n % 3 == 0:                                             # fields without an Open side between them (24 of them, with the w's below)
            cases.append(((n // 3 % 2, 0, 0), (None if n % 2 else "flux", kb, kt), sg, tensor))
    for n, (ks, (kb, kt), sg, tensor) in enumerate(itertools.product(other, [("open", "impenetrable"), ("open", None), (None, "open")], (1, -1),
                                                                     (False, True))):
        cases.append(((0, 0, 1), (ks, kb, kt), sg, tensor))
        if n % 4 == 0:
            cases.append(((0, 0, 1), (ks, None, None), sg, tensor))
    cases += [((1, 1, 0), (None, zother[1], "value"), 1, False)] * (160 - len(cases))
    assert len(cases) == 160
    fields = [(loc, kinds, sg, *_make(osg, rng, grid, loc, kinds, sg, tensor, dtype, gpu, offset)) for loc, kinds, sg, tensor in cases]
    plan = osg.halo_fill_plan([f for _, _, _, f, *_ in fields])
    opens = [c for _, calls, _ in plan._steps for c in calls if c[0].__name__ == "tpg_fill_open_faces"]
    assert len(plan._steps) == 2 and len(opens) == 2 and all(calls[0][0].__name__ == "tpg_fill_open_faces" for _, calls, _ in plan._steps)
    assert sorted(sum(1 for s in c[1][2] if s) for c in opens) == [48, 64]            # > TPG_MAX_FIELDS active fields per call: batch split
    plan()
    torch.cuda.synchronize()
    dy_row = grid.dy_cf[grid.Hy].cpu().numpy().astype(dtype)
    dz = tuple(dtype(d) for d in boundary_z_spacings(grid, tdt))
    for loc, kinds, sg, f, specs, host, fsize, _ in fields:
        want = library_sequence_open(oracle, host, loc[0], loc[1], sg, fsize, halo, specs["south"], specs["bottom"], specs["top"], dy_row, dz)
        assert np.array_equal(f.data.cpu().numpy(), want), (loc, kinds, sg)


@pytest.mark.parametrize("ft", ["f32", "f64"])
def test_direct_call_changes_only_the_documented_cells(osg, gpu, ft):
    """the C call alone on sentinel-filled parents: rows shorter than one chunk (Float32 rows of 2: 8-B chunks), rows of 6 and 10, offset
    pointers, no halo in y or z, one field with all three sides (the z sides own c[i, 1, 1] and c[i, 1, Nz]), scalar and array conditions,
    a field without a side in the middle of the table"""
    lib = osg._lib.lib()
    dtype, code = (np.float32, osg._lib.TPG_F32) if ft == "f32" else (np.float64, osg._lib.TPG_F64)
    for (size, halo), offset in itertools.product((((2, 6, 2), (0, 2, 1)), ((4, 6, 2), (1, 2, 2)), ((6, 5, 3), (2, 2, 0)), ((6, 5, 2), (2, 0, 1)),
                                                   ((16, 7, 4), (4, 3, 2)), ((8, 4, 1), (1, 1, 1))), (0, 1)):
        (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
        sx, sy = Nx + 2 * Hx, Ny + 2 * Hy
        rng = np.random.default_rng(11)
        cs = rng.uniform(-1, 1, (Nz, sx)).astype(dtype)
        cz = rng.uniform(-1, 1, (sy, sx)).astype(dtype)
        ts, tz = _dev(cs, gpu, offset), _dev(cz, gpu, offset)
        s3 = SOUTH | BOTTOM | TOP if Nz >= 2 else SOUTH | TOP
        table = [(SOUTH, (cs, None, None)), (0, (None, None, None)), (BOTTOM, (None, dtype(0.25), None)), (s3, (dtype(-0.5), cz, dtype(2)) if Nz >= 2
                 else (dtype(-0.5), None, cz)), (TOP, (None, None, cz)), (SOUTH, (dtype(0), None, None))]
        hosts = [np.full((Nz + 2 * Hz, sy, sx), SENTINEL, dtype=dtype) for _ in table]
        devs = [_dev(h, gpu, offset) for h in hosts]
        n = len(table)
        sides = (C.c_uint8 * n)(*[s for s, _ in table])
        values, conds = (C.c_double * (3 * n))(), (C.c_void_p * (3 * n))()
        for fi, (s, cond) in enumerate(table):
            for k, c in enumerate(cond):
                if isinstance(c, np.ndarray):
                    conds[3 * fi + k] = (ts if c is cs else tz).data_ptr()
                elif c is not None:
                    values[3 * fi + k] = float(c)
        osg._lib.check(lib.tpg_fill_open_faces(osg._lib.ptr_table(devs), n, sides, values, conds, *size, *halo, code,
                                               osg._lib.current_stream_ptr(gpu)))
        torch.cuda.synchronize()
        for fi, ((s, cond), host, dev) in enumerate(zip(table, hosts, devs)):
            want = open_faces(host.copy(), size, halo, *(c if s & bit else None for c, bit in zip(cond, (SOUTH, BOTTOM, TOP))))
            got = dev.cpu().numpy()
            assert np.array_equal(got, want), (size, halo, offset, fi)
            cells = (Nz if s & SOUTH else 0) + Ny * bool(s & BOTTOM) + Ny * bool(s & TOP) - bool(s & SOUTH) * (bool(s & BOTTOM) + bool(s & TOP))
            assert (got != SENTINEL).sum() == cells * sx, (size, halo, offset, fi)


def _model_fields(osg, grid, gpu, tdt, offset, v_south, w_bottom, w_top):
    nf, per = osg.NoFluxBoundaryCondition, osg.PeriodicBoundaryCondition
    Ce, Fa = osg.Center, osg.Face
    specs = [("u", (Fa, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf())), ("v", (Ce, Fa, Ce), dict(south=v_south, bottom=nf(), top=nf())),
             ("w", (Ce, Ce, Fa), dict(south=nf(), bottom=w_bottom, top=w_top)), ("T", (Ce, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf())),
             ("S", (Ce, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf()))]
    g = getattr(grid, "underlying_grid", grid)                     # a band grid: the local rows, as Field takes them
    (Nx, Ny, Nz), (Hx, Hy, Hz) = (g.Nx, g.Ny, g.Nz), (g.Hx, g.Hy, g.Hz)
    gen = torch.Generator(device=gpu).manual_seed(5)
    out = []
    for name, loc, sides in specs:
        shape = (Nz + (loc[2] is Fa) + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
        data = torch.empty(int(np.prod(shape)) + offset, dtype=tdt, device=gpu)[offset:].view(shape)
        data.uniform_(-1, 1, generator=gen)
        out.append((name, sides, osg.Field(loc, grid, data=data, name=name,
                                           boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **sides))))
    return out


@pytest.mark.parametrize("h,tdt,arrays", [(4, torch.float64, False), (5, torch.float64, True), (5, torch.float32, True), (4, torch.float32, False)],
                         ids=["halo4-f64-impenetrable", "halo5-f64-arrays", "halo5-f32-arrays-offset", "halo4-f32-impenetrable"])
def test_default_model_tuple_at_the_headline_size(osg, gpu, h, tdt, arrays):
    """(u, v, w, T, S) at 3600 x 1800 x 75 through halo_fill_plan: the whole parent of every field equals the same plan WITHOUT the Open
    sides run on a clone whose boundary faces were written beforehand with torch (whole padded rows, the rule of tests/open_ref.py).
    Float32 at halo 5: 3610-element rows and fields / conditions one element past their allocation (GEN)."""
    torch.cuda.reset_peak_memory_stats()
    size, halo = (3600, 1800, 75), (h, h, h)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    sx, sy = Nx + 2 * Hx, Ny + 2 * Hy
    offset = 1 if (tdt == torch.float32 and h == 5) else 0
    grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo)
    gen = torch.Generator(device=gpu).manual_seed(3)
    cond = lambda rows: torch.empty(rows * sx + offset, dtype=tdt, device=gpu)[offset:].view(rows, sx).uniform_(-1, 1, generator=gen)
    if arrays:
        vs, wb, wt = cond(Nz), cond(sy), 0.125
        sides = (osg.OpenBoundaryCondition(vs), osg.OpenBoundaryCondition(wb), osg.OpenBoundaryCondition(wt))
    else:
        vs = wb = wt = 0.0
        sides = (osg.ImpenetrableBoundaryCondition(),) * 3
    fs = _model_fields(osg, grid, gpu, tdt, offset, *sides)
    per = osg.PeriodicBoundaryCondition
    clones = []
    for name, s, f in fs:
        keep = {k: b for k, b in s.items() if not osg.is_open(b)}
        c = osg.Field(f.loc, grid, data=f.data.clone(), boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **keep))
        if name == "v":
            c.data[Hz:Hz + Nz, Hy] = vs
        if name == "w":
            c.data[Hz, Hy:Hy + Ny] = wb[Hy:Hy + Ny] if torch.is_tensor(wb) else wb
            c.data[Hz + Nz, Hy:Hy + Ny] = wt                                           # w has Nz + 1 levels: its top face is level Nz + 1
        clones.append(c)
    plan = osg.halo_fill_plan([f for *_, f in fs])
    assert [[c[0].__name__ for c in calls][0] for _, calls, _ in plan._steps] == ["tpg_fill_open_faces"] * 2
    plan()
    osg.halo_fill_plan(clones)()
    torch.cuda.synchronize()
    for (name, _, f), c in zip(fs, clones):
        assert torch.equal(f.data, c.data), name
    v, w = fs[1][2], fs[2][2]
    assert (v.data[Hz:Hz + Nz, Hy, Hx:Hx + Nx] == (vs[:, Hx:Hx + Nx] if arrays else 0)).all()
    assert (w.data[Hz + Nz, Hy:Hy + Ny - 1] == wt).all() and (w.data[Hz - 1, Hy:Hy + Ny - 1] != w.data[Hz, Hy:Hy + Ny - 1]).any()
    peak = torch.cuda.max_memory_allocated() / 2**30
    print(f"peak HBM of the default-model tuple at {size}, halo {h}, {tdt}: {peak:.1f} GiB (fields + clones)")
    assert peak < 96
    del fs, clones, plan, grid


@pytest.mark.parametrize("stage", [0, 2])
@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("halo", [(4, 4, 2), (5, 5, 5)], ids=["halo442", "halo5"])
def test_bands_with_loopback_transport(osg, gpu, R, stage, halo):
    """every rank's padded slab == the matching rows of the serially filled global field; the south wall is rank 0's only; bottom / top
    are written by every rank on its own rows, from its rows of the global condition arrays"""
    size = (48, 36, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    sx, sy = Nx + 2 * Hx, Ny + 2 * Hy
    rng = np.random.default_rng(29)
    O, imp, nf, V = osg.OpenBoundaryCondition, osg.ImpenetrableBoundaryCondition, osg.NoFluxBoundaryCondition, osg.ValueBoundaryCondition
    south_c = torch.from_numpy(rng.uniform(-1, 1, (Nz, sx))).to(gpu)
    top_g = torch.from_numpy(rng.uniform(-1, 1, (sy, sx))).to(gpu)
    bot_g = torch.from_numpy(rng.uniform(-1, 1, (sy, sx))).to(gpu)
    Ce, Fa = osg.Center, osg.Face

    def specs(top, bot):
        return [((Ce, Fa, Ce), dict(south=imp(), bottom=nf(), top=nf())), ((Ce, Fa, Ce), dict(south=O(south_c), bottom=nf(), top=V(top))),
                ((Ce, Fa, Ce), dict(south=O(0.75))), ((Ce, Ce, Fa), dict(south=nf(), bottom=imp(), top=imp())),
                ((Ce, Ce, Fa), dict(south=V(0.5), bottom=O(bot), top=O(top))), ((Ce, Ce, Fa), dict(top=O(-0.25))),
                ((Fa, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf())), ((Ce, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf()))]

    per = osg.PeriodicBoundaryCondition
    grid = osg.TripolarGrid(osg.GPU(0), torch.float64, size=size, halo=halo)
    shapes = [(Nz + (loc[2] is Fa) + 2 * Hz, sy, sx) for loc, _ in specs(top_g, bot_g)]
    globs = [torch.from_numpy(rng.uniform(-1, 1, s)).to(gpu) for s in shapes]
    serial = [osg.Field(loc, grid, data=g.clone(), boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **sides))
              for (loc, sides), g in zip(specs(top_g, bot_g), globs)]
    osg.halo_fill_plan(serial)()
    ranks = []
    for r in range(R):
        arch = osg.Distributed(osg.GPU(0), osg.Partition(y=R), local_rank=r)
        bg = osg.TripolarGrid(arch, torch.float64, size=size, halo=halo)
        jstart, jend = bg.jrange
        rows = slice(jstart - 1, jend + 2 * Hy)
        top_l, bot_l = top_g[rows].contiguous(), bot_g[rows].contiguous()
        fs = [osg.Field(loc, bg, data=g[:, rows].contiguous(), boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **sides))
              for (loc, sides), g in zip(specs(top_l, bot_l), globs)]
        assert [osg.is_open(f.boundary_conditions.south) for f in fs[:3]] == [r == 0] * 3
        ranks.append((bg, fs, top_l, bot_l))
    mailbox = osg.LoopbackMailbox()
    plans = [osg.halo_fill_plan(fs, exchange=mailbox.endpoint(r), fields_per_stage=stage) for r, (_, fs, *_) in enumerate(ranks)]
    for r, plan in enumerate(plans):
        first = []
        for (_, calls, pending), post in zip(plan._steps, plan._post):
            got = [c[0].__name__ for c in calls]
            assert pending is not None and "tpg_fill_open_faces" not in got[1:] + [c[0].__name__ for c in post]
            first.append(got[0] == "tpg_fill_open_faces")
        assert first == [r == 0, True]                             # the v group's wall is rank 0's; the w group's faces are every rank's
    for plan in plans:
        plan.begin()
    for plan in plans:
        plan.finish()
    torch.cuda.synchronize()
    for r, (bg, fs, *_) in enumerate(ranks):
        jstart, jend = bg.jrange
        for k, (f, s) in enumerate(zip(fs, serial)):
            assert torch.equal(f.data, s.data[:, jstart - 1:jend + 2 * Hy]), (r, k)


@pytest.mark.parametrize("pipelined", [False, True])
def test_rccl_branch_runs_the_open_call_before_the_one_call_fill(osg, gpu, monkeypatch, pipelined):
    """production branch (an RcclComm on the architecture): per plan call and geometry group, tpg_fill_open_faces, then the one distributed C
    call, then the no-flux mirror, all on the caller's stream; the distributed call is replaced by a recorder that runs the local fill
    (no second RCCL rank here)"""
    from orthogonalsphericalshellgrids.jl_amd.distributed import RcclComm
    lib = osg._lib.lib()
    size, halo, R = (32, 24, 4), (4, 4, 2), 3
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    order = []
    real_bounded, real_open = lib.tpg_fill_bounded_halos, lib.tpg_fill_open_faces

    def distributed(comm, rank, nranks, fields, nfields, xl, yl, sg, ss, sn, rs, rn, Nx, Ny, Nz, Hx, Hy, Hz, ft, stream, *pipe):
        order.append(("fill", Nz, stream.value))
        return lib.tpg_fill_halo_regions(fields, nfields, xl, yl, sg, Nx, Ny, Nz, Hx, Hy, Hz, 1 if rank == nranks - 1 else 0, ft, stream)

    def bounded(fields, nfields, sides, *rest):
        order.append(("bounded", rest[2], rest[-1].value))
        return real_bounded(fields, nfields, sides, *rest)

    def opened(fields, nfields, sides, values, conds, *rest):
        order.append(("open", rest[2], list(sides), rest[-1].value))
        return real_open(fields, nfields, sides, values, conds, *rest)

    name = "tpg_fill_halo_regions_distributed_pipelined" if pipelined else "tpg_fill_halo_regions_distributed"
    monkeypatch.setattr(lib, name, distributed, raising=True)
    monkeypatch.setattr(lib, "tpg_fill_bounded_halos", bounded, raising=True)
    monkeypatch.setattr(lib, "tpg_fill_open_faces", opened, raising=True)
    side = torch.cuda.Stream()
    for r in range(R):
        arch = osg.Distributed(osg.GPU(0), osg.Partition(y=R), local_rank=r, rccl_comm=RcclComm(C.c_void_p(0xC0FFEE), r, R))
        grid = osg.TripolarGrid(arch, torch.float64, size=size, halo=halo)
        fs = [f for *_, f in _model_fields(osg, grid, gpu, torch.float64, 0, osg.OpenBoundaryCondition(0.5), osg.ImpenetrableBoundaryCondition(),
                                           osg.OpenBoundaryCondition(-2.0))]
        plan = osg.halo_fill_plan(fs, fields_per_stage=1 if pipelined else 0)
        order.clear()
        with torch.cuda.stream(side):
            plan()
        torch.cuda.synchronize()
        s = side.cuda_stream
        want = ([("open", Nz, [0, SOUTH, 0, 0], s)] if r == 0 else []) + [("fill", Nz, s), ("bounded", Nz, s)] \
            + [("open", Nz + 1, [BOTTOM | TOP], s), ("fill", Nz + 1, s)] + ([("bounded", Nz + 1, s)] if r == 0 else [])
        assert order == want, r
        u, v, w, T, S = fs
        ny = w.Ny
        assert (w.data[Hz, Hy:Hy + ny - 1] == 0).all() and (w.data[Hz + Nz, Hy:Hy + ny - 1] == -2.0).all()      # ran on the device
        assert (v.data[Hz:Hz + Nz, Hy] == 0.5).all() == (r == 0)


def test_graph_replay_reads_tensor_conditions_at_replay(osg, oracle, gpu):
    """a captured serial plan of v (tensor south) and w (tensor top, scalar bottom): updating the tensors in place changes what a replay
    writes; every replay is bit-exact against the host sequence on the whole parent"""
    size, halo = (128, 48, 6), (5, 5, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    sx, sy = Nx + 2 * Hx, Ny + 2 * Hy
    grid = osg.TripolarGrid(osg.GPU(0), torch.float64, size=size, halo=halo)
    per, nf = osg.PeriodicBoundaryCondition, osg.NoFluxBoundaryCondition
    south = torch.rand(Nz, sx, dtype=torch.float64, device=gpu)
    top = torch.rand(sy, sx, dtype=torch.float64, device=gpu)
    v = osg.YFaceField(grid, boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), south=osg.OpenBoundaryCondition(south),
                                                                             bottom=nf(), top=nf()))
    w = osg.ZFaceField(grid, boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), south=nf(), top=osg.OpenBoundaryCondition(top),
                                                                             bottom=osg.OpenBoundaryCondition(0.5)))
    rng = np.random.default_rng(41)
    hv = _sentinel_halos(random_field(rng, size, halo, np.float64), size, halo)
    hw = _sentinel_halos(random_field(rng, (Nx, Ny, Nz + 1), halo, np.float64), (Nx, Ny, Nz + 1), halo)
    plan = osg.halo_fill_plan([v, w])
    graph = plan.graph()                     # graph() runs the plan once eagerly before it captures
    for step in range(2):
        south.copy_(torch.rand_like(south) + step)
        top.copy_(torch.rand_like(top) - step)
        v.data.copy_(torch.from_numpy(hv))
        w.data.copy_(torch.from_numpy(hw))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want_v = library_sequence_open(oracle, hv.copy(), 0, 1, -1, size, halo, (OPEN, south.cpu().numpy()), "flux", "flux", None, None)
        want_w = library_sequence_open(oracle, hw.copy(), 0, 0, 1, (Nx, Ny, Nz + 1), halo, "flux", (OPEN, np.float64(0.5)),
                                       (OPEN, top.cpu().numpy()), None, None)
        assert np.array_equal(v.data.cpu().numpy(), want_v), step
        assert np.array_equal(w.data.cpu().numpy(), want_w), step
