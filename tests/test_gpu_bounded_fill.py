"""GPU tests of the no-flux south / bottom / top halo fill (tpg_fill_bounded_halos and HaloFillPlan's use of it): bit-exact against the
host sequence zipper -> south -> bottom / top -> periodic x (tests/bounded_ref.py, C oracle + numpy) at small and headline sizes, the
oracle-free mirror properties at config 5, latitude bands through the loop-back transport, the production RCCL branch's marshalling,
and graph capture."""
import ctypes as C
import gc
import itertools

import numpy as np
import pytest
import torch

from bounded_ref import BOTTOM, SOUTH, TOP, bounded_sequence, random_field

pytestmark = pytest.mark.gpu
LOCS = [(0, 0), (1, 0), (0, 1), (1, 1)]
SPECS = [(0, 0, 1), (1, 0, -1), (0, 1, -1), (1, 1, 1)]          # c, u, v, zeta: (xloc, yloc, default zipper sign)
MODEL_SIDES = [SOUTH | BOTTOM | TOP, SOUTH | BOTTOM | TOP, BOTTOM | TOP, BOTTOM | TOP]     # no south condition on the y-Face fields


@pytest.fixture(autouse=True)
def _free_hbm():
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _loc(osg, xl, yl):
    return (osg.Face if xl else osg.Center, osg.Face if yl else osg.Center, osg.Center)


def _bcs(osg, sides):
    nf, per = osg.NoFluxBoundaryCondition, osg.PeriodicBoundaryCondition
    return osg.FieldBoundaryConditions(west=per(), east=per(), south=nf() if sides & SOUTH else None,
                                       bottom=nf() if sides & BOTTOM else None, top=nf() if sides & TOP else None)


def _tensor(host, gpu, offset):
    """device copy of `host`, `offset` elements past an allocation (element-aligned, off the 16-B grid for offset 1)"""
    t = torch.empty(host.size + offset, dtype=torch.from_numpy(host[:1, :1, :1]).dtype, device=gpu)[offset:].view(host.shape)
    t.copy_(torch.from_numpy(host))
    return t


def _fill(osg, ts, specs, sides, size, halo, stream=None):
    lib, n = osg._lib.lib(), len(ts)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    ft = osg._lib.ft_of(ts[0].dtype)
    pt = osg._lib.ptr_table(ts)
    xl = (C.c_int8 * n)(*[s[0] for s in specs]); yl = (C.c_int8 * n)(*[s[1] for s in specs]); sg = (C.c_int32 * n)(*[s[2] for s in specs])
    osg._lib.check(lib.tpg_fill_halo_regions(pt, n, xl, yl, sg, Nx, Ny, Nz, Hx, Hy, Hz, 1, ft, stream))
    osg._lib.check(lib.tpg_fill_bounded_halos(pt, n, (C.c_uint8 * n)(*sides), Nx, Ny, Nz, Hx, Hy, Hz, ft, stream))


@pytest.mark.parametrize("halo", [(4, 4, 2), (5, 5, 3), (3, 2, 1), (2, 5, 3)], ids=["h442", "h553", "h321", "h253"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "offset"])
def test_bit_exact_every_location_sign_and_side(osg, oracle, gpu, halo, dtype, offset):
    """48 x 40 x 3: every (location, sign, sides) combination -- 4 x 2 x 8 = 64 fields in ONE call (four batches of 16)"""
    size = (48, 40, 3)
    rng = np.random.default_rng(101)
    combos = list(itertools.product(LOCS, (1, -1), range(8)))
    specs = [(xl, yl, sg) for (xl, yl), sg, _ in combos]
    sides = [s for _, _, s in combos]
    hosts = [random_field(rng, size, halo, dtype) for _ in combos]
    ts = [_tensor(h, gpu, offset) for h in hosts]
    _fill(osg, ts, specs, sides, size, halo)
    torch.cuda.synchronize()
    for t, h, (xl, yl, sg), s in zip(ts, hosts, specs, sides):
        bounded_sequence(oracle, h, xl, yl, sg, size, halo, s)
        assert np.array_equal(t.cpu().numpy(), h), (xl, yl, sg, s)


def test_rows_shorter_than_one_chunk_and_no_z_halo(osg, oracle, gpu):
    """Float32 rows of 2 elements (8-B chunks) and 6 elements; Hz = 0 makes bottom / top a no-op"""
    for size, halo in (((2, 6, 2), (0, 2, 1)), ((4, 6, 2), (1, 2, 2)), ((6, 5, 2), (2, 2, 0))):
        rng = np.random.default_rng(7)
        hosts = [random_field(rng, size, halo, np.float32) for _ in range(2)]
        ts = [_tensor(h, gpu, 1) for h in hosts]
        specs, sides = [(0, 0, 1), (1, 1, -1)], [7, 6]
        (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
        lib = osg._lib.lib()
        osg._lib.check(lib.tpg_fill_bounded_halos(osg._lib.ptr_table(ts), 2, (C.c_uint8 * 2)(*sides), Nx, Ny, Nz, Hx, Hy, Hz,
                                                  osg._lib.TPG_F32, None))
        torch.cuda.synchronize()
        from bounded_ref import south_mirror, z_mirror
        for t, h, s in zip(ts, hosts, sides):
            if s & SOUTH:
                south_mirror(h, size, halo)
            z_mirror(h, size, halo, bool(s & BOTTOM), bool(s & TOP))
            assert np.array_equal(t.cpu().numpy(), h), (size, halo, s)


@pytest.mark.parametrize("h", [4, 5])
@pytest.mark.parametrize("tdt", [torch.float64, torch.float32])
def test_headline_size_model_fields_through_the_plan(osg, oracle, gpu, h, tdt):
    """3600 x 1800 x 75, c / u / v / zeta with the model's no-flux sides, through Field + HaloFillPlan; at halo (5, 5, 5) a Float32
    row is 3610 elements (no 16-B rows) and the fields sit one element past their allocation"""
    size, halo = (3600, 1800, 75), (h, h, h)
    grid = osg.TripolarGrid(osg.GPU(0), tdt, size=size, halo=halo)
    offset = 1 if h == 5 else 0
    shape = (75 + 2 * h, 1800 + 2 * h, 3600 + 2 * h)
    fs, before = [], []
    for k, ((xl, yl, _), s) in enumerate(zip(SPECS, MODEL_SIDES)):
        data = torch.empty(int(np.prod(shape)) + offset, dtype=tdt, device=gpu)[offset:].view(shape)
        gen = torch.Generator(device=gpu).manual_seed(1000 + k)
        data.uniform_(-1, 1, generator=gen)
        fs.append(osg.Field(_loc(osg, xl, yl), grid, data=data, boundary_conditions=_bcs(osg, s)))
        before.append(data.clone())
    osg.halo_fill_plan(fs)()
    torch.cuda.synchronize()
    for f, b, (xl, yl, _), s in zip(fs, before, SPECS, MODEL_SIDES):
        sg = f.boundary_conditions.north.condition
        want = b.cpu().numpy()
        bounded_sequence(oracle, want, xl, yl, sg, size, halo, s)
        assert torch.equal(f.data, torch.from_numpy(want).to(gpu)), (xl, yl, s)
        del want
    del fs, before, grid


def test_config5_mirror_properties_without_an_oracle(osg, gpu, tlib):
    """8640 x 4320 x 100 at halo 5, one 33 GB Float64 field with south, bottom and top no-flux: the mirror identities, everything else as
    the plain horizontal fill of a copy, idempotence, and the peak of device memory under half the card"""
    size, halo = (8640, 4320, 100), (5, 5, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    torch.cuda.reset_peak_memory_stats(gpu)
    shape = (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)
    d = torch.empty(shape, dtype=torch.float64, device=gpu)
    assert tlib.tpg_fill_synthetic(d.data_ptr(), 0xB0B, 12345.0, *size, *halo, osg._lib.TPG_F64, None) == 0
    plain = d.clone()
    lib = osg._lib.lib()
    xl, yl, sg = (C.c_int8 * 1)(0), (C.c_int8 * 1)(0), (C.c_int32 * 1)(1)
    osg._lib.check(lib.tpg_fill_halo_regions(osg._lib.ptr_table([plain]), 1, xl, yl, sg, *size, *halo, 1, osg._lib.TPG_F64, None))
    _fill(osg, [d], [(0, 0, 1)], [SOUTH | BOTTOM | TOP], size, halo)
    torch.cuda.synchronize()
    for m in range(1, Hz + 1):
        assert torch.equal(d[Hz - m], d[Hz + m - 1]), m                     # plane 1-m == plane m
        assert torch.equal(d[Hz + Nz + m - 1], d[Hz + Nz - m]), m           # plane Nz+m == plane Nz+1-m
    for j in range(1, Hy + 1):
        assert torch.equal(d[:, Hy - j], d[:, Hy + j - 1]), j               # row 1-j == row j, every level (z halos included)
    assert torch.equal(d[Hz:Hz + Nz, Hy:], plain[Hz:Hz + Nz, Hy:])          # outside those halos: the plain fill
    assert not bool((d == 12345.0).any())                                   # no sentinel left in any halo
    del plain
    again = d.clone()
    _fill(osg, [d], [(0, 0, 1)], [SOUTH | BOTTOM | TOP], size, halo)
    torch.cuda.synchronize()
    assert torch.equal(d, again)                                            # idempotent
    peak = torch.cuda.max_memory_allocated(gpu)
    del d, again
    assert peak < torch.cuda.get_device_properties(gpu).total_memory / 2, peak


@pytest.mark.parametrize("stage", [0, 1, 3])
@pytest.mark.parametrize("R", [2, 4])
@pytest.mark.parametrize("halo", [(4, 4, 2), (5, 5, 5)], ids=["halo442", "halo5"])
def test_bands_with_loopback_transport(osg, oracle, gpu, R, stage, halo):
    """every rank's padded slab == the matching rows of the serially filled global field; only rank 0 mirrors its south side, every rank
    its bottom and top -- after the seam rows have arrived"""
    size = (48, 40, 5)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(23)
    globs = [random_field(rng, size, halo, np.float64) for _ in SPECS]
    ranks = []
    for r in range(R):
        arch = osg.Distributed(osg.GPU(0), osg.Partition(y=R), local_rank=r)
        grid = osg.TripolarGrid(arch, torch.float64, size=size, halo=halo)
        jstart, jend = grid.jrange
        fs = []
        for (xl, yl, _), s, g in zip(SPECS, MODEL_SIDES, globs):
            f = osg.Field(_loc(osg, xl, yl), grid, boundary_conditions=_bcs(osg, s))
            assert osg.is_flux(f.boundary_conditions.south) == bool(s & SOUTH and r == 0)
            slab = g[:, jstart - 1:jend + 2 * Hy].copy()
            f.data.copy_(torch.from_numpy(slab))
            fs.append(f)
        ranks.append((grid, fs))
    mailbox = osg.LoopbackMailbox()
    plans = [osg.halo_fill_plan(fs, exchange=mailbox.endpoint(r), fields_per_stage=stage) for r, (_, fs) in enumerate(ranks)]
    for plan in plans:
        plan.begin()
    for plan in plans:
        plan.finish()
    torch.cuda.synchronize()
    for (xl, yl, sg), s, g in zip(SPECS, MODEL_SIDES, globs):
        bounded_sequence(oracle, g, xl, yl, sg, size, halo, s)
    for r, (grid, fs) in enumerate(ranks):
        jstart, jend = grid.jrange
        for f, g in zip(fs, globs):
            assert np.array_equal(f.data.cpu().numpy(), g[:, jstart - 1:jend + 2 * Hy]), (r, f.loc)


@pytest.mark.parametrize("pipelined", [False, True])
def test_rccl_branch_appends_the_mirror_after_the_one_call_fill(osg, gpu, monkeypatch, pipelined):
    """production branch (an RcclComm on the architecture): per plan call, the one distributed C call and THEN tpg_fill_bounded_halos,
    both on the caller's stream; the distributed call is replaced by a recorder that runs the local fill (no second RCCL rank here)"""
    from orthogonalsphericalshellgrids.jl_amd.distributed import RcclComm
    lib = osg._lib.lib()
    size, halo, R = (32, 24, 4), (4, 4, 2), 3
    order = []
    real_bounded = lib.tpg_fill_bounded_halos

    def distributed(comm, rank, nranks, fields, nfields, xl, yl, sg, ss, sn, rs, rn, Nx, Ny, Nz, Hx, Hy, Hz, ft, stream, *pipe):
        order.append(("fill", rank, stream.value))
        return lib.tpg_fill_halo_regions(fields, nfields, xl, yl, sg, Nx, Ny, Nz, Hx, Hy, Hz, 1 if rank == nranks - 1 else 0, ft, stream)

    def bounded(fields, nfields, sides, Nx, Ny, Nz, Hx, Hy, Hz, ft, stream):
        order.append(("bounded", list(sides[:nfields]), stream.value))
        return real_bounded(fields, nfields, sides, Nx, Ny, Nz, Hx, Hy, Hz, ft, stream)

    name = "tpg_fill_halo_regions_distributed_pipelined" if pipelined else "tpg_fill_halo_regions_distributed"
    monkeypatch.setattr(lib, name, distributed, raising=True)
    monkeypatch.setattr(lib, "tpg_fill_bounded_halos", bounded, raising=True)
    side = torch.cuda.Stream()
    for r in range(R):
        arch = osg.Distributed(osg.GPU(0), osg.Partition(y=R), local_rank=r, rccl_comm=RcclComm(C.c_void_p(0xC0FFEE), r, R))
        grid = osg.TripolarGrid(arch, torch.float64, size=size, halo=halo)
        fs = [osg.Field(_loc(osg, xl, yl), grid, boundary_conditions=_bcs(osg, s)) for (xl, yl, _), s in zip(SPECS, MODEL_SIDES)]
        for f in fs:
            f.data.copy_(torch.rand_like(f.data))
        plan = osg.halo_fill_plan(fs, fields_per_stage=2 if pipelined else 0)
        order.clear()
        with torch.cuda.stream(side):
            plan()
        torch.cuda.synchronize()
        south = SOUTH if r == 0 else 0
        assert order == [("fill", r, side.cuda_stream), ("bounded", [south | BOTTOM | TOP] * 2 + [BOTTOM | TOP] * 2, side.cuda_stream)]
        Hz = halo[2]
        for f in fs:                                                         # the mirror ran on the device
            assert torch.equal(f.data[Hz - 1], f.data[Hz]) and torch.equal(f.data[Hz + size[2]], f.data[Hz + size[2] - 1])


def test_graph_capture_of_a_plan_with_bounded_fields(osg, gpu):
    """a captured serial plan with no-flux fields replays bit-identically to the eager fill"""
    grid = osg.TripolarGrid(osg.GPU(0), torch.float64, size=(128, 48, 6), halo=(5, 5, 5))
    fs = [osg.Field(_loc(osg, xl, yl), grid, boundary_conditions=_bcs(osg, s)) for (xl, yl, _), s in zip(SPECS, MODEL_SIDES)]
    for f in fs:
        f.data.copy_(torch.rand_like(f.data) * 2 - 1)
    pristine = [f.data.clone() for f in fs]
    plan = osg.halo_fill_plan(fs)
    plan()
    torch.cuda.synchronize()
    eager = [f.data.clone() for f in fs]
    for f, p in zip(fs, pristine):
        f.data.copy_(p)
    graph = plan.graph()                     # graph() runs the plan once eagerly before it captures
    for f, p in zip(fs, pristine):
        f.data.copy_(p)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    for f, e, p in zip(fs, eager, pristine):
        assert torch.equal(f.data, e) and not torch.equal(f.data, p)
