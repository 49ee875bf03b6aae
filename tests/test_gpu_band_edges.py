"""Latitude-band halo fills at the halo-width edge, on the device: R ranks emulated in one process with the loop-back transport (real
kernels, the host protocol), uneven partitions and the default remainder rule, bands of exactly Hy and Hy + 1 rows.
  (a) edge-width chains equal the serial fill (oracle.fill_halo_regions on the global field);
  (b) every pass at once -- immersed mask, Open faces, fold, periodic x, seams, Value / Gradient, no-flux mirror -- on an edge-width chain of
      ImmersedBoundaryGrids equals the same plan on the serial immersed grid;
  (c) chains the protocol cannot fill are refused through the public names, on every rank, before anything is written or posted.
Whole padded slabs are compared as integers (bits); y halo rows hold a sentinel beforehand; the mailbox is drained afterwards.
The widths themselves are tests/test_band_width_conditions.py's subject (the rule against the emulated protocol, without a device)."""
import ctypes as C

import numpy as np
import pytest
import torch

from band_ref import SENTINEL, band_rows, band_slab
from immersed_ref import draw_columns, heights_of

pytestmark = pytest.mark.gpu
KEYS = ("cc", "fc", "cf", "ff")
SPECS = [(0, 0, 0, 1), (1, 0, 0, -1), (0, 1, 0, -1), (1, 1, 0, 1), (0, 0, 1, 1)]      # c, u, v, zeta at z-Center; one (Center, Center, Face) field
FACE_ONLY = [(0, 1, 0, -1), (1, 1, 0, 1)]                                              # v, zeta
# (halo, band widths or None = the default remainder rule on Ny = 40 over 3 ranks, fields)
LAYOUTS = [((4, 4, 2), (4, 4, 5), SPECS), ((4, 4, 2), (4, 5), SPECS), ((4, 4, 2), None, SPECS),
           ((5, 5, 5), (5, 5, 6), SPECS), ((5, 5, 5), (5, 6), SPECS), ((3, 2, 1), (2, 2, 3), SPECS),
           ((4, 4, 2), (5, 4), FACE_ONLY), ((5, 5, 5), (6, 5, 5), FACE_ONLY)]       # y-Face only: the last band at exactly Hy


def _ids(layout):
    halo, sizes, specs = layout
    return "h" + "".join(map(str, halo)) + "-" + ("default" if sizes is None else "x".join(map(str, sizes))) + ("-yface" if specs is FACE_ONLY else "")


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _loc(osg, xl, yl, zl):
    return tuple(osg.Face if b else osg.Center for b in (xl, yl, zl))


def _run(plans, mailbox):
    """phase 1 on every rank (local fill, pack, post), then phase 2 (delivery, unpack, post-passes); every posted message was delivered"""
    for plan in plans:
        plan.begin()
    for plan in plans:
        plan.finish()
    torch.cuda.synchronize()
    assert mailbox.box and all(not q for q in mailbox.box.values())


_truth = {}


def _serial_truth(oracle, halo, sizes, specs, Nx, Nz, dtype):
    """(unfilled global fields, their serial fills), computed once per geometry and shared by the cases that differ in the exchange form"""
    key = (halo, sizes, id(specs), Nx, np.dtype(dtype).str)
    if key not in _truth:
        (Hx, Hy, Hz), Ny = halo, sum(sizes)
        rng = np.random.default_rng([Nx, Ny, *halo, np.dtype(dtype).itemsize])
        globs, filled = [], []
        for xl, yl, zl, sg in specs:
            g = rng.uniform(-1, 1, (Nz + zl + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)).astype(dtype)
            g[:, :Hy] = SENTINEL
            g[:, Hy + Ny:] = SENTINEL
            globs.append(g)
            filled.append(oracle.fill_halo_regions(g.copy(), xl, yl, sg, (Nx, Ny, Nz + zl), halo))
        _truth[key] = (globs, filled)
    return _truth[key]


@pytest.mark.parametrize("stage", [0, 1], ids=["monolithic", "stages-of-1"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("Nx", [48, 50])                  # 50 with Float32: rows of 58 elements, the 8-B chunk forms
@pytest.mark.parametrize("layout", LAYOUTS, ids=_ids)
def test_edge_width_chains_equal_the_serial_fill(osg, oracle, gpu, layout, Nx, dtype, stage):
    halo, sizes, specs = layout
    (Hx, Hy, Hz), Nz = halo, 3
    tdt = torch.float64 if dtype == np.float64 else torch.float32
    partition = (lambda: osg.Partition(y=3)) if sizes is None else (lambda: osg.Partition(y=len(sizes), y_sizes=sizes))
    sizes = tuple(osg.local_sizes(40, 3)) if sizes is None else sizes
    assert layout[1] is not None or sizes == (13, 13, 14)
    R, Ny = len(sizes), sum(sizes)
    globs, filled = _serial_truth(oracle, halo, sizes, specs, Nx, Nz, dtype)
    mailbox = osg.LoopbackMailbox()
    ranks, plans = [], []
    for r in range(R):
        grid = osg.TripolarGrid(osg.Distributed(osg.GPU(0), partition(), local_rank=r), tdt, size=(Nx, Ny, Nz), halo=halo)
        assert grid.Ny == sizes[r] and grid.jrange == (sum(sizes[:r]) + 1, sum(sizes[:r + 1]))
        fs = []
        for (xl, yl, zl, sg), g in zip(specs, globs):
            f = osg.Field(_loc(osg, xl, yl, zl), grid)
            north = f.boundary_conditions.north
            assert osg.is_zipper(north) == (r == R - 1) and (r < R - 1 or north.condition == sg)
            f.data.copy_(torch.from_numpy(band_slab(g, sizes, r, Hy)))
            fs.append(f)
        plan = osg.halo_fill_plan(fs, exchange=mailbox.endpoint(r), fields_per_stage=stage)
        assert len(plan._steps) == len({zl for _, _, zl, _ in specs})              # the z-Face field is a geometry group with its own exchange
        ranks.append(fs)
        plans.append(plan)
    _run(plans, mailbox)
    for r, fs in enumerate(ranks):
        for f, want, spec in zip(fs, filled, specs):
            want = torch.from_numpy(np.ascontiguousarray(want[:, band_rows(sizes, r, Hy)]))
            assert torch.equal(_bits(f.data.cpu()), _bits(want)), (r, spec)


def _model_fields(osg, grid, globs):
    """the model tuple (u, v, w, T, S) with its default conditions and w's bottom Open with a value (as tests/test_gpu_immersed.py's), and
    one tracer with a Value south and a Gradient top condition; `globs`: the data of each, already this grid's rows"""
    nf, per, imp = osg.NoFluxBoundaryCondition, osg.PeriodicBoundaryCondition, osg.ImpenetrableBoundaryCondition
    Ce, Fa = osg.Center, osg.Face
    specs = [("u", (Fa, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf())), ("v", (Ce, Fa, Ce), dict(south=imp(), bottom=nf(), top=nf())),
             ("w", (Ce, Ce, Fa), dict(south=nf(), bottom=osg.OpenBoundaryCondition(0.5), top=imp())),
             ("T", (Ce, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf())), ("S", (Ce, Ce, Ce), dict(south=nf(), bottom=nf(), top=nf())),
             ("b", (Ce, Ce, Ce), dict(south=osg.ValueBoundaryCondition(0.5), bottom=nf(), top=osg.GradientBoundaryCondition(-0.25)))]
    return [osg.Field(loc, grid, name=name, data=g, boundary_conditions=osg.FieldBoundaryConditions(west=per(), east=per(), **sides))
            for (name, loc, sides), g in zip(specs, globs)]


_serial_model = {}


def _serial_model_truth(osg, gpu, halo, sizes, tdt):
    """the serial immersed grid, the (Ny, Nx) bottom it was built from, the unfilled global fields and the serial plan's result: once per
    geometry, left unchanged"""
    key = (halo, sizes, tdt)
    if key not in _serial_model:
        (Nx, Ny, Nz), (Hx, Hy, Hz) = (48, sum(sizes), 6), halo
        grid = osg.TripolarGrid(osg.GPU(0), tdt, size=(Nx, Ny, Nz), halo=halo, z=(-1, 0))
        zc = grid.z_centers[Hz:Hz + Nz].cpu().numpy()
        rng = np.random.default_rng([Ny, *halo, zc.dtype.itemsize])
        hin = torch.from_numpy(heights_of(draw_columns(rng, Nx, Ny, Nz), zc, rng)).to(gpu)
        serial = osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(hin))
        globs = []
        for zl in (0, 0, 1, 0, 0, 0):
            g = torch.from_numpy(rng.uniform(0.5, 1.5, (Nz + zl + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)).astype(zc.dtype)).to(gpu)
            g[:, :Hy] = SENTINEL
            g[:, Hy + Ny:] = SENTINEL
            globs.append(g)
        fields = _model_fields(osg, serial, [g.clone() for g in globs])
        osg.halo_fill_plan(fields, mask_immersed=0.0)()
        torch.cuda.synchronize()
        _serial_model[key] = (serial, hin, globs, fields)
    return _serial_model[key]


@pytest.mark.parametrize("stage", [0, 2], ids=["monolithic", "stages-of-2"])
@pytest.mark.parametrize("tdt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("halo,sizes", [((4, 4, 4), (5, 4, 5)), ((5, 5, 5), (6, 5, 6))], ids=["h444-5x4x5", "h555-6x5x6"])
def test_every_pass_at_once_on_an_edge_width_chain(osg, gpu, halo, sizes, tdt, stage):
    """rank 0 keeps one row more than the halo: its no-flux south mirror needs ny > Hy (tpg_fill_bounded_halos' own rule); the middle
    band owns exactly Hy rows, the zipper band Hy + 1"""
    (Hx, Hy, Hz), R = halo, len(sizes)
    serial, hin, globs, truth = _serial_model_truth(osg, gpu, halo, sizes, tdt)
    size = serial.underlying_grid.size
    mailbox = osg.LoopbackMailbox()
    bands = []
    for r in range(R):
        arch = osg.Distributed(osg.GPU(0), osg.Partition(y=R, y_sizes=sizes), local_rank=r)
        bg = osg.TripolarGrid(arch, tdt, size=size, halo=halo, z=(-1, 0))
        jstart, jend = bg.jrange
        assert bg.Ny == sizes[r]
        bands.append(osg.ImmersedBoundaryGrid(bg, osg.GridFittedBottom(hin[jstart - 1:jend]), exchange=mailbox.endpoint(r)))
    for ibg in bands:
        ibg.finish()
    torch.cuda.synchronize()
    assert all(not q for q in mailbox.box.values())
    hs = serial.immersed_boundary.bottom_height.data
    ranks, plans = [], []
    for r, ibg in enumerate(bands):
        rows = band_rows(sizes, r, Hy)
        assert torch.equal(_bits(ibg.immersed_boundary.bottom_height.data), _bits(hs[:, rows])), r
        for key in KEYS:
            assert torch.equal(ibg.column_counts[key], serial.column_counts[key][rows.start:rows.start + sizes[r]]), (r, key)
        slabs = []
        for g in globs:
            slab = g[:, rows].clone()
            slab[:, :Hy] = SENTINEL
            slab[:, Hy + sizes[r]:] = SENTINEL
            slabs.append(slab)
        fs = _model_fields(osg, ibg, slabs)
        plan = osg.halo_fill_plan(fs, exchange=mailbox.endpoint(r), mask_immersed=0.0, fields_per_stage=stage)
        # two geometry groups, the mask first in each (v's Open south face is rank 0's alone; w's Open bottom / top faces are every rank's)
        assert [calls[0][0].__name__ for _, calls, _ in plan._steps] == ["tpg_mask_immersed_fields"] * 2
        assert any(fn.__name__ == "tpg_fill_open_faces" for _, calls, _ in plan._steps for fn, *_ in calls)
        ranks.append(fs)
        plans.append(plan)
    _run(plans, mailbox)
    for r, fs in enumerate(ranks):
        rows = band_rows(sizes, r, Hy)
        for f, s in zip(fs, truth):
            assert torch.equal(_bits(f.data), _bits(s.data[:, rows])), (r, f.name)
    T = truth[3]
    assert bool((osg.interior(T)[0] == 0).any()) and bool((osg.interior(T)[0] != 0).any())     # the mask wrote, and not everywhere


REFUSED = [(5, 3, 5), (5, 5, 3), (3, 5, 5), (5, 5, 4)]            # at halo 4; the last one for its y-Center fields


@pytest.mark.parametrize("sizes", REFUSED, ids=lambda s: "x".join(map(str, s)))
def test_unfillable_chains_are_refused_through_the_public_names(osg, gpu, monkeypatch, sizes):
    """halo_fill_plan, fill_halo_regions and the ImmersedBoundaryGrid constructor raise the same ValueError on every rank -- with a
    loop-back transport and with an RcclComm on the architecture, where the distributed entry points fail the test if they are reached --
    while the grids themselves build; no field changes and nothing is posted"""
    from orthogonalsphericalshellgrids.jl_amd.distributed import RcclComm
    lib = osg._lib.lib()
    halo, R = (4, 4, 2), len(sizes)
    size = (48, sum(sizes), 3)
    for name in ("tpg_fill_halo_regions_distributed", "tpg_fill_halo_regions_distributed_peers", "tpg_fill_halo_regions_distributed_pipelined",
                 "tpg_fill_halo_regions_distributed_pipelined_peers", "tpg_halo_exchange_y", "tpg_halo_exchange_y_pipelined",
                 "tpg_pack_y_halo", "tpg_unpack_y_halo"):
        monkeypatch.setattr(lib, name, lambda *a, _n=name: pytest.fail(f"{_n} was called for a refused chain"), raising=True)
    mailbox = osg.LoopbackMailbox()
    gen = torch.Generator(device=gpu).manual_seed(5)
    texts, immersed_texts = [], []
    for r in range(R):
        for comm in (None, RcclComm(C.c_void_p(0xC0FFEE), r, R)):
            arch = osg.Distributed(osg.GPU(0), osg.Partition(y=R, y_sizes=sizes), local_rank=r, rccl_comm=comm)
            grid = osg.TripolarGrid(arch, torch.float64, size=size, halo=halo)                   # the grid build of such a layout succeeds
            assert grid.Ny == sizes[r]
            fs = [osg.CenterField(grid), osg.XFaceField(grid), osg.YFaceField(grid), osg.Field((osg.Face, osg.Face, osg.Center), grid)]
            for f in fs:
                f.data.uniform_(-1, 1, generator=gen)
            before = [f.data.clone() for f in fs]
            exchange = mailbox.endpoint(r) if comm is None else None
            for build in (lambda: osg.halo_fill_plan(fs, exchange=exchange), lambda: osg.fill_halo_regions(fs, exchange=exchange),
                          lambda: osg.halo_fill_plan(fs, exchange=exchange, fields_per_stage=2)):
                with pytest.raises(ValueError) as e:
                    build()
                texts.append(str(e.value))
            with pytest.raises(ValueError) as e:
                osg.ImmersedBoundaryGrid(grid, osg.GridFittedBottom(torch.zeros(grid.Ny, grid.Nx, dtype=torch.float64, device=gpu)),
                                         exchange=exchange)
            immersed_texts.append(str(e.value))
            torch.cuda.synchronize()
            for f, b in zip(fs, before):
                assert torch.equal(_bits(f.data), _bits(b)), (r, f.loc)
    assert not mailbox.box                                                                        # nothing was posted
    assert len(set(texts)) == 1 and len(set(immersed_texts)) == 1
    assert str(list(sizes)) in texts[0] and "Hy = 4" in texts[0]
    assert ("ny >= Hy + 1" in texts[0]) == (sizes == (5, 5, 4))


def test_the_c_entry_points_at_exactly_hy_rows(osg, oracle, gpu):
    """Ny == Hy seen from the C ABI.  A chain of ONE band is the serial fill with the reference's semantics (the y-Center fold reads the
    grid's own south halo row), through all four entry points.  The zipper band of a longer chain is refused for a y-Center field with
    nothing written; with y-Face fields alone it is not: the local fill runs and equals the serial fill of the band, and the call then
    stops at the communicator it was not given."""
    lib = osg._lib.lib()
    size, halo = (48, 4, 3), (4, 4, 2)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    rng = np.random.default_rng(44)
    stream = osg._lib.current_stream_ptr(gpu)
    none4 = (None,) * 4

    def fields(specs):
        hosts = [rng.uniform(-1, 1, (Nz + 2 * Hz, Ny + 2 * Hy, Nx + 2 * Hx)) for _ in specs]
        for h in hosts:
            h[:, :Hy] = SENTINEL
            h[:, Hy + Ny:] = SENTINEL
        devs = [torch.from_numpy(h).to(gpu) for h in hosts]
        tables = ((C.c_int8 * len(specs))(*[s[0] for s in specs]), (C.c_int8 * len(specs))(*[s[1] for s in specs]),
                  (C.c_int32 * len(specs))(*[s[2] for s in specs]))
        want = [oracle.fill_halo_regions(h.copy(), *s, size, halo) for h, s in zip(hosts, specs)]
        return hosts, devs, tables, want

    def same(devs, hosts):
        torch.cuda.synchronize()
        return all(np.array_equal(d.cpu().numpy().view(np.uint64), h.view(np.uint64)) for d, h in zip(devs, hosts))

    both = [(0, 0, 1), (1, 0, -1), (0, 1, -1), (1, 1, 1)]
    one_band = [lambda p, t: lib.tpg_fill_halo_regions_distributed_peers(None, -1, -1, 1, p, 4, *t, *none4, *size, *halo, 1, stream),
                lambda p, t: lib.tpg_fill_halo_regions_distributed(None, 0, 1, p, 4, *t, *none4, *size, *halo, 1, stream),
                lambda p, t: lib.tpg_fill_halo_regions_distributed_pipelined_peers(None, -1, -1, 1, p, 4, *t, *none4, *size, *halo, 1, stream, None, 1),
                lambda p, t: lib.tpg_fill_halo_regions_distributed_pipelined(None, 0, 1, p, 4, *t, *none4, *size, *halo, 1, stream, None, 1)]
    for call in one_band:
        hosts, devs, tables, want = fields(both)
        assert call(osg._lib.ptr_table(devs), tables) == 0
        assert same(devs, want)
    chain = [lambda p, n, t: lib.tpg_fill_halo_regions_distributed_peers(None, 0, -1, 1, p, n, *t, *none4, *size, *halo, 1, stream),
             lambda p, n, t: lib.tpg_fill_halo_regions_distributed_pipelined_peers(None, 0, -1, 1, p, n, *t, *none4, *size, *halo, 1, stream, None, 1)]
    for call in chain:
        hosts, devs, tables, _ = fields(both)
        assert call(osg._lib.ptr_table(devs), 4, tables) == -5
        assert b"Ny = 4" in lib.tpg_last_error() and b"Hy = 4" in lib.tpg_last_error()
        assert same(devs, hosts)                                                       # refused before any launch
        hosts, devs, tables, want = fields(both[2:])
        assert call(osg._lib.ptr_table(devs), 2, tables) == -1
        assert b"communicator" in lib.tpg_last_error()
        assert same(devs, want)
