"""The band widths a latitude-band fill is right for, without a GPU: distributed.check_band_widths against the one-process emulation of
the protocol (tests/band_ref.py: the oracle's passes + numpy seams, compared with rows of the serially filled global field) over every
layout near the halo-width edge; the default remainder rule; HaloFillPlan raising the same error on every rank before any collective or
C call; and the refusals of the four C entry points, which precede any launch (dummy pointers, never dereferenced)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from band_ref import LOCATIONS, band_fill, band_rows, default_sign, differing_cells, global_field, serial_fill


def accepted(osg, sizes, Hy, y_center):
    try:
        osg.check_band_widths(sizes, Hy, y_center)
    except ValueError:
        return False
    return True


def test_the_rule_is_tight_against_the_emulated_protocol(osg, oracle):
    """Hy in {2, 4, 5}, R in {2, 3}, every band width in 1 .. Hy + 2, the four horizontal locations (2896 cases; Nx = 12, halo (3, Hy, 1),
    Nz = 1, Float64, default signs).  Accepted => the emulated chain equals the serial fill bit for bit; refused => it differs, or rank 0
    is the only band thinner than the halo (right by the protocol -- nobody reads rank 0's south halo -- but refused by every fill's own
    geometry check, "halo larger than size").  Both classes occur and nothing falls outside them."""
    Nx, Nz, Hx, Hz = 12, 1, 3, 1
    rng = np.random.default_rng(2896)
    n_accepted = n_refused = n_rank0_only = cases = 0
    for Hy, R in itertools.product((2, 4, 5), (2, 3)):
        halo = (Hx, Hy, Hz)
        for sizes in itertools.product(range(1, Hy + 3), repeat=R):
            size = (Nx, sum(sizes), Nz)
            exact = {}
            for xl, yl in LOCATIONS:
                g = global_field(rng, size, halo)
                sg = default_sign(xl, yl)
                slabs = band_fill(oracle, g, sizes, xl, yl, sg, size, halo)
                exact[xl, yl] = differing_cells(slabs, serial_fill(oracle, g, xl, yl, sg, size, halo), sizes, Hy) == 0
            rank0_only = sizes[0] < Hy and all(n >= Hy for n in sizes[1:])
            for (xl, yl), ok in exact.items():
                cases += 1
                if accepted(osg, sizes, Hy, yl == 0):
                    n_accepted += 1
                    assert ok, ("accepted, but the protocol is wrong", sizes, Hy, (xl, yl))
                else:
                    n_refused += 1
                    n_rank0_only += ok
                    assert (not ok) or rank0_only, ("refused, but the protocol is right", sizes, Hy, (xl, yl))
            if accepted(osg, sizes, Hy, True):                     # a group with a y-Center field in it: all four locations
                assert all(exact.values()), (sizes, Hy)
            # the y-Face clause alone never accepts less than the y-Center one
            assert accepted(osg, sizes, Hy, False) or not accepted(osg, sizes, Hy, True)
    assert cases == 2896 and n_accepted > 0 and n_refused > 0 and n_accepted + n_refused == cases
    assert n_rank0_only == 320                                     # the refused-but-right cases: rank 0 the only thin band, nothing else


def test_a_chain_of_one_band_and_a_grid_without_y_halo_have_no_rule(osg):
    assert osg.check_band_widths([4], 4, True) is None and osg.check_band_widths([1], 4, True) is None
    assert osg.check_band_widths([1, 1, 1], 0, True) is None


def test_the_default_remainder_rule(osg):
    """the plain, reachable configuration: Ny = 32 over 8 ranks at Hy = 4 is eight bands of exactly Hy rows"""
    assert osg.local_sizes(32, 8) == [4] * 8
    assert not accepted(osg, osg.local_sizes(32, 8), 4, True)
    assert accepted(osg, osg.local_sizes(32, 8), 4, False)
    assert osg.local_sizes(40, 3) == [13, 13, 14]
    assert accepted(osg, osg.local_sizes(40, 3), 4, True) and accepted(osg, osg.local_sizes(40, 3), 5, True)
    assert osg.local_sizes(33, 8)[-1] == 5 and accepted(osg, osg.local_sizes(33, 8), 4, True)     # the last rank takes the remainder


@pytest.mark.parametrize("sizes,y_center,rank,rows,clause", [
    ((5, 3, 5), True, 1, 3, "ny >= Hy"), ((5, 3, 5), False, 1, 3, "ny >= Hy"), ((5, 5, 3), True, 2, 3, "ny >= Hy"),
    ((3, 5, 5), False, 0, 3, "ny >= Hy"), ((3, 2, 4), True, 0, 3, "ny >= Hy"), ((5, 5, 4), True, 2, 4, "ny >= Hy + 1"),
])
def test_the_message_names_rank_rows_halo_and_clause(osg, sizes, y_center, rank, rows, clause):
    with pytest.raises(ValueError) as e:
        osg.check_band_widths(sizes, 4, y_center)
    msg = str(e.value)
    assert f"rank {rank}" in msg and f"{rows} rows" in msg and "Hy = 4" in msg and clause in msg
    assert ("ny >= Hy + 1" in msg) == (clause == "ny >= Hy + 1")
    if clause == "ny >= Hy":
        return
    assert accepted(osg, sizes, 4, False)                          # the last-band clause is the y-Center fold's alone


def band_host_grid(osg, size, halo, arch):
    """a band grid whose (unused) arrays live in host memory, recording its global size as TripolarGrid does: enough for Field
    construction and for building a HaloFillPlan"""
    from orthogonalsphericalshellgrids.jl_amd.grids import (Bounded, FullyConnected, OrthogonalSphericalShellGrid, PeriodicTopology,
                                                             RightConnected, Tripolar)
    (Nx, Ny, Nz), (Hx, Hy, Hz) = size, halo
    jstart, jend = osg.local_row_range(Ny, arch)
    z = torch.zeros(1, dtype=torch.float64)
    return OrthogonalSphericalShellGrid(architecture=arch, Nx=Nx, Ny=jend - jstart + 1, Nz=Nz, Hx=Hx, Hy=Hy, Hz=Hz, Lz=1.0,
                                        arrays={"lambda_cc": z}, z_faces=z, z_centers=z, radius=1.0, conformal_mapping=Tripolar(55, 70, -80),
                                        topology=(PeriodicTopology, RightConnected if arch.local_rank == 0 else FullyConnected, Bounded),
                                        global_size=tuple(size), jrange=(jstart, jend))


@pytest.mark.parametrize("rccl", [False, True], ids=["host-driven", "rccl_comm"])
@pytest.mark.parametrize("sizes,face_only_ok", [((5, 3, 5), False), ((5, 5, 3), False), ((3, 5, 5), False), ((5, 5, 4), True)])
def test_every_rank_raises_the_same_error_at_plan_build(osg, monkeypatch, sizes, face_only_ok, rccl):
    """HaloFillPlan on every rank of the chain, from the widths of all ranks: one text, before the agreement collective and before the
    library is asked for anything (both are replaced by functions that fail the test), on the host-driven and on the rccl_comm path; a
    y-Face-only group passes the last-band clause"""
    from orthogonalsphericalshellgrids.jl_amd import fields as fields_module
    from orthogonalsphericalshellgrids.jl_amd.distributed import RcclComm
    halo, size = (4, 4, 2), (16, sum(sizes), 3)
    R = len(sizes)
    texts = []
    for r in range(R):
        comm = RcclComm(C.c_void_p(0xC0FFEE), r, R) if rccl else None
        arch = osg.Distributed(osg.GPU(), osg.Partition(y=R, y_sizes=sizes), local_rank=r, rccl_comm=comm)
        grid = band_host_grid(osg, size, halo, arch)
        assert grid.Ny == sizes[r]
        c, v, z = osg.CenterField(grid), osg.YFaceField(grid), osg.Field((osg.Face, osg.Face, osg.Center), grid)
        w = osg.ZFaceField(grid)                                   # a second geometry group, y-Center as well
        with monkeypatch.context() as m:
            m.setattr(fields_module, "_agree_across_ranks", lambda *a: pytest.fail("the agreement collective ran before the width check"))
            m.setattr(fields_module._lib, "lib", lambda: pytest.fail("the library was asked for before the width check"))
            for fs in ([c, v, z, w], [v, c], [w]):
                with pytest.raises(ValueError) as e:
                    osg.halo_fill_plan(fs, exchange=None if rccl else (lambda *a: None))
                texts.append(str(e.value))
            if not face_only_ok:
                with pytest.raises(ValueError):
                    osg.halo_fill_plan([v, z], exchange=None if rccl else (lambda *a: None))
        if face_only_ok:
            plan = osg.halo_fill_plan([v, z], exchange=None if rccl else (lambda *a: None))      # built, not run: host memory
            assert plan.is_distributed
    assert len(set(texts)) == 1 and f"{list(sizes)}" in texts[0]


def test_the_c_entry_points_refuse_the_thin_zipper_band_before_any_launch(osg):
    """all four distributed fill entry points: a zipper band with a south peer, Ny == Hy and a y-Center field is TPG_ERR_UNSUPPORTED with
    both numbers in the message; Ny == Hy - 1 stays the geometry check's refusal ("halo ... larger than size").  The pointers are never
    dereferenced and no communicator is looked at."""
    lib = osg._lib.lib()
    fields = (C.c_void_p * 2)(1 << 20, 2 << 20)
    xl, sg = (C.c_int8 * 2)(0, 1), (C.c_int32 * 2)(-1, 1)
    centre_last, face_only = (C.c_int8 * 2)(1, 0), (C.c_int8 * 2)(1, 1)
    bufs = (None, None, None, None)
    calls = {
        "peers": lambda yl, geom: lib.tpg_fill_halo_regions_distributed_peers(None, 0, -1, 1, fields, 2, xl, yl, sg, *bufs, *geom, 1, None),
        "ranks": lambda yl, geom: lib.tpg_fill_halo_regions_distributed(None, 2, 3, fields, 2, xl, yl, sg, *bufs, *geom, 1, None),
        "pipelined_peers": lambda yl, geom: lib.tpg_fill_halo_regions_distributed_pipelined_peers(None, 0, -1, 1, fields, 2, xl, yl, sg, *bufs,
                                                                                                   *geom, 1, None, None, 1),
        "pipelined_ranks": lambda yl, geom: lib.tpg_fill_halo_regions_distributed_pipelined(None, 2, 3, fields, 2, xl, yl, sg, *bufs,
                                                                                             *geom, 1, None, None, 1),
    }
    for name, call in calls.items():
        for Hy in (4, 5, 7):
            assert call(centre_last, (16, Hy, 3, 4, Hy, 2)) == -5, (name, Hy)
            msg = lib.tpg_last_error().decode()
            assert f"Ny = {Hy}" in msg and f"Hy = {Hy}" in msg and "y-Center" in msg and "field 1" in msg, (name, msg)
        for yl in (centre_last, face_only):
            assert call(yl, (16, 3, 3, 4, 4, 2)) == -5, name                  # Ny == Hy - 1: every fill's geometry check
            msg = lib.tpg_last_error().decode()
            assert "halo" in msg and "larger than size" in msg, (name, msg)
