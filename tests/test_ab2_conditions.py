"""Host-side tests of the AB2 step (no GPU): the export list of libtripolar_hip_timestep.so, every argument error of tpg_ab2_step_velocities
and tpg_ab2_step_fields (status and message; every call below fails in validation, none reaches a launch, the pointers are fabricated and
never dereferenced), every refusal of the Python layer on host-only grid records, and with_dt."""
import ctypes as C

import pytest

from test_barotropic_conditions import _host_grid

NAMES = ["tpg_ab2_step_fields", "tpg_ab2_step_velocities", "tpg_timestep_last_error"]
G = (48, 40, 3, 4, 4, 4)                                           # Nx, Ny, Nz, Hx, Hy, Hz
HY2 = 13
PARENT = 56 * 48 * 11 * 8                                          # bytes of a Float64 parent
PLANE = 56 * (40 + 2 * HY2) * 8                                    # bytes of a Float64 2-D plane with Hy2 = 13
COUNTS = 48 * 40 * 4                                               # bytes of a count plane
BASE = 1 << 30
FAR = 1 << 40
ARGS = ("u", "v", "Gu_n", "Gv_n", "Gu_m", "Gv_m", "GU", "GV", "dz_c", "n_fc", "n_cf")
SIZES = dict(u=PARENT, v=PARENT, Gu_n=PARENT, Gv_n=PARENT, Gu_m=PARENT, Gv_m=PARENT, GU=PLANE, GV=PLANE, dz_c=3 * 8, n_fc=COUNTS, n_cf=COUNTS)
EULER, STORE = 1, 2


def _pointers():
    """11 fabricated pointers: six disjoint parents, two planes, the spacings, two count planes"""
    p = {name: BASE + q * PARENT for q, name in enumerate(ARGS[:8])}
    p.update(dz_c=1 << 20, n_fc=2 << 20, n_cf=3 << 20)
    return p


def _vel(lib, p, geom=G, Hy2=HY2, ft=1, flags=STORE, dt=0.5, chi=0.1):
    return lib.tpg_ab2_step_velocities(*(p[k] for k in ARGS), dt, chi, flags, *geom, Hy2, ft, None)


def test_header_exports_and_signatures_are_the_three_names(osg):
    from test_abi import declared_symbols, exported_symbols
    osg._lib.timestep_lib()
    assert declared_symbols("tripolar_hip_timestep.h") == NAMES == exported_symbols(osg._lib.TIMESTEP_LIB_PATH) == sorted(osg._lib.TIMESTEP_SIGNATURES)


def test_velocity_argument_errors_without_device_work(osg):
    lib = osg._lib.timestep_lib()
    err = lambda: lib.tpg_timestep_last_error().decode()
    good = _pointers()
    assert _vel(lib, good, ft=7) == -1 and err() == "unknown element type ft=7"
    assert _vel(lib, good, (49, 40, 3, 4, 4, 4)) == -2
    assert _vel(lib, good, Hy2=-1) == -1 and err() == "invalid north/south halo Hy2=-1 of the 2-D planes"
    for flags in (4, 8, 7, -1, 1 << 20):
        assert _vel(lib, good, flags=flags) == -1 and err().startswith("unknown flag bits 0x"), flags
    none = {k: None for k in ARGS}
    assert _vel(lib, {**none, "dz_c": good["dz_c"]}) == -1 and err() == "u, v, their tendencies, GU and GV all null: nothing to compute"
    for k in ("Gu_n", "Gv_m", "GU", "GV"):
        assert _vel(lib, {**none, k: good[k]}) == -1 and err() == "a tendency or a forcing plane given without its field: u and v both null", k
    # half-given groups
    u_only = {**good, **{k: None for k in ("v", "Gv_n", "Gv_m", "GV", "n_cf")}}
    v_only = {**good, **{k: None for k in ("u", "Gu_n", "Gu_m", "GU", "n_fc")}}
    for x, group, only in (("u", ("u", "Gu_n", "Gu_m", "GU"), v_only), ("v", ("v", "Gv_n", "Gv_m", "GV"), u_only)):
        assert _vel(lib, {**good, group[0]: None}) == -1 and err() == f"{x} and G{x}_n must be given together"
        assert _vel(lib, {**good, group[1]: None}) == -1 and err() == f"{x} and G{x}_n must be given together"
        for k in group[2:]:
            assert _vel(lib, {**only, k: good[k]}) == -1 and err().startswith(f"G{x}_m or G{x.upper()} given without {x}"), k
        for flags in (0, STORE, EULER | STORE):
            assert _vel(lib, {**good, group[2]: None}, flags=flags) == -1
            assert err() == f"null G{x}_m: it may be null only with TPG_AB2_EULER set and TPG_AB2_STORE_PREVIOUS clear", (x, flags)
    assert _vel(lib, {**good, "dz_c": None}) == -1 and err() == "null dz_c with GU or GV given"
    assert _vel(lib, {**good, "dz_c": None, "GU": None}) == -1 and err() == "null dz_c with GU or GV given"
    # alignment: every array to the element, the count planes to int32
    for name in ARGS[:9]:
        assert _vel(lib, {**good, name: good[name] + 4}) == -1 and err() == f"{name} pointer not aligned to its element type", name
        assert _vel(lib, {**good, name: good[name] + 2}, ft=0) == -1 and err() == f"{name} pointer not aligned to its element type", name
    for planes in ((2, 0), (0, 2), (1, 0), (0, 3)):
        p = {**good, "n_fc": good["n_fc"] + planes[0], "n_cf": good["n_cf"] + planes[1]}
        assert _vel(lib, p) == -1 and err() == "count plane pointer not aligned to int32", planes
    # every written array against every other array of the call, exact to one element: identical, one element inside from either side
    for flags, written in ((STORE, ("u", "v", "Gu_m", "Gv_m", "GU", "GV")), (0, ("u", "v", "GU", "GV"))):
        for out in written:
            for other in ARGS:
                if other == out:
                    continue
                for shift in (0, 8, SIZES[other] - 8, 8 - SIZES[out]):
                    p = {**good, other: FAR, out: FAR + shift}
                    assert _vel(lib, p, flags=flags) == -1 and " overlaps " in err(), (out, other, shift, err())
                    assert {err().split(" overlaps ")[0], err().split(" overlaps ")[1].split(" (")[0]} == {out, other}, (out, other, shift, err())
    assert _vel(lib, {**good, "Gu_m": good["Gu_n"]}) == -1 and err().startswith("Gu_m overlaps Gu_n")
    assert _vel(lib, {**good, "Gv_m": good["Gv_n"]}, flags=EULER | STORE) == -1 and err().startswith("Gv_m overlaps Gv_n")
    assert _vel(lib, {**good, "v": good["u"]}) == -1 and err().startswith("u overlaps v")
    # the no-overlap side: `out` ends where `other` starts, or starts where it ends, and the LAST pair the call checks, GV against n_cf,
    # overlaps (GV is placed over n_cf on the side away from the pair under test): that pair refuses, so every pair before it passed.
    # GV against n_cf itself has no later pair; GU against n_cf is the same code on the same sizes
    for out in ("u", "v", "Gu_m", "Gv_m", "GU", "GV"):
        for other in ARGS:
            if other == out or {out, other} == {"GV", "n_cf"}:
                continue
            for after in (True, False):
                p = {**good, other: FAR}
                p[out] = FAR + SIZES[other] if after else FAR - SIZES[out]
                if "GV" not in (out, other) and other != "n_cf":
                    p["GV"] = p["n_cf"] = FAR << 1
                elif other == "n_cf":
                    p["GV"] = p["n_cf"] + COUNTS - PLANE if after else p["n_cf"]
                else:
                    p["n_cf"] = p["GV"]
                assert _vel(lib, p) == -1 and err().startswith("GV overlaps n_cf"), (out, other, after, err())
                p[out] += -8 if after else 8                       # one element inside
                assert _vel(lib, p) == -1 and " overlaps " in err() and not err().startswith("GV overlaps n_cf"), (out, other, after, err())
    # read-only arrays may be one array; Gm is no written array without STORE, and is not looked at with EULER alone: shown by the last
    # check refusing, more work items than 32 bits index (reachable where the step has no integral and goes by segments of levels)
    big = (32768, 32768, 301, 0, 0, 0)                             # 2^29 chunks of two columns x several segments of levels
    spread = {k: (q + 1) << 44 for q, k in enumerate(ARGS)}
    spread.update(GU=None, GV=None, dz_c=None)
    assert _vel(lib, spread, big, Hy2=0) == -5 and err() == "ab2 velocity step: too many work items for 32-bit indexing"
    assert _vel(lib, {**spread, "Gv_n": spread["Gu_n"], "n_cf": spread["n_fc"]}, big, Hy2=0) == -5
    assert _vel(lib, {**spread, "Gu_m": spread["Gu_n"], "Gv_m": spread["Gv_n"]}, big, Hy2=0, flags=0) == -5
    assert _vel(lib, {**spread, "Gu_m": spread["Gu_n"], "Gv_m": spread["Gv_n"]}, big, Hy2=0, flags=STORE) == -1
    assert _vel(lib, {**spread, "Gu_m": None, "Gv_m": None}, big, Hy2=0, flags=EULER) == -5
    assert _vel(lib, {**spread, "Gu_m": spread["u"], "Gv_m": spread["v"]}, big, Hy2=0, flags=EULER) == -1 and err().startswith("u overlaps Gu_m")
    # one group alone
    for only in (u_only, v_only):
        p = {k: (None if only[k] is None else spread[k]) for k in ARGS}
        assert _vel(lib, p, big, Hy2=0) == -5 and "32-bit" in err()
    # with an integral an item walks all levels: the plane check every entry point shares refuses first
    assert _vel(lib, {k: (q + 1) << 44 for q, k in enumerate(ARGS)}, (65536, 32768, 1, 1, 1, 0), Hy2=0, ft=0) == -5 and "32-bit" in err()
    # Hy2 = 0 and no halo at all are shapes like any other
    assert _vel(lib, {**good, "v": good["u"]}, (48, 40, 3, 0, 0, 0), Hy2=0) == -1 and err().startswith("u overlaps v")


def _tables(n, fields=None, Gn=None, Gm=None):
    mk = lambda base, given: (C.c_void_p * n)(*(given if given is not None else [base + q * PARENT for q in range(n)]))
    return mk(BASE, fields), mk(BASE + 16 * PARENT, Gn), mk(BASE + 32 * PARENT, Gm)


def _fld(lib, tables, n, geom=G, ft=1, flags=STORE):
    return lib.tpg_ab2_step_fields(*tables, n, 0.5, 0.1, flags, *geom, ft, None)


def test_fields_argument_errors_without_device_work(osg):
    lib = osg._lib.timestep_lib()
    err = lambda: lib.tpg_timestep_last_error().decode()
    t3 = _tables(3)
    assert _fld(lib, t3, 3, ft=7) == -1 and err() == "unknown element type ft=7"
    assert _fld(lib, t3, 3, (49, 40, 3, 4, 4, 4)) == -2
    for flags in (4, 12, -2):
        assert _fld(lib, t3, 3, flags=flags) == -1 and err().startswith("unknown flag bits 0x"), flags
    assert _fld(lib, t3, 0) == -1 and err() == "no fields"
    assert _fld(lib, (None, t3[1], t3[2]), 3) == -1 and err() == "no fields"
    assert _fld(lib, (t3[0], None, t3[2]), 3) == -1 and err() == "no fields"
    assert _fld(lib, _tables(17), 17) == -1 and err() == "17 fields: at most TPG_MAX_FIELDS = 16 in one call"
    for flags in (0, STORE, EULER | STORE):
        assert _fld(lib, (t3[0], t3[1], None), 3, flags=flags) == -1
        assert err() == "null Gm table: it may be null only with TPG_AB2_EULER set and TPG_AB2_STORE_PREVIOUS clear"
    base = [BASE + q * PARENT for q in range(48)]
    for f in range(3):
        for q, msg in ((0, f"null field {f}"), (1, f"null Gn of field {f}"),
                       (2, f"null Gm of field {f}: it may be null only with TPG_AB2_EULER set and TPG_AB2_STORE_PREVIOUS clear")):
            rows = [base[0:3], base[16:19], base[32:35]]
            rows[q][f] = None
            assert _fld(lib, _tables(3, *rows), 3) == -1 and err() == msg, (f, q)
        names = (f"field {f}", f"Gn of field {f}", f"Gm of field {f}")
        for q in range(3):
            rows = [base[0:3], base[16:19], base[32:35]]
            rows[q][f] += 4
            assert _fld(lib, _tables(3, *rows), 3) == -1 and err() == f"{names[q]}: pointer not aligned to its element type", (f, q)
            rows[q][f] -= 2
            assert _fld(lib, _tables(3, *rows), 3, ft=0) == -1 and err() == f"{names[q]}: pointer not aligned to its element type", (f, q)
    # every written array against every other array of the call, by name, exact to one element; the no-overlap side by the later check
    big = (32768, 32768, 301, 0, 0, 0)                             # 2^29 chunks of two columns x several segments of levels
    bbytes = (1 << 30) * 301 * 8
    spread = [(q + 1) << 44 for q in range(9)]
    label = lambda q: ("field %d", "Gn of field %d", "Gm of field %d")[q // 3] % (q % 3)
    call = lambda a, geom, flags=STORE: _fld(lib, _tables(3, a[0:3], a[3:6], a[6:9]), 3, geom, flags=flags)
    assert call(spread, big) == -5 and err() == "ab2 field step: too many work items for 32-bit indexing"
    for flags, written in ((STORE, (0, 1, 2, 6, 7, 8)), (0, (0, 1, 2))):
        for out in written:
            for other in range(9):
                if other == out:
                    continue
                for shift in (0, 8, PARENT - 8, 8 - PARENT):
                    a = [BASE + q * PARENT for q in range(9)]
                    a[other], a[out] = FAR, FAR + shift
                    assert call(a, G, flags) == -1 and " overlaps " in err(), (out, other, shift)
                    assert {err().split(" overlaps ")[0], err().split(" overlaps ")[1].split(" (")[0]} == {label(out), label(other)}, err()
                for shift, overlaps in ((bbytes, False), (-bbytes, False), (bbytes - 8, True), (8 - bbytes, True)):
                    a = list(spread)
                    a[out] = a[other] + shift
                    assert call(a, big, flags) == (-1 if overlaps else -5), (out, other, shift, err())
    # tendencies may be shared where nothing writes them; without STORE Gm is read only
    a = list(spread)
    a[4] = a[3]
    a[7] = a[6]
    assert call(a, big, 0) == -5 and call(a, big, STORE) == -1 and err().startswith("Gm of field 0 overlaps Gm of field 1")
    a = list(spread)
    a[6] = a[3]
    assert call(a, big, 0) == -5 and call(a, big, STORE) == -1 and err().startswith("Gm of field 0 overlaps Gn of field 0")
    assert _fld(lib, (_tables(3, spread[0:3])[0], _tables(3, spread[3:6])[0], None), 3, big, flags=EULER) == -5
    # 16 fields are one call
    sixteen = [(q + 1) << 44 for q in range(48)]
    assert _fld(lib, _tables(16, sixteen[0:16], sixteen[16:32], sixteen[32:48]), 16, big) == -5 and "32-bit" in err()


def test_python_refusals(osg):
    import torch
    for name in ("ab2_step_velocities", "ab2_velocity_step_plan", "Ab2VelocityStepPlan", "ab2_step_fields", "ab2_step_plan", "Ab2StepPlan"):
        assert hasattr(osg, name), name
    for name in ("timestep_lib", "check_timestep", "TIMESTEP_SIGNATURES", "TIMESTEP_LIB_PATH"):
        assert hasattr(osg._lib, name), name
    grid, other, ext, ext2 = _host_grid(osg), _host_grid(osg), _host_grid(osg, Hy=3), _host_grid(osg, Hy=2)
    F, Cc = osg.Face, osg.Center
    new_u, new_v, new_c = (lambda g=grid, **kw: osg.XFaceField(g, **kw)), (lambda g=grid, **kw: osg.YFaceField(g, **kw)), \
        (lambda g=grid, **kw: osg.CenterField(g, **kw))
    u, Gu, Gup, v, Gv, Gvp = new_u(), new_u(), new_u(), new_v(), new_v(), new_v()
    GU, GV = osg.Field((F, Cc, None), ext), osg.Field((Cc, F, None), ext)
    six = dict(u=u, v=v, Gu=Gu, Gv=Gv, Gu_prev=Gup, Gv_prev=Gvp)
    order = ("u", "v", "Gu", "Gv", "Gu_prev", "Gv_prev")
    for fn in (osg.ab2_step_velocities, osg.ab2_velocity_step_plan):
        call = lambda kw=None, **more: fn(*({**six, **(kw or {})}[k] for k in order), 0.5, **more)
        shown = {"u": "Face, Center, Center", "v": "Center, Face, Center"}
        for name in order:
            x = "u" if "u" in name else "v"
            with pytest.raises(TypeError, match=rf"{name} must be a Field at \({shown[x]}\)"):
                call({name: new_c()})
            with pytest.raises(TypeError, match=rf"{name} must be a Field at \({shown[x]}\)"):
                call({name: new_v() if x == "u" else new_u()})
            with pytest.raises(TypeError, match=f"{name} must be a Field"):
                call({name: six[name].data})
            with pytest.raises(ValueError, match="one grid"):
                call({name: (new_u if x == "u" else new_v)(other)})
            with pytest.raises(NotImplementedError, match="z-windowed"):
                call({name: (new_u if x == "u" else new_v)(indices=(slice(None), slice(None), 2))})
            with pytest.raises(ValueError, match="one element type"):
                call({name: (new_u if x == "u" else new_v)(data=torch.zeros(u.data.shape, dtype=torch.float32))})
        # groups
        with pytest.raises(TypeError, match="at least one of u"):
            call({k: None for k in order})
        with pytest.raises(TypeError, match="GU needs u"):
            call({k: None for k in order}, GU=GU)
        with pytest.raises(TypeError, match="GU needs u"):
            call({"u": None, "Gu": None, "Gu_prev": None}, GU=GU)
        with pytest.raises(TypeError, match="GV needs v"):
            call({"v": None, "Gv": None, "Gv_prev": None}, GV=GV)
        for missing in (("u",), ("Gu",), ("u", "Gu_prev")):
            with pytest.raises(TypeError, match="u, Gu and Gu_prev are given together"):
                call({k: None for k in missing})
        with pytest.raises(TypeError, match="v, Gv and Gv_prev are given together"):
            call({"Gv": None})
        # the previous tendency: needed unless euler without store
        for kw in (dict(), dict(euler=True), dict(store_tendencies=False)):
            with pytest.raises(TypeError, match="Gu_prev is needed: store_tendencies writes it and euler=False reads it"):
                call({"Gu_prev": None}, **kw)
            with pytest.raises(TypeError, match="Gv_prev is needed"):
                call({"Gv_prev": None}, **kw)
        # aliases
        for name in ("Gu", "Gu_prev"):
            with pytest.raises(ValueError, match="a tendency of u is the field itself"):
                call({name: u})
            with pytest.raises(ValueError, match="a tendency of u is the field itself"):
                call({name: new_u(data=u.data)})
        with pytest.raises(ValueError, match="a tendency of v is the field itself"):
            call({"Gv": v})
        with pytest.raises(ValueError, match="Gu and Gu_prev are one field"):
            call({"Gu_prev": Gu})
        with pytest.raises(ValueError, match="Gv and Gv_prev are one field"):
            call({"Gv_prev": new_v(data=Gv.data)})
        # the 2-D planes: location, shared Nx / Ny / Hx, one Hy2, element type
        with pytest.raises(TypeError, match=r"GU must be a Field at \(Face, Center, Nothing\)"):
            call(GU=GV, GV=GV)
        with pytest.raises(TypeError, match=r"GV must be a Field at \(Center, Face, Nothing\)"):
            call(GU=GU, GV=v)
        with pytest.raises(TypeError, match="GU must be a Field"):
            call(GU=GU.data, GV=GV)
        with pytest.raises(ValueError, match="one north/south halo"):
            call(GU=GU, GV=osg.Field((Cc, F, None), ext2))
        with pytest.raises(ValueError, match="one element type"):
            call(GU=GU, GV=osg.Field((Cc, F, None), ext, data=torch.zeros(GV.data.shape, dtype=torch.float32)))
        wide = osg.OrthogonalSphericalShellGrid(
            architecture=None, Nx=8, Ny=6, Nz=3, Hx=2, Hy=3, Hz=1, Lz=1.0, arrays={"lambda_cc": torch.zeros(12, 12, dtype=torch.float64)},
            z_faces=torch.zeros(6), z_centers=torch.zeros(5), radius=1.0, conformal_mapping=osg.Tripolar(55, 70, -80),
            topology=(osg.PeriodicTopology, osg.RightConnected, osg.Bounded), dtype=torch.float64, z_spec=(-1, 0))
        with pytest.raises(ValueError, match="GU must share Nx, Ny and Hx"):
            call(GU=osg.Field((F, Cc, None), wide), GV=osg.Field((Cc, F, None), wide))
    # the fields call
    c, Gc, Gcp, d, Gd, Gdp = (new_c() for _ in range(6))
    for fn in (osg.ab2_step_fields, osg.ab2_step_plan):
        with pytest.raises(TypeError, match="no fields"):
            fn([], [], [], 0.5)
        with pytest.raises(TypeError, match="lists of one length"):
            fn([c, d], [Gc], [Gcp, Gdp], 0.5)
        with pytest.raises(TypeError, match="field 1 must be a Field"):
            fn([c, d.data], [Gc, Gd], [Gcp, Gdp], 0.5)
        with pytest.raises(TypeError, match=r"Gn of field 1 must be a Field at \(Center, Center, Center\)"):
            fn([c, d], [Gc, new_u()], [Gcp, Gdp], 0.5)
        with pytest.raises(TypeError, match=r"Gm of field 0 must be a Field at \(Center, Center, Center\)"):
            fn([c, d], [Gc, Gd], [None, Gdp], 0.5)
        with pytest.raises(TypeError, match="Gm is needed: store_tendencies writes it and euler=False reads it"):
            fn([c, d], [Gc, Gd], None, 0.5)
        with pytest.raises(TypeError, match="Gm is needed"):
            fn([c, d], [Gc, Gd], None, 0.5, euler=True)
        with pytest.raises(ValueError, match="one grid"):
            fn([c, new_c(other)], [Gc, new_c(other)], [Gcp, new_c(other)], 0.5)
        with pytest.raises(ValueError, match="one element type"):
            fn([c, d], [Gc, Gd], [Gcp, new_c(data=torch.zeros(c.data.shape, dtype=torch.float32))], 0.5)
        with pytest.raises(NotImplementedError, match="z-windowed"):
            w = lambda: new_c(indices=(slice(None), slice(None), range(1, 3)))
            fn([c, w()], [Gc, w()], [Gcp, w()], 0.5)
        with pytest.raises(ValueError, match="one location's geometry"):
            z = lambda: osg.ZFaceField(grid)
            fn([c, z()], [Gc, z()], [Gcp, z()], 0.5)
        with pytest.raises(ValueError, match="a tendency of field 1 is the field itself"):
            fn([c, d], [Gc, d], [Gcp, Gdp], 0.5)
        with pytest.raises(ValueError, match="Gn of field 0 and Gm of field 0 are one field"):
            fn([c, d], [Gc, Gd], [Gc, Gdp], 0.5)


def test_with_dt_changes_only_the_step_in_the_plans_arguments(osg):
    grid, ext = _host_grid(osg), _host_grid(osg, Hy=3)
    F, Cc = osg.Face, osg.Center
    u, Gu, Gup = (osg.XFaceField(grid) for _ in range(3))
    v, Gv, Gvp = (osg.YFaceField(grid) for _ in range(3))
    GU, GV = osg.Field((F, Cc, None), ext), osg.Field((Cc, F, None), ext)
    plan = osg.ab2_velocity_step_plan(u, v, Gu, Gv, Gup, Gvp, 0.5, chi=0.2, GU=GU, GV=GV)
    fn, args = plan._call
    ptrs = tuple(f.data.data_ptr() for f in (u, v, Gu, Gv, Gup, Gvp, GU, GV))
    assert args[:8] == ptrs and args[9:11] == (None, None) and args[11:] == (0.5, 0.2, 2, 8, 6, 3, 1, 1, 1, 3, osg._lib.TPG_F64)
    new = plan.with_dt(0.125)
    assert new is not plan and plan._call == (fn, args) and plan.dt == 0.5 and new.dt == 0.125 and new.chi == 0.2
    assert new._call[0] is fn and new._call[1] == args[:11] + (0.125,) + args[12:]
    assert new._held is plan._held and new.u is u and new.GU is GU
    # euler without store: the previous tendencies are not passed; no integral: no spacings, Hy2 = 0
    bare = osg.ab2_velocity_step_plan(u, None, Gu, None, Gup, None, 0.5, euler=True, store_tendencies=False)._call[1]
    assert bare[:11] == (ptrs[0], None, ptrs[2]) + (None,) * 8 and bare[11:] == (0.5, 0.1, 1, 8, 6, 3, 1, 1, 1, 0, osg._lib.TPG_F64)
    # the fields plan: 20 fields are two calls, both re-stepped
    c, Gc, Gcp = ([osg.CenterField(grid) for _ in range(20)] for _ in range(3))
    plan = osg.ab2_step_plan(c, Gc, Gcp, 0.5, store_tendencies=False)
    assert len(plan._before) == 1 and plan._before[0]._call[1][3:] == (16, 0.5, 0.1, 0, 8, 6, 3, 1, 1, 1, osg._lib.TPG_F64)
    assert plan._call[1][3:] == (4, 0.5, 0.1, 0, 8, 6, 3, 1, 1, 1, osg._lib.TPG_F64)
    assert [plan._before[0]._call[1][0][q] for q in range(16)] == [f.data.data_ptr() for f in c[:16]]
    assert [plan._call[1][2][q] for q in range(4)] == [f.data.data_ptr() for f in Gcp[16:]]
    new = plan.with_dt(2.0)
    for old, got in ((plan, new), (plan._before[0], new._before[0])):
        assert got is not old and got._call[0] is old._call[0] and old._call[1][4] == 0.5 and got._call[1][4] == 2.0
        assert got._call[1][:4] == old._call[1][:4] and got._call[1][5:] == old._call[1][5:]
    assert new.fields is plan.fields and osg.ab2_step_plan(c[:2], Gc[:2], None, 0.5, euler=True, store_tendencies=False)._call[1][2] is None
