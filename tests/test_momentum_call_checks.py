"""The enstrophy-conserving, the WENO5 and the all-upwinded momentum tendency answer a bad call alike (no GPU): one table of fabricated calls,
one per check the three entry points have in common, goes through tpg_momentum_advection_tendency (scheme = 0),
tpg_weno_momentum_advection_tendency and tpg_weno_vi_momentum_advection_tendency, and status and full message must be equal -- but for the
name of the spacing table, which the third call takes at the centres (dz_c for dz_f).  Only the halo refusal may differ otherwise, and only
in the stencil it names and the halo that stencil needs.  Every call fails in validation, none reaches a launch; the pointers are never
dereferenced.  The three Python plans are one body (_MomentumTendencyPlan): their refusals on host-only grid records differ in the `what`
prefix alone."""
import pytest

from test_weno_momentum_conditions import _grid

GEOM = (48, 40, 3, 4, 4, 4)                                        # Nx, Ny, Nz, Hx, Hy, Hz
PLANE = 56 * 48 * 8
PARENT, WPARENT = PLANE * 11, PLANE * 12                           # bytes of a Float64 parent of u, v, Gu, Gv (Nz + 2Hz planes) and of w (one more)
BASE, FAR = 1 << 30, 1 << 40
METRICS = ("dx_fc", "dy_fc", "az_fc", "dx_cf", "dy_cf", "az_cf", "az_cc", "az_ff", "dz_f")
AT = dict(u=BASE, v=BASE + PARENT, w=BASE + 2 * PARENT, Gu=FAR, Gv=FAR + 3 * PARENT, **{name: (q + 1) << 20 for q, name in enumerate(METRICS)})
NFC, NCF = 20 << 20, 21 << 20
AWAY = dict(u=3 * FAR, v=4 * FAR, w=5 * FAR)                       # the inputs out of the way of an output laid over one of them at BASE
F32, F64 = 0, 1
CENTRED_HALO = "the rule reads u, v[i-1..i+1, j-1..j+1, k-1..k+1] and w[i-1, j], w[i, j-1]: Hx >= 1, Hy >= 1 and Hz >= 1 needed (halo ({},{},{}))"
WENO_HALO = ("the rule reads Z[i, j-2..j+3] and Z[i-2..i+3, j], that is u, v[i-3..i+3, j-3..j+3, k-1..k+1], and w[i-1, j], w[i, j-1]: "
             "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo ({},{},{}))")
VI_HALO = ("the rule reads u, v[i-3..i+3, j-3..j+3, k-3..k+3 within 0..Nz+1] and w[i-2..i+1, j], w[i, j-2..j+1]: "
           "Hx >= 3, Hy >= 3 and Hz >= 1 needed (halo ({},{},{}))")
HALO_FORMAT = "the rule reads {}: Hx >= {m}, Hy >= {m} and Hz >= 1 needed (halo ({},{},{}))"
STENCILS = {"centred": ("u, v[i-1..i+1, j-1..j+1, k-1..k+1] and w[i-1, j], w[i, j-1]", 1),
            "weno": ("Z[i, j-2..j+3] and Z[i-2..i+3, j], that is u, v[i-3..i+3, j-3..j+3, k-1..k+1], and w[i-1, j], w[i, j-1]", 3),
            "weno_vi": ("u, v[i-3..i+3, j-3..j+3, k-3..k+3 within 0..Nz+1] and w[i-2..i+1, j], w[i, j-2..j+1]", 3)}


def _cases():
    """(what it is, status, message, keyword arguments of _call) per shared check, each member of a grouped message on its own"""
    null_metric = "null dx_fc, dy_fc, az_fc, dx_cf, dy_cf, az_cf, az_cc, az_ff or dz_f"
    aligned = "pointer not aligned to its element type"
    why = " (every item reads cells while its neighbours write)"
    cases = [(f"null {name}", -1, "null u, v or w", {name: None}) for name in ("u", "v", "w")]
    cases += [(f"null {name}", -1, "null Gu or Gv", {name: None}) for name in ("Gu", "Gv")]
    cases += [(f"null {name}", -1, null_metric, {name: None}) for name in METRICS]
    cases += [("n_fc alone", -1, "the count planes n_fc and n_cf are given together or not at all (n_cf is null)", dict(n_fc=NFC)),
              ("n_cf alone", -1, "the count planes n_fc and n_cf are given together or not at all (n_fc is null)", dict(n_cf=NCF))]
    for ft, off in ((F64, 4), (F32, 2)):
        cases += [(f"misaligned {name}, ft {ft}", -1, f"u, v or w {aligned}", {name: AT[name] + off, "ft": ft}) for name in ("u", "v", "w")]
        cases += [(f"misaligned {name}, ft {ft}", -1, f"Gu or Gv {aligned}", {name: AT[name] + off, "ft": ft}) for name in ("Gu", "Gv")]
        cases += [(f"misaligned {name}, ft {ft}", -1, f"{', '.join(METRICS[:-1])} or dz_f {aligned}", {name: AT[name] + off, "ft": ft})
                  for name in METRICS]
    cases += [("misaligned n_fc", -1, "count plane pointer not aligned to int32", dict(n_fc=NFC + 2, n_cf=NCF)),
              ("misaligned n_cf", -1, "count plane pointer not aligned to int32", dict(n_fc=NFC, n_cf=NCF + 2))]
    # an output one element inside an input, from above (on its last element) and from below (the output's last element on its first)
    for out in ("Gu", "Gv"):
        for name, size in (("u", PARENT), ("v", PARENT), ("w", WPARENT)):
            for shift in (size - 8, 8 - PARENT):
                cases.append((f"{out} on {name}, {shift:+d}", -1, f"{out} overlaps {name}{why}", {**AWAY, name: BASE, out: BASE + shift}))
    cases += [(f"Gv on Gu, {shift:+d}", -1, "Gv overlaps Gu", dict(Gv=AT["Gu"] + shift)) for shift in (PARENT - 8, 8 - PARENT)]
    return cases


def _call(kind, lib, n_fc=None, n_cf=None, geom=GEOM, ft=F64, **over):
    s = {**AT, **over}
    head = (s["u"], s["v"], s["w"], s["Gu"], s["Gv"], *(s[k] for k in METRICS), n_fc, n_cf, 0.0)
    if kind == "centred":
        return lib.tpg_momentum_advection_tendency(*head, 0, *geom, ft, None), lib.tpg_momentum_last_error().decode()
    if kind == "weno_vi":                                          # the ninth table is dz_c here
        return lib.tpg_weno_vi_momentum_advection_tendency(*head, *geom, ft, None), lib.tpg_weno_vi_last_error().decode()
    return lib.tpg_weno_momentum_advection_tendency(*head, *geom, ft, None), lib.tpg_weno_momentum_last_error().decode()


@pytest.fixture(scope="module")
def libs(osg):
    return {"centred": osg._lib.momentum_lib(), "weno": osg._lib.weno_momentum_lib(), "weno_vi": osg._lib.weno_vi_lib()}


def test_shared_checks_answer_alike(libs):
    cases = _cases()
    assert len(cases) == 3 + 2 + 9 + 2 + 2 * (3 + 2 + 9) + 2 + 2 * 3 * 2 + 2
    for what, status, message, kw in cases:
        got = {kind: _call(kind, lib, **kw) for kind, lib in libs.items()}
        assert got["centred"] == got["weno"] == (status, message), what
        assert got["weno_vi"] == (status, message.replace("dz_f", "dz_c")), what


@pytest.mark.parametrize("halo", [(4, 4, 0), (0, 0, 0), (2, 4, 4)])
def test_halo_refusals_differ_in_the_stencil_only(libs, halo):
    assert _call("weno", libs["weno"], geom=GEOM[:3] + halo) == (-5, WENO_HALO.format(*halo))
    assert _call("weno_vi", libs["weno_vi"], geom=GEOM[:3] + halo) == (-5, VI_HALO.format(*halo))
    if halo != (2, 4, 4):                                          # a halo the centred stencil has room in: not a bad call of it
        assert _call("centred", libs["centred"], geom=GEOM[:3] + halo) == (-5, CENTRED_HALO.format(*halo))
    for kind, literal in (("centred", CENTRED_HALO), ("weno", WENO_HALO), ("weno_vi", VI_HALO)):      # one sentence around the stencil and its minimum
        stencil, least = STENCILS[kind]
        assert HALO_FORMAT.format(stencil, *halo, m=least) == literal.format(*halo)


def _raised(fn, *args, **kw):
    with pytest.raises(Exception) as e:
        fn(*args, **kw)
    return type(e.value), str(e.value)


def test_the_two_plans_are_one_body(osg):
    import torch
    from orthogonalsphericalshellgrids.jl_amd.momentum import _MomentumTendencyPlan
    assert issubclass(osg.MomentumAdvectionPlan, _MomentumTendencyPlan) and issubclass(osg.WenoMomentumAdvectionPlan, _MomentumTendencyPlan)
    assert issubclass(osg.WenoViMomentumAdvectionPlan, _MomentumTendencyPlan)
    assert osg.MomentumAdvectionPlan.__init__ is not osg.WenoMomentumAdvectionPlan.__init__            # each keeps its own defaults
    grid, other = _grid(osg), _grid(osg)
    u, v, w = osg.XFaceField(grid), osg.YFaceField(grid), osg.ZFaceField(grid)
    Gu, Gv, c = osg.XFaceField(grid), osg.YFaceField(grid), osg.CenterField(grid)
    makers = dict(u=osg.XFaceField, v=osg.YFaceField, w=osg.ZFaceField, Gu=osg.XFaceField, Gv=osg.YFaceField)
    f32 = lambda make: make(grid, data=torch.zeros(make(grid).data.shape, dtype=torch.float32))       # noqa: E731
    window = (slice(None), slice(None), range(1, 3))
    base = dict(u=u, v=v, w=w, Gu=Gu, Gv=Gv)
    loc = "{} must be a Field at ({})"
    calls = [(TypeError, loc.format("u", "Face, Center, Center"), dict(base, u=v)),
             (TypeError, loc.format("v", "Center, Face, Center"), dict(base, v=c)),
             (TypeError, loc.format("w", "Center, Center, Face"), dict(base, w=c)),
             (TypeError, loc.format("w", "Center, Center, Face"), dict(base, w=w.data)),
             (TypeError, loc.format("Gu", "Face, Center, Center"), dict(base, Gu=Gv)),
             (TypeError, loc.format("Gv", "Center, Face, Center"), dict(base, Gv=osg.XFaceField(grid))),
             (TypeError, loc.format("Gu", "Face, Center, Center"), dict(base, Gu=Gu.data))]
    for name in ("v", "w", "Gu", "Gv"):
        calls += [(ValueError, "u, v, w, Gu and Gv must live on one grid", dict(base, **{name: makers[name](other)})),
                  (ValueError, "u, v, w, Gu and Gv must share one element type and device", dict(base, **{name: f32(makers[name])}))]
    calls += [(NotImplementedError, "z-windowed fields are not handled", dict(base, **{name: makers[name](grid, indices=window)})) for name in makers]
    reason = " (every node reads its neighbours while they are written)"
    calls += [(ValueError, "Gu is u itself" + reason, dict(base, Gu=u)),
              (ValueError, "Gv is v itself" + reason, dict(base, Gv=osg.YFaceField(grid, data=v.data))),
              (ValueError, "Gu is u itself" + reason, dict(base, Gu=osg.XFaceField(grid, data=u.data))),
              (ValueError, "Gu and Gv are one field", dict(base, Gv=osg.YFaceField(grid, data=Gu.data)))]
    one_shot = lambda f: lambda u_, v_, w_, a, b: f(u_, v_, w_, out=(a, b))                            # noqa: E731
    forms = {"momentum_advection_plan": osg.momentum_advection_plan, "weno_momentum_advection_plan": osg.weno_momentum_advection_plan,
             "momentum_advection_tendency": one_shot(osg.momentum_advection_tendency),
             "weno_momentum_advection_tendency": one_shot(osg.weno_momentum_advection_tendency),
             "weno_vi_momentum_advection_plan": osg.weno_vi_momentum_advection_plan,
             "weno_vi_momentum_advection_tendency": one_shot(osg.weno_vi_momentum_advection_tendency)}
    for kind, message, fields in calls:
        for what, fn in forms.items():
            assert _raised(fn, *fields.values()) == (kind, f"{what}: {message}"), (what, message)
    # out=None: one helper allocates for the one-shot calls, and only after u is known to be an XFace field
    for what in ("momentum_advection_tendency", "weno_momentum_advection_tendency", "weno_vi_momentum_advection_tendency"):
        for bad in (v, u.data):
            assert _raised(getattr(osg, what), bad, v, w) == (TypeError, f"{what}: u must be a Field at (Face, Center, Center)")
