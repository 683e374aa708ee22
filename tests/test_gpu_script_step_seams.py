"""GPU: k_script_predict and k_script_correct (cfd_script_step.hip) at their
seams, bit for bit against the restatement (tests/_script_step_ref.py) on the
cases of tests/_script_step_cases.py, whose premises
test_script_step_seams_cpu.py checks without a device:

* the predictor's wave columns and row segments -- the face-nx chunk on lane 5
  (the smallest grid), 61 (its right neighbour out of the domain), alone in the
  next wave column (248, 496) and two lanes further (256); R = 4 and R = 8, one
  segment, an overlapping last segment, a fifth segment in a second block --
  for every scheme on both division paths, with a cylinder where one fits;
* discs clipped by the inlet, the outlet, the walls and the corners, a disc
  with one u face and no v face, one smaller than any face and one outside the
  domain, through both kernels and both inlet profiles;
* values that overflow f32 on the one rounding, that land on f32 subnormals,
  and NaN / +-Inf at wave and segment seams and on the first and last column;
* the whole substep once per solver (2, 4, 5) on a seam shape.

The two kernels run separately through script_phase, so no solver sits between
the input and the assertion.  Every comparison is bitwise on the u32 views;
nan_equal only where the restatement itself holds a NaN (the `nonfinite`
flavour, and the rhs of `huge`, which subtracts stored infinities), and there
the NaN and the +-Inf words sit exactly where the restatement has them.
"""
import numpy as np
import pytest

import _script_step_cases as t
import _script_step_ref as ref
from _util import assert_bitwise
from test_gpu_script_step import _check_against_restatement

pytestmark = pytest.mark.gpu


def _model(g, solver=5):
    import cfdamd
    cyl = cfdamd.Cylinder(*g.cyl) if g.cyl else None
    params = cfdamd.SimulationParams(viscosity=g.nu, pressure_solver=cfdamd.PressureSolver(solver),
                                     jacobi_iters=20, tol_enabled=True, p_tol=1e-4)
    return cfdamd.Model(cfdamd.Grid(g.nx, g.ny, g.lx, g.ly, cyl), params)


def _shapes(g):
    return {"u": (g.ny, g.nx + 1), "v": (g.ny + 1, g.nx), "p": (g.ny, g.nx)}


def _same(tag, got, want, nan_equal=False):
    """Bitwise; with nan_equal also: NaN where the restatement has NaN, the
    infinities where it has them, sign included."""
    got = np.asarray(got).reshape(np.shape(want))
    assert_bitwise(tag, got, want, nan_equal=nan_equal)
    if nan_equal:
        assert np.array_equal(np.isnan(got), np.isnan(want)), tag
        assert np.array_equal(np.isposinf(got), np.isposinf(want)), tag
        assert np.array_equal(np.isneginf(got), np.isneginf(want)), tag


def _predict_and_check(tag, m, g, u, v, p, dt_sub, scheme, want, nan_equal=(False, False, False)):
    import cfdamd
    sh = _shapes(g)
    junk = {f: np.full(sh[k], 7.0, np.float32) for f, k in (("u_star", "u"), ("v_star", "v"), ("rhs", "p"))}
    m.set_state(u=u, v=v, p=p, **junk)     # every word of the outputs is written
    m.script_phase(cfdamd.ScriptPhase.Predict, dt_sub, scheme, t.INLET, 0)
    st = m.get_state()
    for f, k, w, ne in (("u_star", "u", want[0], nan_equal[0]), ("v_star", "v", want[1], nan_equal[1]),
                        ("rhs", "p", want[2], nan_equal[2])):
        _same(f"{tag}:{f}", st[f], w, ne)
    for f, a in (("u", u), ("v", v), ("p", p)):     # inputs untouched
        _same(f"{tag}:{f}", st[f], a, nan_equal=bool(np.isnan(a).any()))


def _correct_and_check(tag, m, g, us, vs, pp, p, dt_sub, profile, want, nan_equal=False):
    import cfdamd
    sh = _shapes(g)
    rhs = np.full(sh["p"], 3.0, np.float32)
    m.set_state(u=np.full(sh["u"], 7.0, np.float32), v=np.full(sh["v"], 7.0, np.float32), p=p,
                u_star=us, v_star=vs, p_prime=pp, rhs=rhs)
    m.script_phase(cfdamd.ScriptPhase.Correct, dt_sub, t.DISC_SCHEME, t.INLET, profile)
    st = m.get_state()
    for f, w in zip(("u", "v", "p"), want):
        _same(f"{tag}:{f}", st[f], w, nan_equal)
    for f, a in (("u_star", us), ("v_star", vs), ("p_prime", pp), ("rhs", rhs)):
        _same(f"{tag}:{f}", st[f], a, nan_equal=bool(np.isnan(a).any()))


# ------------------------------------------------------------ predictor shapes
@pytest.mark.parametrize("name", [c.name for c in t.DEVICE_CASES])
def test_predictor_shape_matches_restatement(name):
    c = t.BY_NAME[name]
    g = t.grid_of(c)
    m = _model(g)
    try:
        for scheme in t.SCHEMES:
            u, v, p, us, vs, rhs, _ = t.predicted(c, scheme)
            _predict_and_check(f"{name} scheme {scheme}", m, g, u, v, p, c.dt_sub, scheme, (us, vs, rhs))
    finally:
        m.close()


@pytest.mark.parametrize("solver", t.SUBSTEP_SOLVERS)
def test_whole_substep_on_a_seam_shape(solver):
    c = t.BY_NAME[t.SUBSTEP_CASE]
    g = t.grid_of(c)
    m = _model(g, solver)
    try:
        u, v, p = t.random_state(g, c.seed, c.dt_sub, cfl=0.3)
        m.set_state(u=u, v=v, p=p)
        before = m.get_state()
        m.script_piso_step(c.dt_sub, ref.QUICK, t.INLET, 1)
        _check_against_restatement(f"{c.name} solver {solver}", g, m, before, m.get_state(), c.dt_sub,
                                   ref.QUICK, t.INLET, 1)
    finally:
        m.close()


# ---------------------------------------------------------------- clipped discs
@pytest.mark.parametrize("name", [d.name for d in t.DEVICE_DISCS])
def test_clipped_disc_matches_restatement(name):
    """A disc the script accepts is accepted (one outside the domain included:
    every interval empty); Predict, then Correct under both inlet profiles."""
    d = t.DISC_BY_NAME[name]
    g = t.disc_grid(d)
    m = _model(g)
    try:
        u, v, p, us, vs, rhs = t.disc_predicted(d)
        _predict_and_check(f"{name} predict", m, g, u, v, p, t.DT_SUB, t.DISC_SCHEME, (us, vs, rhs))
        for profile in t.PROFILES:
            cs, cv, cpp, cp, wu, wv, wp = t.disc_corrected(d, profile)
            _correct_and_check(f"{name} correct profile {profile}", m, g, cs, cv, cpp, cp, t.DT_SUB,
                               profile, (wu, wv, wp))
    finally:
        m.close()


# --------------------------------------------------------------- extreme values
@pytest.mark.parametrize("flavour", t.FLAVOURS)
@pytest.mark.parametrize("nx,ny", t.EXTREME_DEVICE_SHAPES)
def test_extreme_values_in_the_predictor(nx, ny, flavour):
    models = {}
    try:
        for scheme in t.SCHEMES:
            g, dt_sub, u, v, p, us, vs, rhs = t.extreme_predicted(nx, ny, flavour, scheme)
            key = (g.lx, g.ly)
            if key not in models:
                models[key] = _model(g)
            if flavour == "nonfinite":
                ne = (True, True, True)
            else:     # u*, v* come from finite doubles; the rhs of `huge` subtracts infinities
                assert not np.isnan(us).any() and not np.isnan(vs).any()
                ne = (False, False, bool(np.isnan(rhs).any()))
                assert not ne[2] or flavour == "huge"
            _predict_and_check(f"{nx}x{ny} {flavour} scheme {scheme}", models[key], g, u, v, p, dt_sub,
                               scheme, (us, vs, rhs), ne)
    finally:
        for m in models.values():
            m.close()


@pytest.mark.parametrize("path", t.PATHS)
@pytest.mark.parametrize("flavour", t.FLAVOURS)
def test_extreme_values_in_the_corrector(flavour, path):
    g, dt_sub, us, vs, pp, p, wu, wv, wp = t.extreme_corrected(flavour, path)
    m = _model(g)
    try:
        if flavour != "nonfinite":
            assert not any(np.isnan(a).any() for a in (wu, wv, wp))
        _correct_and_check(f"corrector {flavour} {path}", m, g, us, vs, pp, p, dt_sub, ref.PARABOLIC,
                           (wu, wv, wp), nan_equal=flavour == "nonfinite")
    finally:
        m.close()
