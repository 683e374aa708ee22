"""GPU: cfd_script_options -- the double pressure residual of solvers 2, 4 and 5
(residual_f64) bit for bit against the restatements, the option on against the
option off, cfd_script_update with residual_scaling against the script's own
numbers under node (tests/golden/js_update_scaling_*.npz), residual_f64 alone on
an existing js_update_* fixture, and the ABI's edges.

Shapes.  Solver 4 gives a wave a band of 64 interior rows: the three- and
four-band cases of _sor_lex_cases.py with the maximum in the first, a middle
and the last band, and an exit at the first and at the last iteration.  Solver 5
tiles the grid by workgroups of 4 waves, a wave 124 columns (62 pairs) by 4
interior rows (launch_jacobi_script: nwc = ceil(nx / 2 / 62) wave columns,
ceil(ceil((ny - 2) / 4) / 4) workgroup rows): 256 x 36 is 3 x 3 workgroups with
a ragged last one each way, 16 x 4 is one wave of one workgroup.  Solver 2: the
one-level 16 x 4 and the four-level 216 x 57 of test_gpu_solver_seams.py, and
its one-level 2048 x 4 for the NaN case.
"""
import json
import os
import sys

import numpy as np
import pytest

import _jacobi_script_ref as jac
import _script_step_ref as step
import _script_update_ref as upd
import _sor_lex_cases as lex
from _util import assert_bitwise

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
SCAL = json.load(open(os.path.join(GOLD, "js_update_scaling_manifest.json")))
UPD = json.load(open(os.path.join(GOLD, "js_update_manifest.json")))

LEX_CASES = ["first_band", "middle_band", "last_band_s0.03", "four_bands_odd",
             "four_bands_first_iteration", "first_band_exit_at_last",
             # fixed counts (no exit test), three and four bands
             "24x130_fixed7", "32x195_fixed7"]
JAC_SHAPES = [(256, 36), (16, 4)]
MG_SHAPES = [(16, 4), (216, 57)]
LX, LY = 30.0, 10.0


def _cfd():
    import cfdamd
    return cfdamd


def _bits(x):
    return np.float64(x).view(np.uint64)


# ---- the solve-level cases: name -> (solver, nx, ny, lx, ly, iters, tol, p_tol, rhs, p', n, double)
_SOLVES = {}


def _jac_rhs(nx, ny, scale, seed=77):
    return (np.random.default_rng(seed + nx).uniform(-1, 1, nx * ny) * scale).astype(np.float32)


def _solve_case(name):
    if name in _SOLVES:
        return _SOLVES[name]
    kind, _, tag = name.partition(":")
    if kind == "lex":
        c = lex.BY_NAME[tag]
        rhs, want, n, errs = lex.restated(c)
        out = (4, c.nx, c.ny, c.lx, c.ly, c.iters, c.tol, lex.P_TOL, rhs, want, n, errs[-1])
    elif kind == "jac":
        shape, mode = tag.split("-")
        nx, ny = (int(x) for x in shape.split("x"))
        dx, dy = np.float32(LX) / np.float32(nx), np.float32(LY) / np.float32(ny)
        # fixed: 9 iterations, none below p_tol; exit: a small rhs meets 1e-6 mid-run
        iters, tol, scale = (9, False, 1.0) if mode == "fixed" else (400, True, 1e-3 if nx > 16 else 1e-4)
        rhs = _jac_rhs(nx, ny, scale)
        want, n, errs = jac.jacobi_script(rhs, nx, ny, dx, dy, iters, tol, jac.P_TOL)
        if mode == "exit":
            assert 1 < n < iters, (name, n)
        out = (5, nx, ny, LX, LY, iters, tol, jac.P_TOL, rhs, want, n, errs[-1])
    else:
        nx, ny = (int(x) for x in tag.split("x"))
        g = step.Grid(nx, ny, LX, LY, 0.01, None)
        rhs = _jac_rhs(nx, ny, 1.0, seed=99)
        want, r = upd.solve(g, rhs.reshape(ny, nx), 2)
        out = (2, nx, ny, LX, LY, 50, True, 1e-4, rhs, want, 1, r)
    for a in out[8:10]:
        a.setflags(write=False)
    _SOLVES[name] = out
    return out


SOLVE_NAMES = (["lex:" + n for n in LEX_CASES] +
               [f"jac:{nx}x{ny}-{m}" for nx, ny in JAC_SHAPES for m in ("fixed", "exit")] +
               [f"mg:{nx}x{ny}" for nx, ny in MG_SHAPES])


def _solve_model(c, case, f64, iters=None):
    solver, nx, ny, lx, ly, it, tol, p_tol = case[:8]
    m = c.Model(c.Grid(nx, ny, lx, ly),
                c.SimulationParams(pressure_solver=c.PressureSolver(solver),
                                   jacobi_iters=it if iters is None else iters, tol_enabled=tol,
                                   p_tol=p_tol))
    if f64:
        assert m.script_options(residual_f64=True) == dict(residual_f64=1, residual_scaling=0)
    return m


def _run_solve(m, rhs):
    m.set_state(rhs=rhs)
    before = m.get_state()["jacobi_sweeps_total"]
    r = m.pressure_solve()
    st = m.get_state()
    return st["p_prime"], np.float32(r), np.float32(st["last_p_residual"]), st["jacobi_sweeps_total"] - before


@pytest.mark.parametrize("name", SOLVE_NAMES)
def test_solve_publishes_the_scripts_double(name):
    """p_residual_f64()[0] is the restatement's double, its f32 is
    last_p_residual, and everything else is what the option-off solve gives."""
    c = _cfd()
    case = _solve_case(name)
    rhs, want, n, dbl = case[8:]
    m = _solve_model(c, case, True)
    try:
        pp, r, last, ran = _run_solve(m, rhs)
        got = m.p_residual_f64()[0]
        assert _bits(got) == _bits(dbl), (name, got, dbl)
        assert np.float32(got) == last == r, (name, got, last, r)
        assert_bitwise(f"{name}: p'", pp, want.reshape(-1))
        assert ran == n, (name, ran, n)
        # a second solve on the same model: the slot sets were left clean
        pp2, r2, _, ran2 = _run_solve(m, rhs)
        assert _bits(m.p_residual_f64()[0]) == _bits(dbl) and ran2 == n and r2 == r, name
    finally:
        m.close()
    off = _solve_model(c, case, False)
    try:
        pp0, r0, last0, ran0 = _run_solve(off, rhs)
        assert_bitwise(f"{name}: p', option on vs off", pp, pp0)
        assert (r.view(np.uint32), last.view(np.uint32), ran) == (r0.view(np.uint32), last0.view(np.uint32), ran0), name
    finally:
        off.close()


@pytest.mark.parametrize("name", ["lex:middle_band", "jac:256x36-fixed", "mg:2048x4"])
def test_nan_in_rhs_is_ignored_by_the_double(name):
    """A NaN planted in rhs away from the maximum: the restatement's maximum
    skips the NaN cells (`>` never takes one), and so does the device's double.
    The multigrid runs on the one-level 2048 x 4 of test_gpu_solver_seams.py:
    its 45 smoothing sweeps carry the NaN 45 columns each way and no further, so
    the finite maximum of the other 98 % of the grid survives beside it (a
    coarser level would spread it over the whole grid)."""
    c = _cfd()
    case = _solve_case(name)
    solver, nx, ny = case[:3]
    rhs = case[8].copy()
    if solver == 4:
        # two iterations: the NaN has reached its neighbours only, rows away from the maximum
        rhs[8 + 120 * nx] = np.nan
        cc = lex.BY_NAME["middle_band"]
        want, n, errs = lex.solve(cc, rhs, iters=2, tol=False)
        dbl, iters = errs[-1], 2
        case = case[:6] + (False,) + case[7:]
    elif solver == 5:
        rhs[5 + 3 * nx] = np.nan
        dx, dy = np.float32(LX) / np.float32(nx), np.float32(LY) / np.float32(ny)
        want, n, errs = jac.jacobi_script(rhs, nx, ny, dx, dy, 3, False, jac.P_TOL)
        dbl, iters = errs[-1], 3
    else:
        rhs[1000 + 1 * nx] = np.nan
        want, dbl = upd.solve(step.Grid(nx, ny, LX, LY, 0.01, None), rhs.reshape(ny, nx), 2)
        iters = None
    assert np.isnan(want).any() and np.isfinite(dbl) and dbl > 0
    m = _solve_model(c, case, True, iters=iters)
    try:
        pp, r, last, _ = _run_solve(m, rhs)
        got = m.p_residual_f64()[0]
        assert _bits(got) == _bits(dbl), (name, got, dbl)
        assert np.float32(got) == last, name
        assert_bitwise(f"{name}: p'", pp, want.reshape(-1), nan_equal=True)
    finally:
        m.close()


@pytest.mark.parametrize("solver", [4, 5])
def test_no_iterations_publish_zero(solver):
    c = _cfd()
    m = c.Model(c.Grid(16, 4, LX, LY), c.SimulationParams(pressure_solver=c.PressureSolver(solver),
                                                         jacobi_iters=0, tol_enabled=True, p_tol=1e-4))
    try:
        m.script_options(residual_f64=True)
        m.set_state(rhs=_jac_rhs(16, 4, 1.0))
        assert m.pressure_solve() == 0.0
        assert m.p_residual_f64()[0] == 0.0
    finally:
        m.close()


# ---- script_update
def _model(c, meta, man, solver=None):
    solver = meta["solver"] if solver is None else solver
    cyl = c.Cylinder(*meta["cylinder"]) if meta["cylinder"] else None
    return c.Model(c.Grid(meta["nx"], meta["ny"], meta["lx"], meta["ly"], cyl),
                   c.SimulationParams(viscosity=man["viscosity"], pressure_solver=c.PressureSolver(solver),
                                      jacobi_iters=man["iters"], tol_enabled=True,
                                      p_tol=man["p_tol"][str(solver)]))


def _begin(m, meta, fx):
    m.set_state(u=fx["start_u"].ravel(), v=fx["start_v"].ravel(), p=fx["start_p"].ravel())
    m.script_begin(dict(dt=meta["start_dt"], substep_count=meta["start_substep_count"],
                        step_count=meta["start_step_count"], u_prev=fx["start_u_prev"],
                        v_prev=fx["start_v_prev"]))


def _cfg(c, meta):
    return (c.ScriptScheme(meta["scheme"]), meta["target"], meta["dt_user"], c.InletProfile(meta["profile"]))


def _check_report(tag, r, meta, fx, s, nsub_before):
    assert r.step_count == meta["start_step_count"] + s + 1, tag
    assert r.substeps_run == nsub_before, tag
    got = np.array([r.residual_u, r.residual_v, r.residual_p, r.dt_next, r.inlet_velocity])
    want = np.array([fx["res_u"][s], fx["res_v"][s], fx["res_p"][s], fx["dt"][s], fx["inlet"][s]])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (tag, got, want)
    assert r.substep_count_next == fx["substeps"][s], tag


def _check_final(tag, m, meta, fx):
    st = m.get_state()
    for f in ("u", "v", "p"):
        assert_bitwise(f"{tag}: {f}", st[f], fx["steps_" + f][-1].ravel())
    ss = m.script_state()
    assert_bitwise(f"{tag}: u_prev", ss["u_prev"], fx["final_u_prev"].ravel())
    assert_bitwise(f"{tag}: v_prev", ss["v_prev"], fx["final_v_prev"].ravel())
    assert (ss["dt"], ss["substep_count"], ss["step_count"]) == \
        (fx["dt"][-1], fx["substeps"][-1], meta["start_step_count"] + meta["steps"]), tag


@pytest.mark.parametrize("name", sorted(SCAL["fixtures"]))
def test_update_with_residual_scaling_matches_reference_javascript(name):
    """Every step of every scaling fixture, one call per step and through
    script_update_n: fields, uPrev / vPrev, the report and the state's dt and
    substep count are the script's bits."""
    c = _cfd()
    meta = SCAL["fixtures"][name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    K = meta["steps"]
    nsubs = [meta["start_substep_count"]] + [int(x) for x in fx["substeps"][:-1]]
    m = _model(c, meta, SCAL)
    try:
        assert m.script_options(residual_scaling=True) == dict(residual_f64=1, residual_scaling=1)
        _begin(m, meta, fx)
        assert m.script_options() == dict(residual_f64=1, residual_scaling=1)   # survives script_begin
        for s in range(K):
            r = m.script_update(*_cfg(c, meta))
            _check_report(f"{name} step {s}", r, meta, fx, s, nsubs[s])
            st = m.get_state()
            for f in ("u", "v", "p"):
                assert_bitwise(f"{name} step {s}: {f}", st[f], fx["steps_" + f][s].ravel())
            assert _bits(m.p_residual_f64()[1]) == _bits(fx["res_p"][s]), (name, s)
            ss = m.script_state()
            assert (ss["dt"], ss["substep_count"]) == (fx["dt"][s], fx["substeps"][s]), (name, s)
        _check_final(name, m, meta, fx)
    finally:
        m.close()
    m = _model(c, meta, SCAL)
    try:
        m.script_options(residual_scaling=True)
        _begin(m, meta, fx)
        reps = m.script_update_n(K, *_cfg(c, meta))
        assert len(reps) == K
        for s, r in enumerate(reps):
            _check_report(f"{name} update_n step {s}", r, meta, fx, s, nsubs[s])
        _check_final(f"{name} update_n", m, meta, fx)
    finally:
        m.close()


@pytest.mark.parametrize("name", ["js_update_40x12_cyl_quick_jac", "js_update_16x5_rest_quick_sor",
                                  "js_update_24x7_ramp_second_mg_p2"])
def test_residual_f64_alone_keeps_the_bits_and_reports_the_double(name):
    """residual_f64 on, scaling off, on an existing fixture: the same fields and
    decisions as today, residual_p now the script's double."""
    c = _cfd()
    meta = UPD["fixtures"][name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    K = meta["steps"]
    nsubs = [meta["start_substep_count"]] + [int(x) for x in fx["substeps"][:-1]]
    m = _model(c, meta, UPD)
    try:
        assert m.script_options(residual_f64=True) == dict(residual_f64=1, residual_scaling=0)
        _begin(m, meta, fx)
        for s in range(K):
            r = m.script_update(*_cfg(c, meta))
            _check_report(f"{name} step {s}", r, meta, fx, s, nsubs[s])
            st = m.get_state()
            for f in ("u", "v", "p"):
                assert_bitwise(f"{name} step {s}: {f}", st[f], fx["steps_" + f][s].ravel())
    finally:
        m.close()


# ---- ABI edges
def test_options_are_rejected_where_they_cannot_hold():
    c = _cfd()
    from cfdamd._lib import CfdError, CfdScriptOptions, load
    import ctypes as C
    m = c.Model(c.Grid(16, 4, LX, LY), c.SimulationParams(pressure_solver=c.PressureSolver(5)))
    try:
        assert m.script_options() == dict(residual_f64=0, residual_scaling=0)
        for bad in ((2, 0), (0, 2), (-1, 0), (0, -1)):
            o = CfdScriptOptions(*bad)
            assert load().cfd_script_set_options(m._hh(), C.byref(o)) == c._lib.CFD_EINVAL, bad
        assert m.script_options() == dict(residual_f64=0, residual_scaling=0)
    finally:
        m.close()
    hub = c.LocalHub(2)
    grid, params = c.Grid(64, 64, 1.0, 1.0), c.SimulationParams(tol_enabled=False, jacobi_iters=8)
    ms = [c.Model(grid, params, device=0, n_ranks=2, rank=r, local_hub=hub) for r in range(2)]
    try:
        with pytest.raises(CfdError) as e:
            ms[0].script_options(residual_f64=True)
        assert e.value.code == c._lib.CFD_EINVAL
    finally:
        for x in ms:
            x.close()


def test_double_is_refused_until_a_solve_publishes_one():
    c = _cfd()
    from cfdamd._lib import CfdError
    estate = c._lib.CFD_ESTATE

    def refused(m):
        with pytest.raises(CfdError) as e:
            m.p_residual_f64()
        return e.value.code == estate

    rhs = _jac_rhs(16, 4, 1.0)
    m = c.Model(c.Grid(16, 4, LX, LY), c.SimulationParams(pressure_solver=c.PressureSolver(5),
                                                         jacobi_iters=5, tol_enabled=False))
    try:
        m.set_state(rhs=rhs)
        m.pressure_solve()
        assert refused(m)                       # the option is off
        m.script_options(residual_f64=True)
        assert refused(m)                       # on, nothing published yet
        m.pressure_solve()
        last = m.p_residual_f64()[0]
        assert last > 0.0 and np.float32(last) == np.float32(m.get_state()["last_p_residual"])
        m.set_state(rhs=rhs)
        assert refused(m)                       # cfd_set_state cleared it
        m.pressure_solve()
        assert m.p_residual_f64()[0] == last
        # a solver-0 solve publishes none
        m.set_parameters(c.SimulationParams(pressure_solver=c.PressureSolver(0), jacobi_iters=5,
                                            tol_enabled=False))
        m.pressure_solve()
        assert refused(m)
        m.script_options(residual_f64=False)
        assert refused(m)
    finally:
        m.close()
