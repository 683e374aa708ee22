"""GPU: pressure_solver 4 (cfd_sor_lex.hip) at its seams, bit for bit against
the restatement (tests/_sor_lex_ref.py) on the cases of tests/_sor_lex_cases.py,
whose premises test_sor_lex_seams_cpu.py checks without a device:

* tolerance exits on three and four bands -- the maximum in the first, a
  middle and the last band, an exit at the first and at the last iteration, a
  replay of one iteration, both parities, an all-zero rhs: the residual fold
  across bands, the exit word raced by iterations that ran ahead, the replay;
* band shapes (ny - 2 = 2, 63, 64, 65, 128, 129, 193: a one-row last band that
  takes the exit test) and both remainders of the last 16-step chunk
  ((nx + 62) % 16 = 14 and 6; a width off the 8-grid is refused at create);
* stale state: NaN in both p' buffers, either buffer current, the exit word of
  an earlier solve, the polled block regrown through set_parameters;
* a non-finite rhs word that crosses a band seam through memory;
* the solve inside script_piso_step and Model.update on three bands with the
  tolerance met.

Every case runs at CFD_SOR_LEX_WGS = default, 1, 2, 3 (the non-finite ones at
default and 1) through Model.pressure_solve().  All comparisons are bitwise.
"""
import numpy as np
import pytest

import _script_step_ref as sref
import _sor_lex_cases as t
import _sor_lex_ref as ref
from _util import assert_bitwise
from test_gpu_script_step import _check_against_restatement, _random_state

pytestmark = pytest.mark.gpu

WGS = ["default", "1", "2", "3"]


def _cfd():
    import cfdamd
    return cfdamd


def _set_wgs(monkeypatch, wgs):
    if wgs == "default":
        monkeypatch.delenv("CFD_SOR_LEX_WGS", raising=False)
    else:
        monkeypatch.setenv("CFD_SOR_LEX_WGS", wgs)


def _params(c, case, **kw):
    return c.SimulationParams(pressure_solver=c.PressureSolver.SorLex, jacobi_iters=case.iters,
                              tol_enabled=case.tol, p_tol=t.P_TOL, **kw)


def _nan(case):
    return np.full(case.nx * case.ny, np.nan, np.float32)


def _solve_and_check(tag, m, rhs, want, n, errs, stale=None, nan_equal=False):
    """One pressure_solve() of `m` on rhs against (want, n, errs) of the restatement."""
    kw = dict(rhs=rhs) if stale is None else dict(rhs=rhs, p_prime=stale)
    m.set_state(**kw)
    before = m.get_state()["jacobi_sweeps_total"]
    r = m.pressure_solve()
    st = m.get_state()
    assert_bitwise(f"{tag}: p'", st["p_prime"], want.reshape(-1), nan_equal=nan_equal)
    assert np.float32(r) == np.float32(errs[-1]), (tag, r, errs[-1])
    assert np.float32(st["last_p_residual"]) == np.float32(errs[-1]), tag
    assert st["jacobi_sweeps_total"] - before == n, (tag, st["jacobi_sweeps_total"] - before, n)


@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("name", [c.name for c in t.DEVICE_CASES])
def test_table_case_matches_restatement(monkeypatch, name, wgs):
    c = _cfd()
    _set_wgs(monkeypatch, wgs)
    case = t.BY_NAME[name]
    rhs, want, n, errs = t.restated(case)
    m = c.Model(c.Grid(case.nx, case.ny, case.lx, case.ly), _params(c, case))
    try:
        # NaN in both p' buffers: set_state fills the current one, a solve of one
        # iteration writes the other and makes it current, set_state fills that.
        # Iteration 0 reads zeros (index.html:743), and every cell of the result
        # is written, whichever buffer it lands in: a stale NaN would show
        m.set_state(p_prime=_nan(case))
        m.set_parameters(_params(c, case._replace(iters=1, tol=False)))
        m.pressure_solve()
        m.set_parameters(_params(c, case))
        _solve_and_check(f"{name} wgs={wgs}", m, rhs, want, n, errs, stale=_nan(case))
    finally:
        m.close()


@pytest.mark.parametrize("wgs", WGS)
def test_stale_buffers_exit_word_and_polled_block(monkeypatch, wgs):
    """STALE_SEQUENCE on one model.  set_state writes the current p' buffer
    only, and a solve leaves the buffer current that its last iteration wrote:
    NaN goes into one buffer before the odd fixed-count solve and into the
    other before the one-iteration solve, which writes a single buffer -- so
    both hold NaN before the first tolerance solve, which then exits mid-run.
    The next solve never meets the tolerance (the exit word of the one before
    must not end it), the fourth needs a longer polled block, the last a
    shorter one."""
    c = _cfd()
    _set_wgs(monkeypatch, wgs)
    seq = t.STALE_SEQUENCE
    assert [k.iters for k in seq] == [7, 1, 26, 9, 100, 30] and t.bands(seq[0].ny) == 3
    m = c.Model(c.Grid(seq[0].nx, seq[0].ny, seq[0].lx, seq[0].ly), _params(c, seq[0]))
    try:
        for k, case in enumerate(seq):
            rhs, want, n, errs = t.restated(case)
            if k:
                m.set_parameters(_params(c, case))
            # NaN into the current buffer before the first three, then whatever the
            # solve before left (the finite p' of an exit or of a full run)
            _solve_and_check(f"solve {k} ({case.name}) wgs={wgs}", m, rhs, want, n, errs,
                             stale=_nan(case) if k < 3 else None)
    finally:
        m.close()


@pytest.mark.parametrize("wgs", ["default", "1"])
@pytest.mark.parametrize("k", range(len(t.NONFINITE_CASES)))
def test_nonfinite_rhs_crosses_a_band_seam(monkeypatch, k, wgs):
    """The script's `error > maxError` ignores NaN, and so does the kernel's
    fold; the spoilt cells (under 5 % of the grid, asserted on the CPU) compare
    as any NaN with any NaN, every other word bitwise.  cfd_pressure_solve
    documents no non-finite report: the call returns the residual as usual."""
    c = _cfd()
    _set_wgs(monkeypatch, wgs)
    case, word = t.NONFINITE_CASES[k]
    rhs, want, n, errs = t.nonfinite_restated(case, word)
    m = c.Model(c.Grid(case.nx, case.ny, case.lx, case.ly), _params(c, case))
    try:
        _solve_and_check(f"{case.name} wgs={wgs}", m, rhs, want, n, errs,
                         stale=np.full(case.nx * case.ny, 7.0, np.float32), nan_equal=True)
        # the non-finite words themselves sit where the restatement has them
        got = m.get_state()["p_prime"]
        assert np.array_equal(np.isnan(got), np.isnan(want.reshape(-1)))
        assert np.array_equal(np.isinf(got), np.isinf(want.reshape(-1)))
    finally:
        m.close()


def _step_grid():
    return sref.Grid(**t.STEP_GRID)


@pytest.mark.parametrize("wgs", WGS)
def test_script_substep_exits_on_three_bands(monkeypatch, wgs):
    """script_piso_step, QUICK, cylinder: the solve in the middle is solver 4
    on three bands and meets the tolerance mid-run."""
    c = _cfd()
    _set_wgs(monkeypatch, wgs)
    g = _step_grid()
    dt_sub, scheme, inlet, profile = float(np.float32(0.004)), 2, 0.8, 1
    m = c.Model(c.Grid(g.nx, g.ny, g.lx, g.ly, c.Cylinder(*g.cyl)),
                c.SimulationParams(viscosity=g.nu, pressure_solver=c.PressureSolver.SorLex,
                                   jacobi_iters=t.STEP_ITERS, tol_enabled=True, p_tol=t.P_TOL))
    try:
        u, v, p = _random_state(g, 4500, dt_sub, cfl=t.STEP_CFL)
        m.set_state(u=u, v=v, p=p, p_prime=np.full(g.nx * g.ny, np.nan, np.float32))
        before = m.get_state()
        m.script_piso_step(dt_sub, scheme, inlet, profile)
        st = m.get_state()
        want, n, errs = ref.sor_lex_diag(st["rhs"], g.nx, g.ny, g.dx, g.dy, t.STEP_ITERS, True, t.P_TOL)
        assert 1 < n < t.STEP_ITERS and not ref.slivers(errs, t.P_TOL), n
        assert_bitwise(f"substep wgs={wgs}: p'", st["p_prime"], want.reshape(-1))
        assert np.float32(st["last_p_residual"]) == np.float32(errs[-1])
        assert st["jacobi_sweeps_total"] - before["jacobi_sweeps_total"] == n
        _check_against_restatement(f"24x132 wgs={wgs}", g, m, before, st, dt_sub, scheme, inlet, profile)
    finally:
        m.close()


@pytest.mark.parametrize("wgs", WGS)
def test_update_exits_on_three_bands(monkeypatch, wgs):
    """Model.update with corrector_passes 0 (the step's only solve) on the same
    grid: p' is the restatement of the step's rhs, as in
    test_gpu_sor_lex.py::test_switching_solvers_mid_run, here with an exit."""
    c = _cfd()
    _set_wgs(monkeypatch, wgs)
    g = _step_grid()
    m = c.Model(c.Grid(g.nx, g.ny, g.lx, g.ly, c.Cylinder(*g.cyl)),
                c.SimulationParams(viscosity=g.nu, pressure_solver=c.PressureSolver.SorLex,
                                   jacobi_iters=t.STEP_ITERS, corrector_passes=0, tol_enabled=True,
                                   p_tol=t.P_TOL))
    try:
        u, v, p = _random_state(g, 4600, 0.005, cfl=t.STEP_CFL)
        m.set_state(u=u, v=v, p=p, p_prime=np.full(g.nx * g.ny, np.nan, np.float32),
                    simulation_step=50)
        for step in range(2):
            before = m.get_residuals().jacobi_sweeps_total
            m.update()
            st = m.get_state()
            want, n, errs = ref.sor_lex_diag(st["rhs"], g.nx, g.ny, g.dx, g.dy, t.STEP_ITERS, True,
                                             t.P_TOL)
            assert not ref.slivers(errs, t.P_TOL)
            if step == 0:
                assert 1 < n < t.STEP_ITERS, n
            assert_bitwise(f"update {step} wgs={wgs}: p'", st["p_prime"], want.reshape(-1))
            r = m.get_residuals()
            assert np.float32(r.p) == np.float32(errs[-1])
            assert r.jacobi_sweeps_total - before == n
    finally:
        m.close()
