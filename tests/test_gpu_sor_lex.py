"""GPU: pressure_solver 4, the JavaScript variant's SOR in the script's own
order (index.html:741-774; cfd_sor_lex.hip), bit for bit

* against the reference script itself, executed by node on the same inputs
  (tests/golden/js_sor_*.npz, make_js_sor_golden.py), at the default workgroup
  count and with CFD_SOR_LEX_WGS = 1, 2, 3 (fewer workgroups than bands and
  than iterations);
* against the anti-diagonal restatement (tests/_sor_lex_ref.py, pinned to the
  same fixtures by test_sor_lex_cpu.py) on larger grids;
* inside piso_step, Model::update and across solver switches.
"""
import json
import os

import numpy as np
import pytest

import _sor_lex_ref as ref
from _util import assert_bitwise

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
JS = json.load(open(os.path.join(GOLD, "js_sor_manifest.json")))["fixtures"]
FIELDS7 = ("u", "v", "p", "u_star", "v_star", "p_prime", "rhs")
WGS = ["default", "1", "2", "3"]


def _cfd():
    import cfdamd
    return cfdamd


def _set_wgs(monkeypatch, wgs):
    if wgs == "default":
        monkeypatch.delenv("CFD_SOR_LEX_WGS", raising=False)
    else:
        monkeypatch.setenv("CFD_SOR_LEX_WGS", wgs)


@pytest.mark.parametrize("wgs", WGS)
@pytest.mark.parametrize("name", sorted(JS))
def test_solve_matches_reference_javascript(monkeypatch, name, wgs):
    c = _cfd()
    _set_wgs(monkeypatch, wgs)
    meta = JS[name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    nx, ny = meta["nx"], meta["ny"]
    n = int(fx["iters_run"][0])
    # the script always tests its tolerance; a fixture that never meets it is
    # also the fixed-count solve
    for tol in ([True] if n < meta["iterations"] else [True, False]):
        m = c.Model(c.Grid(nx, ny, meta["lx"], meta["ly"]),
                    c.SimulationParams(pressure_solver=c.PressureSolver.SorLex,
                                       jacobi_iters=meta["iterations"], tol_enabled=tol, p_tol=1e-4))
        m.set_state(rhs=fx["in_rhs"], p_prime=np.full(nx * ny, 7.0, np.float32))
        r = m.pressure_solve()
        st = m.get_state()
        assert_bitwise(f"{name} wgs={wgs} tol={tol}: p'", st["p_prime"], fx["out_solve"])
        assert np.float32(r) == np.float32(fx["out_residual_f64"][0])
        assert st["jacobi_sweeps_total"] == n
        m.close()


_REF = {}


def _restated(nx, ny, lx, ly, iters, scale):
    """(rhs, p', iterations run, maxError list) of the anti-diagonal form with
    the tolerance on, computed once per shape; the fixed-count result is the
    same when the tolerance is never met (asserted by the caller)."""
    key = (nx, ny, lx, ly, iters, scale)
    if key not in _REF:
        rng = np.random.default_rng([nx, ny, iters])
        rhs = (rng.uniform(-1, 1, nx * ny) * scale).astype(np.float32)
        dx, dy = np.float32(lx) / np.float32(nx), np.float32(ly) / np.float32(ny)
        _REF[key] = (rhs,) + ref.sor_lex_diag(rhs, nx, ny, dx, dy, iters, True, 1e-4)
    return _REF[key]


@pytest.mark.parametrize("tol", [False, True])
@pytest.mark.parametrize("nx,ny,lx,ly,iters", [(800, 264, 30.0, 10.0, 50), (264, 150, 2.64, 1.5, 33)])
def test_solve_matches_restatement_on_larger_grids(nx, ny, lx, ly, iters, tol):
    """The default channel (five bands, the last one 6 rows) and a grid with a
    ragged last band; rhs of the size a step forms, so the tolerance is never
    met and one restatement serves both modes."""
    c = _cfd()
    rhs, want, n, errs = _restated(nx, ny, lx, ly, iters, 100.0)
    assert n == iters and not ref.slivers(errs)
    m = c.Model(c.Grid(nx, ny, lx, ly),
                c.SimulationParams(pressure_solver=c.PressureSolver.SorLex, jacobi_iters=iters,
                                   tol_enabled=tol, p_tol=1e-4))
    m.set_state(rhs=rhs, p_prime=np.full(nx * ny, 7.0, np.float32))
    r = m.pressure_solve()
    st = m.get_state()
    assert_bitwise(f"{nx}x{ny} tol={tol}: p'", st["p_prime"], want.reshape(-1))
    assert np.float32(r) == np.float32(errs[-1])
    assert st["jacobi_sweeps_total"] == n


def _developed_state(c, grid):
    m = c.Model(grid, c.SimulationParams(jacobi_iters=20, corrector_passes=0, tol_enabled=False))
    m.update_n(4)
    st = m.get_state()
    m.close()
    return {f: st[f] for f in FIELDS7}


def _phases_with_solve(c, m, dt, solve):
    """The phases piso_step runs with corrector_passes 0, the pressure solve
    replaced by solve(rhs) -> p'."""
    for ph in (0, 1, 2):   # u predictor, v predictor, divergence
        m.run_phase(ph, dt)
    m.set_state(p_prime=solve(m.get_state()["rhs"]))
    for ph in (3, 4):      # corrector, boundary
        m.run_phase(ph, dt)


@pytest.mark.parametrize("tol", [False, True])
def test_piso_step_matches_phases_around_the_restatement(tol):
    c = _cfd()
    import oracle
    nx, ny, lx, ly, iters, dt = 128, 64, 30.0, 10.0, 12, 0.004
    grid = c.Grid(nx, ny, lx, ly, c.Cylinder(7.5, 5.0, 0.75))
    dx, dy = np.float32(lx) / np.float32(nx), np.float32(ly) / np.float32(ny)
    st0 = _developed_state(c, grid)

    def params(solver):
        return c.SimulationParams(pressure_solver=c.PressureSolver(solver), jacobi_iters=iters,
                                  corrector_passes=0, tol_enabled=tol, p_tol=1e-4)

    def sor_rb(rhs):
        want = np.empty(nx * ny, np.float32)
        oracle.sor_solve(want, rhs, nx, ny, dx, dy, iters, tol, 1e-4)
        return want

    def sor_lex(rhs):
        return ref.sor_lex_diag(rhs, nx, ny, dx, dy, iters, tol, 1e-4)[0].reshape(-1)

    # control: the composition reproduces piso_step for solver 1 with its own oracle solve
    for solver, solve in ((1, sor_rb), (4, sor_lex)):
        a = c.Model(grid, params(solver))
        a.set_state(**st0)
        a.piso_step(dt)
        b = c.Model(grid, params(1))
        b.set_state(**st0)
        _phases_with_solve(c, b, dt, solve)
        sa, sb = a.get_state(), b.get_state()
        for f in FIELDS7:
            assert_bitwise(f"solver {solver} tol={tol}: {f}", sa[f], sb[f])
        a.close()
        b.close()


def test_update_steps_identical_at_every_workgroup_cap(monkeypatch):
    c = _cfd()
    grid = c.Grid(128, 64, 30.0, 10.0, c.Cylinder(7.5, 5.0, 0.75))
    out = {}
    for wgs in ("default", "1"):
        _set_wgs(monkeypatch, wgs)
        m = c.Model(grid, c.SimulationParams(pressure_solver=c.PressureSolver.SorLex))   # reference knobs
        sweeps = 0
        for _ in range(5):
            m.update()
            s = m.get_residuals().jacobi_sweeps_total
            assert s > sweeps
            sweeps = s
        st = m.get_state()
        for f in FIELDS7:
            assert np.all(np.isfinite(st[f])), f
        out[wgs] = (st, sweeps)
        m.close()
    assert out["default"][1] == out["1"][1]
    for f in FIELDS7:
        assert_bitwise(f"update x5 default vs 1 workgroup: {f}", out["default"][0][f], out["1"][0][f])


def test_switching_solvers_mid_run():
    """0 -> 4 -> 1 -> 4 through set_parameters; every solver-4 step's p' is the
    restatement of that step's rhs (corrector_passes 0: the step's only solve)."""
    c = _cfd()
    nx, ny, lx, ly, iters = 64, 48, 3.0, 2.0, 15
    dx, dy = np.float32(lx) / np.float32(nx), np.float32(ly) / np.float32(ny)
    m = c.Model(c.Grid(nx, ny, lx, ly, c.Cylinder(1.0, 1.0, 0.3)), c.SimulationParams())
    for solver in (0, 4, 1, 4):
        m.set_parameters(c.SimulationParams(pressure_solver=c.PressureSolver(solver),
                                            jacobi_iters=iters, corrector_passes=0))
        for _ in range(2):
            before = m.get_residuals().jacobi_sweeps_total
            m.update()
            if solver != 4:
                continue
            st = m.get_state()
            want, n, errs = ref.sor_lex_diag(st["rhs"], nx, ny, dx, dy, iters, True, 1e-4)
            assert_bitwise("p' of a solver-4 step", st["p_prime"], want.reshape(-1))
            r = m.get_residuals()
            assert np.float32(r.p) == np.float32(errs[-1])
            assert r.jacobi_sweeps_total - before == n
