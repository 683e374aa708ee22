"""GPU: pressure_solver 5, the JavaScript variant's default solver -- Jacobi
with omega 0.7 (index.html:796-838; cfd_jacobi_script.hip), bit for bit

* against the reference script itself, executed by node on the same inputs
  (tests/golden/js_jac_*.npz, make_js_jacobi_golden.py): every tile seam of the
  kernel, both ping-pong parities of the early exit, rhs = 0, one iteration;
* inside the script's substep, against node's own pisoStep with that solver
  (tests/golden/js_jacstep_*.npz);
* against the restatement (tests/_jacobi_script_ref.py, pinned to the same
  fixtures by test_script_update_cpu.py) on the default 800 x 264 channel;
* inside Model::update and across solver switches.
"""
import json
import os

import numpy as np
import pytest

import _jacobi_script_ref as ref
from _util import assert_bitwise

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
JS = json.load(open(os.path.join(GOLD, "js_jac_manifest.json")))
P_TOL = JS["p_tol"]
JS = JS["fixtures"]
JSTEP = json.load(open(os.path.join(GOLD, "js_jacstep_manifest.json")))
FIELDS7 = ("u", "v", "p", "u_star", "v_star", "p_prime", "rhs")


def _cfd():
    import cfdamd
    return cfdamd


@pytest.mark.parametrize("name", sorted(JS))
def test_solve_matches_reference_javascript(name):
    c = _cfd()
    meta = JS[name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    nx, ny = meta["nx"], meta["ny"]
    n = int(fx["iters_run"][0])
    errs = fx["max_errors_f64"]
    assert len(errs) == n
    # the script always tests its tolerance; a fixture that never meets it is
    # also the fixed-count solve
    for tol in ([True] if n < meta["iterations"] else [True, False]):
        m = c.Model(c.Grid(nx, ny, meta["lx"], meta["ly"]),
                    c.SimulationParams(pressure_solver=c.PressureSolver.JacobiScript,
                                       jacobi_iters=meta["iterations"], tol_enabled=tol, p_tol=P_TOL))
        # both p' buffers hold junk: the solve restarts from 0 and writes every cell
        m.set_state(rhs=fx["in_rhs"], p_prime=np.full(nx * ny, 7.0, np.float32))
        before = m.get_state()["jacobi_sweeps_total"]
        r = m.pressure_solve()
        st = m.get_state()
        assert_bitwise(f"{name} tol={tol}: p'", st["p_prime"], fx["out_solve"])
        assert np.float32(r) == np.float32(errs[-1])
        assert st["jacobi_sweeps_total"] - before == n
        # a second solve from the other buffer parity gives the same bits
        r2 = m.pressure_solve()
        st2 = m.get_state()
        assert_bitwise(f"{name} tol={tol}: p' of a second solve", st2["p_prime"], fx["out_solve"])
        assert np.float32(r2) == np.float32(errs[-1])
        assert st2["jacobi_sweeps_total"] - before == 2 * n
        m.close()


@pytest.mark.parametrize("name", sorted(JSTEP["fixtures"]))
def test_script_substep_matches_reference_javascript(name):
    """pisoStep(dt_sub) of the script with its default solver, through
    script_piso_step; lastPResidual lands in last_p_residual."""
    c = _cfd()
    meta = JSTEP["fixtures"][name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    cyl = c.Cylinder(*meta["cylinder"]) if meta["cylinder"] else None
    m = c.Model(c.Grid(meta["nx"], meta["ny"], meta["lx"], meta["ly"], cyl),
                c.SimulationParams(viscosity=JSTEP["viscosity"],
                                   pressure_solver=c.PressureSolver.JacobiScript,
                                   jacobi_iters=JSTEP["iters"], tol_enabled=True, p_tol=JSTEP["p_tol"]))
    m.set_state(u=fx["in_u"].ravel(), v=fx["in_v"].ravel(), p=fx["in_p"].ravel())
    m.script_piso_step(meta["dt_sub"], c.ScriptScheme(meta["scheme"]), meta["inlet_velocity"],
                       c.InletProfile(meta["profile"]))
    st = m.get_state()
    for f in FIELDS7:
        assert_bitwise(f"{name}: {f}", st[f], fx[f].ravel())
    assert np.float32(st["last_p_residual"]) == np.float32(fx["lastPResidual"][0])
    assert st["jacobi_sweeps_total"] == meta["iterations_run"]
    m.close()


@pytest.mark.parametrize("tol", [False, True])
def test_default_channel_matches_restatement(tol):
    """800 x 264: seven wave columns, 66 row segments in 17 workgroup rows (the
    last one half empty); rhs of the size a step forms, so the tolerance is
    never met and one restatement serves both modes."""
    c = _cfd()
    nx, ny, lx, ly, iters = 800, 264, 30.0, 10.0, 9
    rng = np.random.default_rng([nx, ny, iters])
    rhs = (rng.uniform(-1, 1, nx * ny) * 100.0).astype(np.float32)
    dx, dy = np.float32(lx) / np.float32(nx), np.float32(ly) / np.float32(ny)
    want, n, errs = ref.jacobi_script(rhs, nx, ny, dx, dy, iters, True, P_TOL)
    assert n == iters and not ref.slivers(errs)
    m = c.Model(c.Grid(nx, ny, lx, ly),
                c.SimulationParams(pressure_solver=c.PressureSolver.JacobiScript, jacobi_iters=iters,
                                   tol_enabled=tol, p_tol=P_TOL))
    m.set_state(rhs=rhs, p_prime=np.full(nx * ny, 7.0, np.float32))
    r = m.pressure_solve()
    st = m.get_state()
    assert_bitwise(f"800x264 tol={tol}: p'", st["p_prime"], want.reshape(-1))
    assert np.float32(r) == np.float32(errs[-1])
    assert st["jacobi_sweeps_total"] == n
    m.close()


def test_update_runs_and_repeats():
    """Model::update with solver 5 (reference knobs: corrector passes included);
    two runs give the same bits."""
    c = _cfd()
    grid = c.Grid(128, 64, 30.0, 10.0, c.Cylinder(7.5, 5.0, 0.75))
    out = []
    for _ in range(2):
        m = c.Model(grid, c.SimulationParams(pressure_solver=c.PressureSolver.JacobiScript))
        sweeps = 0
        for _ in range(4):
            m.update()
            s = m.get_residuals().jacobi_sweeps_total
            assert s > sweeps
            sweeps = s
        st = m.get_state()
        for f in FIELDS7:
            assert np.all(np.isfinite(st[f])), f
        out.append((st, sweeps))
        m.close()
    assert out[0][1] == out[1][1]
    for f in FIELDS7:
        assert_bitwise(f"update x4, run 1 vs run 2: {f}", out[0][0][f], out[1][0][f])


def test_switching_solvers_mid_run():
    """5 -> 0 -> 5 through set_parameters; every solver-5 step's p' is the
    restatement of that step's rhs (corrector_passes 0: the step's only solve)."""
    c = _cfd()
    nx, ny, lx, ly, iters = 64, 48, 3.0, 2.0, 15
    dx, dy = np.float32(lx) / np.float32(nx), np.float32(ly) / np.float32(ny)
    m = c.Model(c.Grid(nx, ny, lx, ly, c.Cylinder(1.0, 1.0, 0.3)), c.SimulationParams())
    for solver in (5, 0, 5):
        m.set_parameters(c.SimulationParams(pressure_solver=c.PressureSolver(solver),
                                            jacobi_iters=iters, corrector_passes=0))
        for _ in range(2):
            before = m.get_residuals().jacobi_sweeps_total
            m.update()
            if solver != 5:
                continue
            st = m.get_state()
            want, n, errs = ref.jacobi_script(st["rhs"], nx, ny, dx, dy, iters, True, 1e-4)
            assert_bitwise("p' of a solver-5 step", st["p_prime"], want.reshape(-1))
            r = m.get_residuals()
            assert np.float32(r.p) == np.float32(errs[-1])
            assert r.jacobi_sweeps_total - before == n
    m.close()
