"""numpy restatement of the script's time step: updateSimulation()
(index.html:261-363) with computeAutomaticTimeStep (:1322-1342), for
cfd_script_update.

The substep is tests/_script_step_ref.py's (predict / correct) around one of
the three solves pinned to the script: 2 the multigrid (the C oracle's
mg_solve, pinned to node by tests/test_oracle_solvers.py), 4 the script-order
SOR (tests/_sor_lex_ref.py), 5 the script's Jacobi
(tests/_jacobi_script_ref.py).  Every scalar is a Python float, i.e. a C
double, JavaScript's number.

`update` returns the new state and a report that holds BOTH residual
conventions: `residual_p_f64`, the script's double maximum, and `residual_p`,
the library's (double)(float) of it, with the substep and dt decisions taken
from the latter; `script_decisions` are those the script's own double gives
(tests/golden/make_js_update_golden.py asserts the two equal on every step of
every fixture).  `branches` names the branches the step took; `dt_is_cfl`
marks the steps whose new dt IS the CFL quotient 0.5 min(dx, dy) / maxVel (below dt_user and not cut
by the 1.1 limit), the only steps where maxVel reaches a result by value, with
`cfl_from_u` / `cfl_from_v` for the array that held the maximum.
"""
import math

import numpy as np

import _jacobi_script_ref as jac
import _script_step_ref as step
import _sor_lex_ref as sor

RAMP_UP_STEPS = 1000
ITERS = 50
P_TOL = {2: 1e-4, 4: 1e-4, 5: 1e-6}   # multigrid has no exit test; the library's default is kept


def solve(g, rhs, solver):
    """p' (ny, nx) f32 and the script's double lastPResidual."""
    nx, ny = g.nx, g.ny
    if solver == 4:
        pp, _, errs = sor.sor_lex_diag(rhs, nx, ny, g.dx, g.dy, ITERS, True, P_TOL[4])
        return pp, errs[-1]
    if solver == 5:
        pp, _, errs = jac.jacobi_script(rhs, nx, ny, g.dx, g.dy, ITERS, True, P_TOL[5])
        return pp, errs[-1]
    assert solver == 2
    import oracle
    pp = np.zeros(nx * ny, np.float32)
    rhs = np.ascontiguousarray(rhs, np.float32).reshape(-1)
    r32 = oracle.mg_solve(pp, rhs, nx, ny, np.float32(g.dx), np.float32(g.dy))
    # the oracle returns the float; the script's double is :784-794 on its p'
    D = pp.reshape(ny, nx).astype(np.float64)
    R = rhs.reshape(ny, nx).astype(np.float64)[1:-1, 1:-1]
    dx, dy = g.dx, g.dy
    denom_local = 2 / (dx * dx) + 2 / (dy * dy)
    with np.errstate(all="ignore"):
        r = np.abs((D[1:-1, 2:] + D[1:-1, :-2]) / (dx * dx) + (D[2:, 1:-1] + D[:-2, 1:-1]) / (dy * dy)
                   - denom_local * D[1:-1, 1:-1] - R)
    r = _max_ignoring_nan(r)
    assert np.float32(r) == np.float32(r32), "multigrid residual: restatement vs oracle"
    return pp.reshape(ny, nx), r


def _max_ignoring_nan(a):
    a = a[a > 0.0]
    return float(a.max()) if a.size else 0.0


def decisions(substep_count, res_u, res_v, res_p, max_vel, dt, dt_user, g, branches=None):
    """:310-317 and :333-357 -> (next substepCount, next dt)."""
    def hit(b):
        if branches is not None:
            branches.append(b)
    error_norm = max(res_u, res_v, res_p)
    tolerance = 1e-3
    nxt = substep_count
    if error_norm > tolerance:
        factor = error_norm / tolerance
        want = substep_count * factor
        want = math.ceil(want) if math.isfinite(want) else want
        nxt = int(min(want, 20))
        hit("sub_capped" if want >= 20 else "sub_grown")
    elif error_norm < tolerance / 10 and substep_count > 1:
        nxt = max(math.floor(substep_count / 2), 1)
        hit("sub_floored" if nxt == 1 else "sub_halved")
    else:
        hit("sub_unchanged")
    if max_vel == 0:
        dt_cfl = dt_user
        hit("maxvel_zero")
    else:
        dt_cfl = 0.5 * min(g.dx, g.dy) / max_vel
        hit("dt_user" if dt_user < dt_cfl else "dt_cfl")
        dt_cfl = min(dt_cfl, dt_user)
    new_dt = dt_cfl
    if new_dt > dt:
        lim = dt * 1.1
        if lim < new_dt:
            hit("dt_limited")
        new_dt = min(new_dt, lim)
    # the CFL quotient itself becomes dt: it is below dt_user and survives the
    # 1.1 limit (only then does max_vel reach the result by value)
    if max_vel != 0 and new_dt == 0.5 * min(g.dx, g.dy) / max_vel and new_dt < dt_user:
        hit("dt_is_cfl")
    return nxt, new_dt


def update(g, st, scheme, profile, target, dt_user, solver):
    """One updateSimulation().  st: dict u (ny, nx+1), v (ny+1, nx), p (ny, nx),
    u_prev, v_prev (f32), dt (0 / None: unset), substep_count, step_count."""
    nx, ny = g.nx, g.ny
    u = np.asarray(st["u"], np.float32).reshape(ny, nx + 1)
    v = np.asarray(st["v"], np.float32).reshape(ny + 1, nx)
    p = np.asarray(st["p"], np.float32).reshape(ny, nx)
    dt = float(st["dt"]) if st.get("dt") else float(dt_user)
    n = int(st["step_count"])
    nsub = int(st["substep_count"])
    branches = []
    with np.errstate(all="ignore"):
        if n > 0:
            u = (2 * u.astype(np.float64) - np.asarray(st["u_prev"], np.float32).reshape(u.shape).astype(np.float64)).astype(np.float32)
            v = (2 * v.astype(np.float64) - np.asarray(st["v_prev"], np.float32).reshape(v.shape).astype(np.float64)).astype(np.float32)
            branches.append("extrapolated")
        else:
            branches.append("step0")
    u_old, v_old = u.copy(), v.copy()
    if n < RAMP_UP_STEPS:
        inlet = (n / RAMP_UP_STEPS) * float(target)
        branches.append("ramp")
    else:
        inlet = float(target)
        branches.append("ramp_done")
    dt_sub = dt / nsub
    max_p = 0.0
    for _ in range(nsub):
        us, vs, rhs = step.predict(g, u, v, dt_sub, scheme)
        pp, res = solve(g, rhs, solver)
        u, v, p = step.correct(g, us, vs, pp, p, dt_sub, inlet, profile)
        if res > max_p:
            max_p = res
    with np.errstate(all="ignore"):
        res_u = _max_ignoring_nan(np.abs(u.astype(np.float64) - u_old.astype(np.float64)))
        res_v = _max_ignoring_nan(np.abs(v.astype(np.float64) - v_old.astype(np.float64)))
        max_abs_u = _max_ignoring_nan(np.abs(u.astype(np.float64)))
        max_abs_v = _max_ignoring_nan(np.abs(v.astype(np.float64)))
        max_vel = max(max_abs_u, max_abs_v)
    res_p32 = float(np.float32(max_p))
    nxt, new_dt = decisions(nsub, res_u, res_v, res_p32, max_vel, dt, float(dt_user), g, branches)
    if "dt_is_cfl" in branches:   # which array the maximum that became dt came from
        branches.append("cfl_from_v" if max_abs_v > max_abs_u else "cfl_from_u")
    new = dict(u=u, v=v, p=p, u_prev=u.copy(), v_prev=v.copy(), dt=new_dt, substep_count=nxt,
               step_count=n + 1)
    report = dict(step_count=n + 1, substeps_run=nsub, substep_count_next=nxt, residual_u=res_u,
                  residual_v=res_v, residual_p=res_p32, residual_p_f64=max_p, dt_next=new_dt,
                  inlet_velocity=inlet, max_vel=max_vel, branches=branches,
                  script_decisions=decisions(nsub, res_u, res_v, max_p, max_vel, dt, float(dt_user), g))
    return new, report
