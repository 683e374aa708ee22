"""numpy restatement of the script's time step with the double pressure
residual and the page's residualScalingEnabled branch (index.html:338-348), for
cfd_script_update under cfd_script_options.

The fields, the residuals and maxVel of a step are tests/_script_update_ref.py's
(its `update` is called unchanged: none of them depends on the decisions it
takes afterwards).  What differs is decided here, from the script's double
maxPressureResidual (`residual_p_f64` of that report): errorNorm and the
substep rule (:310-317), and the dt rule, which with scaling on is

    dt_pressure = dt_cfl
    if maxP > 1e-3: dt_pressure = dt_cfl * (1e-3 / (maxP + 1e-10))
    newDt = min(dt_cfl, dt_pressure)

before the unchanged 1.1 x previous dt limit.  Every scalar is a Python float,
a C double, JavaScript's number.

`update` returns the new state and a report whose `residual_p` is the double,
with `branches` (scale_idle, scale_accepted, scale_limited, scale_maxvel_zero
on top of the substep branches) and, for the fixture conditions,
`dt_unscaled` (the rule without the branch) and `dt_from_f32` (the scaled rule
evaluated on (double)(float)maxP).
"""
import math

import numpy as np

import _jacobi_script_ref as jac
import _script_step_ref as step
import _script_update_ref as upd
import _sor_lex_ref as sor

PRESSURE_TOL = 1e-3


def dt_rule(res_p, max_vel, dt, dt_user, g, scaling, branches=None):
    """computeAutomaticTimeStep (:1322-1342), :337-350 and :352-357 -> next dt."""
    def hit(b):
        if branches is not None:
            branches.append(b)
    if max_vel == 0:
        dt_cfl = dt_user
    else:
        dt_cfl = min(0.5 * min(g.dx, g.dy) / max_vel, dt_user)
    new_dt = dt_cfl
    scaled = False
    if scaling:
        dt_pressure = dt_cfl
        if res_p > PRESSURE_TOL:
            dt_pressure = dt_cfl * (PRESSURE_TOL / (res_p + 1e-10))
            scaled = True
        new_dt = min(dt_cfl, dt_pressure)
    limited = False
    if new_dt > dt:
        lim = dt * 1.1
        limited = lim < new_dt
        new_dt = min(new_dt, lim)
    if scaling:
        if max_vel == 0:
            hit("scale_maxvel_zero")
        if not scaled:
            hit("scale_idle")
        elif limited:
            hit("scale_limited")
        else:
            hit("scale_accepted")
    return new_dt


def substep_rule(substep_count, res_u, res_v, res_p):
    """:310-317 -> next substepCount."""
    error_norm = max(res_u, res_v, res_p)
    tolerance = 1e-3
    if error_norm > tolerance:
        want = substep_count * (error_norm / tolerance)
        want = math.ceil(want) if math.isfinite(want) else want
        return int(min(want, 20))
    if error_norm < tolerance / 10 and substep_count > 1:
        return max(math.floor(substep_count / 2), 1)
    return substep_count


def update(g, st, scheme, profile, target, dt_user, solver, scaling=True):
    """One updateSimulation() decided from the double residual.  st as
    _script_update_ref.update takes it."""
    dt = float(st["dt"]) if st.get("dt") else float(dt_user)
    nsub = int(st["substep_count"])
    new, rep = upd.update(g, st, scheme, profile, target, dt_user, solver)
    ru, rv, rp, mv = rep["residual_u"], rep["residual_v"], rep["residual_p_f64"], rep["max_vel"]
    branches = []
    nxt = substep_rule(nsub, ru, rv, rp)
    new_dt = dt_rule(rp, mv, dt, float(dt_user), g, scaling, branches)
    new = dict(new, dt=new_dt, substep_count=nxt)
    report = dict(step_count=rep["step_count"], substeps_run=nsub, substep_count_next=nxt,
                  residual_u=ru, residual_v=rv, residual_p=rp, dt_next=new_dt,
                  inlet_velocity=rep["inlet_velocity"], max_vel=mv, branches=branches,
                  dt_unscaled=dt_rule(rp, mv, dt, float(dt_user), g, False),
                  dt_from_f32=dt_rule(float(np.float32(rp)), mv, dt, float(dt_user), g, scaling))
    return new, report


def solve_slivers(g, st, scheme, profile, target, dt_user, solver):
    """Iterations of the step's solves whose exit test differs between the
    library's (float)maxError < (float)p_tol and the script's double comparison
    (the solve-level caveat zone; the multigrid has no exit test).  The same
    walk as _script_update_ref.update."""
    if solver == 2:
        return []
    nx, ny = g.nx, g.ny
    u = np.asarray(st["u"], np.float32).reshape(ny, nx + 1)
    v = np.asarray(st["v"], np.float32).reshape(ny + 1, nx)
    p = np.asarray(st["p"], np.float32).reshape(ny, nx)
    dt = float(st["dt"]) if st.get("dt") else float(dt_user)
    n, nsub = int(st["step_count"]), int(st["substep_count"])
    with np.errstate(all="ignore"):
        if n > 0:
            u = (2 * u.astype(np.float64) - np.asarray(st["u_prev"], np.float32).reshape(u.shape).astype(np.float64)).astype(np.float32)
            v = (2 * v.astype(np.float64) - np.asarray(st["v_prev"], np.float32).reshape(v.shape).astype(np.float64)).astype(np.float32)
    inlet = (n / upd.RAMP_UP_STEPS) * float(target) if n < upd.RAMP_UP_STEPS else float(target)
    p_tol = upd.P_TOL[solver]
    bad = []
    for sub in range(nsub):
        us, vs, rhs = step.predict(g, u, v, dt / nsub, scheme)
        if solver == 4:
            pp, _, errs = sor.sor_lex_diag(rhs, nx, ny, g.dx, g.dy, upd.ITERS, True, p_tol)
        else:
            pp, _, errs = jac.jacobi_script(rhs, nx, ny, g.dx, g.dy, upd.ITERS, True, p_tol)
        bad += [(sub, k) for k in jac.slivers(errs, p_tol)]
        u, v, p = step.correct(g, us, vs, pp, p, dt / nsub, inlet, profile)
    return bad
