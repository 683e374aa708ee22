#!/usr/bin/env python3
"""The script's time step on the device against the host-driven route, on the
default 800 x 264 channel developed for a few hundred steps.

    python tools/bench_script_update.py [DEVELOP_STEPS] [TIMED_STEPS] [REPEATS]

(a) ms per `script_update` per solver (2 multigrid, 4 script-order SOR, 5 the
    script's Jacobi) against the only route there was before it: a Python loop
    around `script_piso_step` that extrapolates, forms the residuals and the CFL
    maximum in numpy through `get_state` / `set_state` and applies the script's
    rules on the host.  Both routes run the same steps from the same state (the
    host route's decisions are the device route's: asserted), wall clock around
    a synchronised batch, best and worst of REPEATS.
(b) us per iteration of the solver-5 kernel beside the red-black SOR's
    `k_sor_march` on the same grid: `pressure_solve` with a fixed count of 400
    iterations, wall clock over the solve divided by the count (launch gaps
    included; the per-kernel means come from running this tool under
    `rocprofv3 --kernel-trace --stats`).
(c) the share of a step spent in the begin and end passes is read from the same
    kernel trace: k_script_begin + k_script_end + k_script_pmax over the sum of
    all kernels between them.

Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cfd-demo_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cfdamd as c   # noqa: E402
import _script_step_ref as step   # noqa: E402
import _script_update_ref as upd   # noqa: E402

NU, TARGET, DT_USER = 0.01, 1.0, 0.5
SCHEME, PROFILE = c.ScriptScheme.Quick, c.InletProfile.Parabolic
P_TOL = {2: 1e-4, 4: 1e-4, 5: 1e-6}


def model(solver, **kw):
    p = dict(viscosity=NU, pressure_solver=c.PressureSolver(solver), jacobi_iters=50, tol_enabled=True,
             p_tol=P_TOL.get(solver, 1e-4))
    p.update(kw)
    return c.Model(c.default_grid(), c.SimulationParams(**p))


def host_route(m, g, ss, n):
    """n steps of updateSimulation driven from Python around script_piso_step."""
    reports = []
    for _ in range(n):
        st = m.get_state()
        u, v = st["u"], st["v"]
        if ss["step_count"] > 0:
            u = (2 * u.astype(np.float64) - ss["u_prev"].astype(np.float64)).astype(np.float32)
            v = (2 * v.astype(np.float64) - ss["v_prev"].astype(np.float64)).astype(np.float32)
            m.set_state(u=u, v=v)
        u_old, v_old = u, v
        k = ss["step_count"]
        inlet = (k / 1000) * TARGET if k < 1000 else TARGET
        dt_sub = ss["dt"] / ss["substep_count"]
        max_p = 0.0
        for _ in range(ss["substep_count"]):
            m.script_piso_step(dt_sub, SCHEME, inlet, PROFILE)
            max_p = max(max_p, float(m.get_residuals().p))
        st = m.get_state()
        u, v = st["u"], st["v"]
        res_u = float(np.abs(u.astype(np.float64) - u_old).max())
        res_v = float(np.abs(v.astype(np.float64) - v_old).max())
        max_vel = float(max(np.abs(u).max(), np.abs(v).max()))
        nxt, dt = upd.decisions(ss["substep_count"], res_u, res_v, max_p, max_vel, ss["dt"], DT_USER, g)
        ss = dict(u_prev=u, v_prev=v, dt=dt, substep_count=nxt, step_count=k + 1)
        reports.append((nxt, dt))
    return ss, reports


def main():
    develop = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    timed = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    grid = c.default_grid()
    g = step.Grid(grid.nx, grid.ny, grid.lx, grid.ly, NU,
                  (grid.obstacle.center_x, grid.obstacle.center_y, grid.obstacle.radius))
    out = {"grid": [grid.nx, grid.ny], "develop_steps": develop, "timed_steps": timed, "update_ms": {}}
    for solver in (2, 4, 5):
        m = model(solver)
        m.script_begin()
        m.script_update_n(develop, SCHEME, TARGET, DT_USER, PROFILE)
        st0, ss0 = m.get_state(), m.script_state()
        dev, host = [], []
        for _ in range(repeats):
            m.set_state(u=st0["u"], v=st0["v"], p=st0["p"])
            m.script_begin(ss0)
            m.synchronize()
            t0 = time.perf_counter()
            reps = m.script_update_n(timed, SCHEME, TARGET, DT_USER, PROFILE)
            m.synchronize()
            dev.append((time.perf_counter() - t0) / timed * 1e3)
            m.set_state(u=st0["u"], v=st0["v"], p=st0["p"])
            m.synchronize()
            t0 = time.perf_counter()
            _, hreps = host_route(m, g, dict(ss0), timed)
            m.synchronize()
            host.append((time.perf_counter() - t0) / timed * 1e3)
            assert hreps == [(r.substep_count_next, r.dt_next) for r in reps], "the two routes diverged"
        out["update_ms"][str(solver)] = {
            "device": [min(dev), max(dev)], "host_route": [min(host), max(host)],
            "ratio_best": min(host) / min(dev), "substeps": [r.substeps_run for r in reps]}
        m.close()
    iters = 400
    rng = np.random.default_rng(3)
    rhs = (rng.uniform(-1, 1, grid.nx * grid.ny) * 100).astype(np.float32)
    out["iteration_us"] = {}
    for solver in (5, 1):
        m = model(solver, jacobi_iters=iters, tol_enabled=False)
        m.set_state(rhs=rhs)
        m.pressure_solve()
        ts = []
        for _ in range(max(repeats, 3)):
            m.synchronize()
            t0 = time.perf_counter()
            m.pressure_solve()
            ts.append((time.perf_counter() - t0) / iters * 1e6)
        out["iteration_us"][str(solver)] = [min(ts), max(ts)]
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
