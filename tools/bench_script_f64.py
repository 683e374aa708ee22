#!/usr/bin/env python3
"""What the double pressure residual costs a script update
(cfd_script_options.residual_f64), on tools/bench_script_update.py's shape: the
default 800 x 264 channel developed for a few hundred steps, then batches of
`script_update` per solver (2 multigrid, 4 script-order SOR, 5 the script's
Jacobi) from the same state with the option off and on.

    python tools/bench_script_f64.py [DEVELOP_STEPS] [TIMED_STEPS] [BATCHES]

Wall clock around a synchronised batch, ms per update, every batch listed (the
spread of the batches is the yardstick for the on/off ratio).  The two routes
run the same steps unless the f32 rounding moves a substep decision
(`same_decisions` says whether it did).  `spread_off` / `spread_on` are
(worst - best) / best of a mode's batches, the yardstick beside which
`ratio_best` (best on / best off) and `ratio_mean` are read.

The parent commit's figure comes from the same tool with CFD_LIB pointing at a
library built from the parent commit (cfdamd loads that file in place of the
tree's, and tolerates the symbols it lacks): such a library has no
cfd_script_set_options and is timed with the option off only.

Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cfd-demo_amd"))
import cfdamd as c   # noqa: E402
from cfdamd import _lib   # noqa: E402

NU, TARGET, DT_USER = 0.01, 1.0, 0.5
SCHEME, PROFILE = c.ScriptScheme.Quick, c.InletProfile.Parabolic
P_TOL = {2: 1e-4, 4: 1e-4, 5: 1e-6}


def main():
    develop = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    timed = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    batches = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    has_option = hasattr(_lib.load(), "cfd_script_set_options")
    grid = c.default_grid()
    out = {"grid": [grid.nx, grid.ny], "develop_steps": develop, "timed_steps": timed, "update_ms": {}}
    for solver in (2, 4, 5):
        m = c.Model(grid, c.SimulationParams(viscosity=NU, pressure_solver=c.PressureSolver(solver),
                                             jacobi_iters=50, tol_enabled=True, p_tol=P_TOL[solver]))
        m.script_begin()
        m.script_update_n(develop, SCHEME, TARGET, DT_USER, PROFILE)
        st0, ss0 = m.get_state(), m.script_state()
        ms = {"off": [], "on": []}
        decisions = {}
        for _ in range(batches):
            for mode in ("off", "on") if has_option else ("off",):
                if has_option:
                    m.script_options(residual_f64=(mode == "on"), residual_scaling=False)
                m.set_state(u=st0["u"], v=st0["v"], p=st0["p"])
                m.script_begin(ss0)
                m.synchronize()
                t0 = time.perf_counter()
                reps = m.script_update_n(timed, SCHEME, TARGET, DT_USER, PROFILE)
                m.synchronize()
                ms[mode].append((time.perf_counter() - t0) / timed * 1e3)
                decisions[mode] = [(r.substeps_run, r.substep_count_next, r.dt_next) for r in reps]
        def spread(x):
            return (max(x) - min(x)) / min(x)
        rec = {"off": ms["off"], "spread_off": spread(ms["off"]),
               "substeps": [d[0] for d in decisions["off"]]}
        if has_option:
            rec.update(on=ms["on"], spread_on=spread(ms["on"]),
                       ratio_best=min(ms["on"]) / min(ms["off"]),
                       ratio_mean=sum(ms["on"]) / sum(ms["off"]),
                       same_decisions=decisions["on"] == decisions["off"])
        out["update_ms"][str(solver)] = rec
        m.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
