#!/usr/bin/env python3
"""Kernel-time comparison of the script substep's two launches with the Rust
step's: run under `rocprofv3 --kernel-trace --stats -- python
tools/bench_script_step.py NX NY [REPS]` and read the per-kernel averages of
k_script_predict / k_predict_march and k_script_correct / k_correct_finish*.

The Rust legs are `update` steps of a second-order and a first-order model
(fixed 8-sweep Jacobi, no corrector passes: one march and one fused finish per
step); the script legs are `script_piso_step` with each scheme on a multigrid
model.  Same grid, same process.  Fields are a smooth channel flow plus noise,
so upwind sides vary.  Prints nothing a profile needs; the stats file is the
result."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cfd-demo_amd"))
import cfdamd   # noqa: E402


def main():
    nx, ny = int(sys.argv[1]), int(sys.argv[2])
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    lx, ly = (30.0, 10.0) if (nx, ny) == (800, 264) else (float(nx) / float(ny), 1.0)
    cyl = cfdamd.Cylinder(lx / 4, ly / 2, 0.075 * ly)
    grid = cfdamd.Grid(nx, ny, lx, ly, cyl)
    dt = 0.1 * grid.dx
    rng = np.random.default_rng(1)
    u = (1.0 + 0.5 * rng.uniform(-1, 1, (nx + 1) * ny)).astype(np.float32)
    v = (0.5 * rng.uniform(-1, 1, nx * (ny + 1))).astype(np.float32)
    for scheme in (cfdamd.VelocityScheme.SecondOrder, cfdamd.VelocityScheme.FirstOrder):
        m = cfdamd.Model(grid, cfdamd.SimulationParams(dt=dt, velocity_scheme=scheme, jacobi_iters=8,
                                                       corrector_passes=0, tol_enabled=False))
        m.set_state(u=u, v=v)
        m.update_n(reps)
        m.synchronize()
        m.close()
    m = cfdamd.Model(grid, cfdamd.SimulationParams(dt=dt, pressure_solver=cfdamd.PressureSolver.Multigrid))
    for scheme in cfdamd.ScriptScheme:
        m.set_state(u=u, v=v)
        for _ in range(reps):
            m.script_piso_step(dt, scheme, 1.0, cfdamd.InletProfile.Parabolic)
        m.synchronize()
    m.close()
    print(f"bench_script_step: {nx}x{ny}, {reps} repetitions per leg")


if __name__ == "__main__":
    main()
