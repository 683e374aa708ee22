"""Golden vectors for the script's substep with its DEFAULT pressure solver (the
Jacobi branch, pressure_solver 5), produced by the reference's OWN JavaScript
(test infrastructure).

Everything is make_js_script_step_golden.py's -- its extraction of pisoStep and
applyBoundaryConditions from the reference at generation time, its node harness
(a `new Function` whose parameters are the script's globals), its seeded inputs
and its checks of the restatement against node -- with currentPressureSolver set
to a value that falls through to the script's Jacobi branch (index.html:796).
Only numbers are stored, as tests/golden/js_jacstep_*.npz plus a manifest; no
reference source is written to the repository.

The generator asserts, per fixture, that tests/_script_step_ref.py equals node
bit for bit around the solve, that tests/_jacobi_script_ref.py reproduces node's
p_prime from node's rhs and its lastPResidual, and that no iteration's maxError
lies in the sliver below 1e-6 where the script's double test and the library's
float test differ.

    python tests/golden/make_js_jacobi_step_golden.py

Only fixtures whose .npz is missing are generated; the seed of a case is
7171 + its position in CASES.
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _jacobi_script_ref as jac              # noqa: E402
import _script_step_ref as ref                # noqa: E402
import make_js_script_step_golden as step     # noqa: E402

step.SOLVER_NAMES = {**step.SOLVER_NAMES, 5: "jacobi"}   # pressureSolverSelect's default value
ITERS, P_TOL, NU = step.ITERS, jac.P_TOL, step.NU

# name -> (nx, ny, lx, ly, cylinder, scheme, profile, inlet velocity, dt_sub, cfl)
CASES = {
    "js_jacstep_24x7_second_p2": (24, 7, 24 / 128.0, 7 / 128.0, None, 1, 0, 0.5, 0.001, 0.5),
    "js_jacstep_40x12_cyl_quick": (40, 12, 30.0, 10.0, (7.5, 5.0, 2.0), 2, 1, 1.5, 0.05, 0.7),
    # nx = 136: the solve's wave seam in x; 20 rows: its workgroup seam in y
    "js_jacstep_136x20_cyl_first": (136, 20, 30.0, 10.0, (7.5, 5.0, 1.75), 0, 0, 1.5, 0.02, 0.7),
}


def main():
    text = step.extract()
    assert "jacobiOmega = 0.7" in text
    mpath = os.path.join(HERE, "js_jacstep_manifest.json")
    if os.path.exists(mpath):
        manifest = json.load(open(mpath))
    else:
        manifest = {"generator": "tests/golden/make_js_jacobi_step_golden.py",
                    "source": "reference index.html:366-867 (pisoStep, Jacobi branch :796-838), "
                              ":870-930, :212-215, :181-184, executed by node " +
                              subprocess.run(["node", "--version"], capture_output=True,
                                             text=True).stdout.strip(),
                    "iters": ITERS, "p_tol": P_TOL, "viscosity": NU, "fixtures": {}}
    for k, (name, case) in enumerate(CASES.items()):
        nx, ny, lx, ly, cyl, scheme, profile, inlet, dt_sub, cfl = case
        if os.path.exists(os.path.join(HERE, name + ".npz")):
            assert name in manifest["fixtures"], f"{name}.npz has no manifest entry"
            print(name, "kept")
            continue
        g = ref.Grid(nx, ny, lx, ly, NU, cyl)
        dt_sub = float(np.float32(dt_sub))
        inlet = float(np.float32(inlet))
        rng = np.random.default_rng(7171 + k)
        u, v, p = step.make_inputs(g, rng, dt_sub, cfl)
        node = step.run_node(text, g, u, v, p, scheme, 5, profile, inlet, dt_sub)
        step.check_host_data(name, g, node, profile, inlet)
        us, vs, rhs = ref.predict(g, u, v, dt_sub, scheme)
        for nm, a in (("u_star", us), ("v_star", vs), ("rhs", rhs)):
            assert ref.bits_equal(a, node[nm]), (name, nm)
        pp, n_run, errs = jac.jacobi_script(node["rhs"], nx, ny, g.dx, g.dy, ITERS, True, P_TOL)
        assert not jac.slivers(errs), (name, "maxError in the sliver below 1e-6")
        assert ref.bits_equal(pp, node["p_prime"]), (name, "p_prime vs _jacobi_script_ref")
        assert errs[-1] == float(node["lastPResidual"][0]), (name, "lastPResidual")
        un, vn, pn = ref.correct(g, node["u_star"], node["v_star"], node["p_prime"], p, dt_sub,
                                 inlet, profile)
        for nm, a in (("u", un), ("v", vn), ("p", pn)):
            assert ref.bits_equal(a, node[nm]), (name, nm)
            assert np.isfinite(node[nm]).all(), (name, nm, "non-finite")
        np.savez_compressed(os.path.join(HERE, name + ".npz"), in_u=u, in_v=v, in_p=p,
                            **{nm: node[nm] for nm in ("u_star", "v_star", "rhs", "p_prime", "u",
                                                       "v", "p", "lastPResidual")})
        manifest["fixtures"][name] = {
            "nx": nx, "ny": ny, "lx": lx, "ly": ly, "cylinder": list(cyl) if cyl else None,
            "scheme": scheme, "solver": 5, "profile": profile, "inlet_velocity": inlet,
            "dt_sub": dt_sub, "seed": 7171 + k, "iterations_run": n_run}
        json.dump(manifest, open(mpath, "w"), indent=1)
        print(name, "residual", float(node["lastPResidual"][0]), "iterations", n_run)


if __name__ == "__main__":
    sys.exit(main())
