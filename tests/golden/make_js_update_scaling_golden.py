"""Golden vectors for cfd_script_update with cfd_script_options.residual_scaling:
the reference's OWN JavaScript with residualScalingEnabled = true (test
infrastructure).

Everything make_js_update_golden.py does holds here -- the script's functions
are read from the reference at generation time and run under node, only
numbers are stored (tests/golden/js_update_scaling_*.npz and a manifest), no
reference source is written to the repository -- except that this harness
starts the page with the "residual scaling" checkbox ticked, so
updateSimulation takes :338-348 and dt follows the double pressure residual.

The .npz layout is make_js_update_golden.py's: the start state, per step res_u,
res_v, res_p (the script's doubles), substeps, dt and inlet, u / v / p after
every step (steps_*) and the final uPrev / vPrev.

The generator asserts, per step, that tests/_script_scaling_ref.py reproduces
node's numbers bit for bit, and four conditions on the set (re-asserted by
tests/test_script_scaling_cpu.py from the restatement alone):

  * every fixture has a step with maxP > 1e-3 whose dt differs in bits from
    the unscaled rule's;
  * every fixture has a step where the rule evaluated on (double)(float)maxP
    gives another dt than the double does: the double is needed.  max |new -
    old| of two f32 values is itself an f32 whenever the two lie within a
    factor of two of each other (the subtraction is then exact), which is the
    rule at the last iteration of a solve that has not converged; the seeds of
    the SOR and Jacobi cases were searched on the CPU, with the restatement,
    for a step whose maximum sits at a cell that changes sign or more than
    doubles, and the multigrid's |A p' - rhs| carries low bits by itself;
  * over the set the branches scale_idle (maxP <= 1e-3), scale_accepted,
    scale_limited (scaled and still cut by the 1.1 limit) and
    scale_maxvel_zero (maxVel === 0 with scaling on) are all taken;
  * no solve of any step sits in the solve-level caveat zone: (float)maxError <
    p_tol agrees with the script's double comparison on every iteration.

    python tests/golden/make_js_update_scaling_golden.py

Only fixtures whose .npz is missing are generated.
"""
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
sys.path.insert(0, HERE)
import _script_scaling_ref as scal            # noqa: E402
import _script_step_ref as ref                # noqa: E402
import _script_update_ref as upd              # noqa: E402
import make_js_update_golden as base          # noqa: E402

NU = base.NU
BRANCHES = ("scale_idle", "scale_accepted", "scale_limited", "scale_maxvel_zero")

# as make_js_update_golden.CASES, plus the seed of the start state's noise
CASES = {
    "js_update_scaling_24x7_rest_second_mg_p2": dict(nx=24, ny=7, lx=24 / 128.0, ly=7 / 128.0, cyl=None,
                                                     scheme=1, solver=2, profile=0, target=40.0,
                                                     dt_user=0.001, K=5, start="rest", seed=1),
    "js_update_scaling_16x4_first_jac": dict(nx=16, ny=4, lx=30.0, ly=10.0, cyl=None, scheme=0, solver=5,
                                             profile=0, target=0.5, dt_user=0.5, K=3,
                                             start=(1500, 1, 0.05, 1.0), seed=8833),
    "js_update_scaling_16x5_quick_sor": dict(nx=16, ny=5, lx=30.0, ly=10.0, cyl=None, scheme=2, solver=4,
                                             profile=1, target=2.0, dt_user=0.5, K=3,
                                             start=(1500, 1, 0.05, 1.0), seed=7047),
}

_OFF = "residualScalingEnabled = false"
assert base.HARNESS.count(_OFF) == 1
HARNESS = base.HARNESS.replace(_OFF, "residualScalingEnabled = true")


def run_node(text, g, case, st):
    """make_js_update_golden.run_node under this module's harness."""
    keep = base.HARNESS
    base.HARNESS = HARNESS
    try:
        return base.run_node(text, g, case, st)
    finally:
        base.HARNESS = keep


def fixture_conditions(name, reps):
    """The three per-fixture conditions on the reports of a fixture's steps
    (_script_scaling_ref.update's, with `slivers` added)."""
    assert any(r["residual_p"] > scal.PRESSURE_TOL and r["dt_next"] != r["dt_unscaled"] for r in reps), \
        (name, "no step whose dt the scaling moves")
    assert any(r["dt_next"] != r["dt_from_f32"] for r in reps), \
        (name, "the float-rounded residual gives the same dt on every step")
    assert not any(r["slivers"] for r in reps), (name, "a solve sits in the solve-level caveat zone")


def conditions(per_fixture):
    """All four conditions on {name: [report per step]}."""
    for name, reps in per_fixture.items():
        fixture_conditions(name, reps)
    seen = {b for reps in per_fixture.values() for r in reps for b in r["branches"]}
    assert set(BRANCHES) <= seen, ("the set never takes", sorted(set(BRANCHES) - seen))


def restate(case, st0):
    """The K steps of a case from st0 with the restatement: (states, reports)."""
    g = ref.Grid(case["nx"], case["ny"], case["lx"], case["ly"], NU, case["cyl"])
    st, states, reps = dict(st0), [], []
    for _ in range(case["K"]):
        sl = scal.solve_slivers(g, st, case["scheme"], case["profile"], case["target"], case["dt_user"],
                                case["solver"])
        st, rep = scal.update(g, st, case["scheme"], case["profile"], case["target"], case["dt_user"],
                              case["solver"])
        rep["slivers"] = sl
        states.append(st)
        reps.append(rep)
    return states, reps


def main():
    text = base.extract()
    assert "if (residualScalingEnabled) {" in text and "maxPressureResidual + 1e-10" in text
    mpath = os.path.join(HERE, "js_update_scaling_manifest.json")
    if os.path.exists(mpath):
        manifest = json.load(open(mpath))
    else:
        manifest = {"generator": "tests/golden/make_js_update_scaling_golden.py",
                    "source": "reference index.html:261-363 (updateSimulation) with residualScalingEnabled "
                              "= true, :1322-1342 and the substep's sources, executed by node " +
                              subprocess.run(["node", "--version"], capture_output=True,
                                             text=True).stdout.strip(),
                    "iters": upd.ITERS, "p_tol": {str(k): v for k, v in upd.P_TOL.items()},
                    "viscosity": NU, "fixtures": {}}
    for name, case in CASES.items():
        if os.path.exists(os.path.join(HERE, name + ".npz")):
            assert name in manifest["fixtures"], f"{name}.npz has no manifest entry"
            print(name, "kept")
            continue
        g = ref.Grid(case["nx"], case["ny"], case["lx"], case["ly"], NU, case["cyl"])
        st0 = base.start_state(g, case, np.random.default_rng(case["seed"]))
        node = run_node(text, g, case, st0)
        states, reps = restate(case, st0)
        for s, (st, rep) in enumerate(zip(states, reps)):
            ru, rv, rp, nsub, dt, inlet, cnt = node["scal"][s]
            assert (rep["residual_u"], rep["residual_v"], rep["residual_p"]) == (ru, rv, rp), (name, s, "residuals")
            assert (rep["substep_count_next"], rep["dt_next"]) == (nsub, dt), (name, s, "decisions")
            assert (rep["inlet_velocity"], rep["step_count"]) == (inlet, cnt), (name, s)
            for f in ("u", "v", "p", "u_prev", "v_prev"):
                assert ref.bits_equal(st[f], node[f][s]), (name, s, f)
                assert np.isfinite(node[f][s]).all(), (name, s, f, "non-finite")
            assert np.isfinite([ru, rv, rp, dt]).all() and dt > 0, (name, s)
        fixture_conditions(name, reps)
        arrays = dict(start_u=st0["u"], start_v=st0["v"], start_p=st0["p"], start_u_prev=st0["u_prev"],
                      start_v_prev=st0["v_prev"], res_u=node["scal"][:, 0], res_v=node["scal"][:, 1],
                      res_p=node["scal"][:, 2], substeps=node["scal"][:, 3].astype(np.int64),
                      dt=node["scal"][:, 4], inlet=node["scal"][:, 5], steps_u=node["u"],
                      steps_v=node["v"], steps_p=node["p"], final_u_prev=node["u_prev"][-1],
                      final_v_prev=node["v_prev"][-1])
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
        manifest["fixtures"][name] = {
            "nx": case["nx"], "ny": case["ny"], "lx": case["lx"], "ly": case["ly"],
            "cylinder": list(case["cyl"]) if case["cyl"] else None, "scheme": case["scheme"],
            "solver": case["solver"], "profile": case["profile"], "target": case["target"],
            "dt_user": case["dt_user"], "steps": case["K"], "start_dt": st0["dt"],
            "start_substep_count": st0["substep_count"], "start_step_count": st0["step_count"],
            "fields": "steps", "tracers": None, "seed": case["seed"],
            "branches": [r["branches"] for r in reps]}
        json.dump(manifest, open(mpath, "w"), indent=1)
        print(name, "substeps", list(arrays["substeps"]), "dt", list(arrays["dt"]))
        print("   ", [r["branches"] for r in reps])
    if set(CASES) <= set(manifest["fixtures"]):
        per = {}
        for name, case in CASES.items():
            fx = np.load(os.path.join(HERE, name + ".npz"))
            meta = manifest["fixtures"][name]
            st0 = dict(u=fx["start_u"], v=fx["start_v"], p=fx["start_p"], u_prev=fx["start_u_prev"],
                       v_prev=fx["start_v_prev"], dt=meta["start_dt"],
                       substep_count=meta["start_substep_count"], step_count=meta["start_step_count"])
            per[name] = restate(case, st0)[1]
        conditions(per)
        assert {fx["solver"] for fx in manifest["fixtures"].values()} == {2, 4, 5}


if __name__ == "__main__":
    sys.exit(main())
