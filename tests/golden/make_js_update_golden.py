"""Golden vectors for the script's time step (cfd_script_update), produced by
the reference's OWN JavaScript (test infrastructure).

updateSimulation (index.html:261-363), computeAutomaticTimeStep (:1322-1342),
simulationLoop (:1229-1243), the tracer functions (:1475-1543) and everything
make_js_script_step_golden.py extracts for pisoStep are read from the reference
at generation time and run under node inside a `new Function` whose parameters
and leading `let`s are the script's globals; only numbers are stored, as
tests/golden/js_update_*.npz plus a manifest.  No reference source is written to
the repository.  The page's DOM objects are plain objects holding numbers or
strings (timeStepInput = {value: dt_user}, residualText = {value: ""}, ...), the
drawing functions and requestAnimationFrame do nothing, and
tracerInjectionInterval is the job's number.

Each fixture is K consecutive simulationLoop() calls from a stored start
(start_u, start_v, start_p, start_u_prev, start_v_prev, and dt, substepCount,
simulationStepCount in the manifest).  Per step the .npz holds res_u, res_v,
res_p (the script's doubles), substeps (substepCount after the step), dt (after
the step) and inlet (currentInletVelocity); u, v, p after every step (small
shapes: steps_u[k] ...) or after the last step only (final_u ...); the tracer
fixture also holds the tracer lists after each step (trc_n, trc_x, trc_y, trc_i,
concatenated).

The generator asserts, per step, that tests/_script_update_ref.py reproduces
node's numbers bit for bit, and that the substep and dt decisions taken with
the float-rounded pressure residual (the library's convention, include/cfd.h)
equal the script's own; over the set, that every branch of BRANCHES is taken
and that the schemes, profiles, solvers and cylinder / no cylinder all occur.
`dt_cfl` only says that the CFL quotient was below dt_user; `dt_is_cfl` says
that it became the step's dt (not cut by the 1.1 limit), once with dx < dy and
the velocity maximum in u and once with dy < dx and the maximum in v, and the
stored dt of those steps is neither dt_user nor 1.1 x the previous dt.

    python tests/golden/make_js_update_golden.py

Only fixtures whose .npz is missing are generated; the seed of a case is
8181 + its position in CASES.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
sys.path.insert(0, HERE)
import _script_step_ref as ref                # noqa: E402
import _script_update_ref as upd              # noqa: E402
import _tracers_ref as trc                    # noqa: E402
import make_js_script_step_golden as step     # noqa: E402

REF_HTML = step.REF_HTML
SOLVER_NAMES = {2: "multigrid", 4: "sor", 5: "jacobi"}
NU = 0.01
BRANCHES = ("step0", "extrapolated", "ramp", "ramp_done", "sub_grown", "sub_capped", "sub_halved",
            "sub_floored", "sub_unchanged", "maxvel_zero", "dt_cfl", "dt_user", "dt_limited",
            "dt_is_cfl", "cfl_from_u", "cfl_from_v")

# name -> dict(nx, ny, lx, ly, cyl, scheme, solver, profile, target, dt_user, K,
#   start: "rest" (initSimulation: zeros, step 0, dt = dt_user, substepCount 5)
#          or (step_count, substep_count, dt, amplitude of the seeded fields),
#   fields: "steps" / "final", tracers: injection interval or None)
CASES = {
    "js_update_16x4_rest_first_jac": dict(nx=16, ny=4, lx=30.0, ly=10.0, cyl=None, scheme=0, solver=5,
                                          profile=0, target=0.05, dt_user=0.5, K=8, start="rest"),
    "js_update_16x5_rest_quick_sor": dict(nx=16, ny=5, lx=30.0, ly=10.0, cyl=None, scheme=2, solver=4,
                                          profile=1, target=2.0, dt_user=0.5, K=8, start="rest"),
    "js_update_24x7_ramp_second_mg_p2": dict(nx=24, ny=7, lx=24 / 128.0, ly=7 / 128.0, cyl=None, scheme=1,
                                             solver=2, profile=0, target=0.5, dt_user=0.001, K=6,
                                             start=(998, 3, 0.0005, 0.3)),
    "js_update_40x12_cyl_quick_jac": dict(nx=40, ny=12, lx=30.0, ly=10.0, cyl=(7.5, 5.0, 2.0), scheme=2,
                                          solver=5, profile=1, target=1.5, dt_user=0.5, K=6,
                                          start=(1200, 20, 0.05, 1.0)),
    "js_update_40x12_tracers_first_sor": dict(nx=40, ny=12, lx=30.0, ly=10.0, cyl=(7.5, 5.0, 2.0),
                                              scheme=0, solver=4, profile=0, target=1.0, dt_user=0.2,
                                              K=7, start=(41, 4, 0.1, 0.5), tracers=2),
    "js_update_136x24_cyl_second_jac": dict(nx=136, ny=24, lx=30.0, ly=10.0, cyl=(7.5, 5.0, 1.5),
                                            scheme=1, solver=5, profile=1, target=1.0, dt_user=0.01,
                                            K=6, start=(300, 2, 0.01, 0.4), fields="final"),
    "js_update_64x24_cyl_first_mg": dict(nx=64, ny=24, lx=30.0, ly=10.0, cyl=(7.5, 5.0, 1.5), scheme=0,
                                         solver=2, profile=1, target=1.0, dt_user=0.02, K=6,
                                         start=(2000, 1, 0.02, 0.02), fields="final"),
    # dt IS the CFL quotient: the previous dt and dt_user both lie above
    # 0.5 min(dx, dy) / maxVel.  dx < dy with the maximum in u; dy < dx with a
    # cross flow stronger than the channel's, so the maximum is in v
    "js_update_40x12_cfl_second_jac": dict(nx=40, ny=12, lx=30.0, ly=10.0, cyl=(7.5, 5.0, 2.0), scheme=1,
                                           solver=5, profile=1, target=1.5, dt_user=0.5, K=6,
                                           start=(1500, 20, 0.4, 0.5)),
    "js_update_24x12_cfl_v_first_sor": dict(nx=24, ny=12, lx=30.0, ly=10.0, cyl=None, scheme=0, solver=4,
                                            profile=0, target=0.05, dt_user=2.0, K=6,
                                            start=(1500, 20, 1.5, 0.5), v_amp=0.6),
}

HARNESS = r"""
'use strict';
const fs = require('fs');
const text = fs.readFileSync(process.argv[2], 'utf8');
const job = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const dir = process.argv[4];
function f32(name, n) {
  const b = fs.readFileSync(dir + '/' + name);
  return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + 4 * n));
}
const Nx = job.nx, Ny = job.ny;
const nop = function () {};
// the script's functions with the script's own global names
const run = new Function('Nx', 'Ny', 'dx', 'dy', 'Lx', 'Ly', 'nu', 'u', 'v', 'p', 'uPrev', 'vPrev',
  'cylinderCenterX', 'cylinderCenterY', 'cylinderRadius', 'currentVelocityScheme',
  'currentPressureSolver', 'inletProfileSelect', 'timeStepInput', 'targetInletVelocity',
  'rampUpSteps', 'tracerInjectionInterval', 'residualText', 'document', 'drawSimulation',
  'drawResidualGraph', 'drawLegend', 'requestAnimationFrame', 'job', 'out',
  'const uStar = new Float32Array(u.length), vStar = new Float32Array(v.length);\n' +
  'const uOld = new Float32Array(u.length), vOld = new Float32Array(v.length);\n' +
  'const rhs = new Float32Array(Nx * Ny), pPrime = new Float32Array(Nx * Ny);\n' +
  'const pPrime_new = new Float32Array(Nx * Ny);\nlet lastPResidual = 0;\n' +
  'let simulationStepCount = job.step_count, substepCount = job.substep_count, dt = job.dt;\n' +
  'let currentInletVelocity = 0, residualScalingEnabled = false, simulationRunning = true;\n' +
  'let tracersEnabled = job.tracers > 0, tracers = [];\n' +
  'let residualHistoryU = [], residualHistoryV = [], residualHistoryP = [];\n' + text + `
  if (tracersEnabled) initTracers();
  for (let k = 0; k < job.K; k++) {
    simulationLoop();
    out.scal.push([residualHistoryU[k].residual, residualHistoryV[k].residual,
                   residualHistoryP[k].residual, substepCount, dt, currentInletVelocity,
                   simulationStepCount]);
    out.u.push(new Float32Array(u)); out.v.push(new Float32Array(v)); out.p.push(new Float32Array(p));
    out.up.push(new Float32Array(uPrev)); out.vp.push(new Float32Array(vPrev));
    out.trc.push(tracers.map(t => [t.x, t.y, t.initialY]));
  }`);
const u = f32('u.bin', (Nx + 1) * Ny), v = f32('v.bin', Nx * (Ny + 1)), p = f32('p.bin', Nx * Ny);
const up = f32('up.bin', (Nx + 1) * Ny), vp = f32('vp.bin', Nx * (Ny + 1));
const out = { scal: [], u: [], v: [], p: [], up: [], vp: [], trc: [] };
run(Nx, Ny, job.dx, job.dy, job.lx, job.ly, job.nu, u, v, p, up, vp, job.cx, job.cy, job.cr, job.scheme,
    job.solver, { value: job.profile }, { value: job.dt_user }, job.target, 1000, job.tracers,
    { value: '', scrollTop: 0, scrollHeight: 0 },
    { getElementById: function () { return { textContent: '' }; } }, nop, nop, nop, nop, job, out);
function cat(list) {
  const n = list.reduce((a, x) => a + x.length, 0), r = new Float32Array(n);
  let o = 0;
  for (const x of list) { r.set(x, o); o += x.length; }
  return r;
}
for (const k of ['u', 'v', 'p', 'up', 'vp']) {
  const a = cat(out[k]);
  fs.writeFileSync(dir + '/' + k + '_out.bin', Buffer.from(a.buffer, a.byteOffset, a.byteLength));
}
const sc = new Float64Array([].concat(...out.scal));
fs.writeFileSync(dir + '/scal.bin', Buffer.from(sc.buffer));
const tn = new Float64Array(out.trc.map(l => l.length));
const tv = new Float64Array([].concat(...out.trc.map(l => [].concat(...l))));
fs.writeFileSync(dir + '/trc_n.bin', Buffer.from(tn.buffer));
fs.writeFileSync(dir + '/trc_v.bin', Buffer.from(tv.buffer));
"""


def extract():
    html = open(REF_HTML).read()
    fns = [step._function_text(html, n) for n in
           ("updateSimulation", "computeAutomaticTimeStep", "simulationLoop", "initTracers",
            "updateTracers", "getVelocityAt", "injectTracers")]
    return step.extract() + "\n" + "\n".join(fns)


def start_state(g, case, rng):
    nx, ny = g.nx, g.ny
    if case["start"] == "rest":
        z = dict(u=np.zeros((ny, nx + 1), np.float32), v=np.zeros((ny + 1, nx), np.float32),
                 p=np.zeros((ny, nx), np.float32))
        return dict(z, u_prev=z["u"].copy(), v_prev=z["v"].copy(), dt=float(case["dt_user"]),
                    substep_count=5, step_count=0)
    n, nsub, dt, amp = case["start"]
    # a smooth flow (so a run of steps stays finite) plus seeded noise; the
    # previous fields differ from the current ones
    y = (np.arange(ny) + 0.5) / ny
    prof = (4 * y * (1 - y))[:, None] * case["target"]
    u = (prof + amp * 0.05 * rng.uniform(-1, 1, (ny, nx + 1))).astype(np.float32)
    v = (case.get("v_amp", amp * 0.05) * rng.uniform(-1, 1, (ny + 1, nx))).astype(np.float32)
    p = (amp * rng.uniform(-1, 1, (ny, nx))).astype(np.float32)
    up = (u * np.float32(0.98) + np.float32(amp * 0.01) * rng.uniform(-1, 1, u.shape).astype(np.float32)).astype(np.float32)
    vp = (v * np.float32(0.98)).astype(np.float32)
    return dict(u=u, v=v, p=p, u_prev=up, v_prev=vp, dt=float(dt), substep_count=int(nsub),
                step_count=int(n))


def run_node(text, g, case, st):
    nx, ny = g.nx, g.ny
    K = case["K"]
    cx, cy, cr = g.cyl if g.cyl else (0.0, 0.0, -1.0)
    with tempfile.TemporaryDirectory() as d:
        for fn, txt in (("update.js", text), ("harness.js", HARNESS)):
            open(os.path.join(d, fn), "w").write(txt)
        for nm, key in (("u", "u"), ("v", "v"), ("p", "p"), ("up", "u_prev"), ("vp", "v_prev")):
            st[key].tofile(os.path.join(d, nm + ".bin"))
        json.dump({"nx": nx, "ny": ny, "dx": g.dx, "dy": g.dy, "lx": g.lx, "ly": g.ly, "nu": g.nu,
                   "cx": cx, "cy": cy, "cr": cr, "scheme": ref.SCHEME_NAMES[case["scheme"]],
                   "solver": SOLVER_NAMES[case["solver"]], "profile": ref.PROFILE_NAMES[case["profile"]],
                   "dt_user": case["dt_user"], "target": case["target"], "K": K,
                   "tracers": case.get("tracers") or 0, "step_count": st["step_count"],
                   "substep_count": st["substep_count"], "dt": st["dt"]},
                  open(os.path.join(d, "job.json"), "w"))
        subprocess.run(["node", os.path.join(d, "harness.js"), os.path.join(d, "update.js"),
                        os.path.join(d, "job.json"), d], check=True)

        def rd(name, shape, dt=np.float32):
            return np.fromfile(os.path.join(d, name + ".bin"), dt).reshape(shape)
        out = {"u": rd("u_out", (K, ny, nx + 1)), "v": rd("v_out", (K, ny + 1, nx)),
               "p": rd("p_out", (K, ny, nx)), "u_prev": rd("up_out", (K, ny, nx + 1)),
               "v_prev": rd("vp_out", (K, ny + 1, nx)), "scal": rd("scal", (K, 7), np.float64),
               "trc_n": rd("trc_n", (K,), np.float64).astype(np.int64),
               "trc_v": rd("trc_v", (-1, 3), np.float64)}
    return out


def main():
    text = extract()
    assert "u[i] = 2 * u[i] - uPrev[i]" in text and "const maxIncreaseFactor = 1.1;" in text
    assert "updateTracers(dt);" in text
    mpath = os.path.join(HERE, "js_update_manifest.json")
    if os.path.exists(mpath):
        manifest = json.load(open(mpath))
    else:
        manifest = {"generator": "tests/golden/make_js_update_golden.py",
                    "source": "reference index.html:261-363 (updateSimulation), :1322-1342, "
                              ":1229-1243, :1475-1543 and the substep's sources, executed by node " +
                              subprocess.run(["node", "--version"], capture_output=True,
                                             text=True).stdout.strip(),
                    "iters": upd.ITERS, "p_tol": {str(k): v for k, v in upd.P_TOL.items()},
                    "viscosity": NU, "fixtures": {}}
    for k, (name, case) in enumerate(CASES.items()):
        if os.path.exists(os.path.join(HERE, name + ".npz")):
            assert name in manifest["fixtures"], f"{name}.npz has no manifest entry"
            print(name, "kept")
            continue
        g = ref.Grid(case["nx"], case["ny"], case["lx"], case["ly"], NU, case["cyl"])
        rng = np.random.default_rng(8181 + k)
        st0 = start_state(g, case, rng)
        node = run_node(text, g, case, st0)
        K = case["K"]
        st = dict(st0)
        dom = trc.Domain(g.nx, g.ny, g.lx, g.ly)
        tr = trc.init(dom) if case.get("tracers") else None
        taken, toff = [], 0
        for s in range(K):
            st, rep = upd.update(g, st, case["scheme"], case["profile"], case["target"],
                                 case["dt_user"], case["solver"])
            ru, rv, rp, nsub, dt, inlet, cnt = node["scal"][s]
            assert (rep["residual_u"], rep["residual_v"], rep["residual_p_f64"]) == (ru, rv, rp), (name, s, "residuals")
            assert (rep["substep_count_next"], rep["dt_next"]) == (nsub, dt), (name, s, "decisions")
            assert rep["script_decisions"] == (nsub, dt), (name, s, "the float-rounded residual moves a decision")
            assert (rep["inlet_velocity"], rep["step_count"]) == (inlet, cnt), (name, s)
            for f in ("u", "v", "p", "u_prev", "v_prev"):
                assert ref.bits_equal(st[f], node[f][s]), (name, s, f)
                assert np.isfinite(node[f][s]).all(), (name, s, f, "non-finite")
            assert np.isfinite([ru, rv, rp, dt]).all() and dt > 0, (name, s)
            if tr is not None:
                tr = trc.step(dom, st["u"].ravel(), st["v"].ravel(), st["dt"], st["step_count"],
                              case["tracers"], tr)
                n = int(node["trc_n"][s])
                want = node["trc_v"][toff:toff + n]
                toff += n
                assert len(tr[0]) == n and all(trc.bits_equal(tr[c], want[:, c]) for c in range(3)), (name, s, "tracers")
            taken.append(rep["branches"])
        arrays = dict(start_u=st0["u"], start_v=st0["v"], start_p=st0["p"], start_u_prev=st0["u_prev"],
                      start_v_prev=st0["v_prev"], res_u=node["scal"][:, 0], res_v=node["scal"][:, 1],
                      res_p=node["scal"][:, 2], substeps=node["scal"][:, 3].astype(np.int64),
                      dt=node["scal"][:, 4], inlet=node["scal"][:, 5])
        if case.get("fields", "steps") == "steps":
            arrays.update(steps_u=node["u"], steps_v=node["v"], steps_p=node["p"])
        else:
            arrays.update(final_u=node["u"][-1], final_v=node["v"][-1], final_p=node["p"][-1])
        arrays.update(final_u_prev=node["u_prev"][-1], final_v_prev=node["v_prev"][-1])
        if tr is not None:
            arrays.update(trc_n=node["trc_n"], trc_x=node["trc_v"][:, 0], trc_y=node["trc_v"][:, 1],
                          trc_i=node["trc_v"][:, 2])
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
        manifest["fixtures"][name] = {
            "nx": case["nx"], "ny": case["ny"], "lx": case["lx"], "ly": case["ly"],
            "cylinder": list(case["cyl"]) if case["cyl"] else None, "scheme": case["scheme"],
            "solver": case["solver"], "profile": case["profile"], "target": case["target"],
            "dt_user": case["dt_user"], "steps": K, "start_dt": st0["dt"],
            "start_substep_count": st0["substep_count"], "start_step_count": st0["step_count"],
            "fields": case.get("fields", "steps"), "tracers": case.get("tracers"),
            "seed": 8181 + k, "branches": taken}
        json.dump(manifest, open(mpath, "w"), indent=1)
        print(name, "substeps", list(arrays["substeps"]), "dt", list(arrays["dt"]))
        print("   ", sorted({b for bs in taken for b in bs}))
    if set(CASES) <= set(manifest["fixtures"]):
        fxs = manifest["fixtures"].values()
        seen = {b for fx in fxs for bs in fx["branches"] for b in bs}
        assert seen == set(BRANCHES), ("the set never takes", sorted(set(BRANCHES) - seen))
        assert {fx["scheme"] for fx in fxs} == {0, 1, 2} and {fx["profile"] for fx in fxs} == {0, 1}
        assert {fx["solver"] for fx in fxs} == {2, 4, 5}
        assert {fx["cylinder"] is None for fx in fxs} == {True, False}
        assert any(fx["tracers"] for fx in fxs)
        # some step's dt is the CFL value itself: neither dt_user nor 1.1 x the previous dt
        free = 0
        for name, fx in manifest["fixtures"].items():
            dts = [fx["start_dt"]] + list(np.load(os.path.join(HERE, name + ".npz"))["dt"])
            free += sum(1 for a, b in zip(dts, dts[1:]) if b != fx["dt_user"] and b != a * 1.1)
        assert free >= 2, "no step's dt is the CFL quotient"


if __name__ == "__main__":
    sys.exit(main())
