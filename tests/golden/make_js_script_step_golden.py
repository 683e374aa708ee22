"""Golden vectors for the script's substep (cfd_script_piso_step), produced by
the reference's OWN JavaScript (test infrastructure).

pisoStep (index.html:366-867), applyBoundaryConditions (:870-930),
isPointInObstacle (:212-215), the mg* functions (:1344-1470) and the four
constants of :181-184 are read from the reference at generation time and run
under node inside a `new Function` whose parameters are the script's globals;
only numbers are stored, as tests/golden/js_step_*.npz plus a manifest.  No
reference source is written to the repository.

nu, dx, dy, Lx, Ly and the cylinder are passed as the library's f32 values
widened; `inletProfileSelect` is {value: ...}; without a cylinder the radius is
-1, so no distance is <= it.  Each .npz holds in_u, in_v, in_p and, after one
pisoStep(dt_sub): u_star, v_star, rhs, p_prime, u, v, p (f32) and
lastPResidual (f64).

Inputs are seeded random-sign fields, |u| dt_sub / dx up to `cfl`, with planted
3x3 blocks of +0 and of -0 (so selectors that are sums of neighbours hit exact
zeros too).  The generator asserts, per fixture:
  - tests/_script_step_ref.py equals node bit for bit on u_star, v_star, rhs
    (predict) and on u, v, p from node's p_prime (correct);
  - node's obstacle faces (isPointInObstacle at every u and v face) equal the
    restatement's host evaluation, their interval form reproduces them, and
    node's inlet column equals the host's (Math.pow(x, 2) == x * x on every row);
  - for pressure solver 4: tests/_sor_lex_ref.py reproduces node's p_prime from
    node's rhs and no iteration's maxError lies in the sliver below 1e-4 where
    the script's double test and the library's float test differ;
and over the set, for each scheme, that every branch counter of the
restatement is non-zero.

    python tests/golden/make_js_script_step_golden.py [NAME ...]

Only fixtures whose .npz is missing are generated; the seed of a case is
9191 + its position in CASES.
"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _script_step_ref as ref   # noqa: E402
import _sor_lex_ref as sor       # noqa: E402

REF_HTML = "/root/reference/index.html"
ITERS, P_TOL = 50, 1e-4          # the script's own (:184, :745)
SOLVER_NAMES = {2: "multigrid", 4: "sor"}

# name -> (nx, ny, lx, ly, cylinder (x, y, r) or None, scheme, solver, profile,
#          inlet velocity, dt_sub, cfl)
CASES = {
    # nx at its minimum; ny where the j guards overlap (rows 1 .. ny-2 are all edge rows)
    "js_step_16x4_first_mg": (16, 4, 30.0, 10.0, None, 0, 2, 0, 1.25, 0.05, 0.8),
    "js_step_16x4_quick_sor": (16, 4, 30.0, 10.0, None, 2, 4, 1, 0.75, 0.05, 0.8),
    "js_step_16x5_second_mg": (16, 5, 30.0, 10.0, None, 1, 2, 1, 1.0, 0.04, 0.6),
    "js_step_16x5_quick_mg": (16, 5, 30.0, 10.0, None, 2, 2, 0, 1.0, 0.04, 0.6),
    # power-of-two spacing (the multiply-by-reciprocal form of every division)
    "js_step_24x7_second_sor_p2": (24, 7, 24 / 128.0, 7 / 128.0, None, 1, 4, 0, 0.5, 0.001, 0.5),
    "js_step_24x7_quick_sor_p2": (24, 7, 24 / 128.0, 7 / 128.0, (0.09375, 0.03125, 0.0234375),
                                  2, 4, 1, 0.5, 0.001, 0.5),
    # the cylinder, once per scheme
    "js_step_40x12_cyl_first_sor": (40, 12, 30.0, 10.0, (7.5, 5.0, 2.0), 0, 4, 1, 1.5, 0.05, 0.7),
    "js_step_64x24_cyl_second_mg": (64, 24, 30.0, 10.0, (7.5, 5.0, 1.5), 1, 2, 1, 1.5, 0.03, 0.7),
    # nx = 264: a wave covers 248 columns, so the row crosses a wave seam; 20
    # rows: more than a march segment, so a row seam falls inside the grid
    "js_step_264x20_cyl_quick_mg": (264, 20, 30.0, 10.0, (7.5, 5.0, 1.75), 2, 2, 0, 1.5, 0.01, 0.7),
}
NU = 0.01

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
function wr(name, a) { fs.writeFileSync(dir + '/' + name, Buffer.from(a.buffer, a.byteOffset, a.byteLength)); }
const Nx = job.nx, Ny = job.ny;
// the script's functions with the script's own global names
const run = new Function('Nx', 'Ny', 'dx', 'dy', 'Lx', 'Ly', 'nu', 'u', 'v', 'p',
  'cylinderCenterX', 'cylinderCenterY', 'cylinderRadius', 'currentVelocityScheme',
  'currentPressureSolver', 'currentInletVelocity', 'inletProfileSelect', 'dt_sub', 'out',
  'const uStar = new Float32Array(u.length), vStar = new Float32Array(v.length);\n' +
  'const rhs = new Float32Array(Nx * Ny), pPrime = new Float32Array(Nx * Ny);\n' +
  'const pPrime_new = new Float32Array(Nx * Ny);\nlet lastPResidual = 0;\n' + text + `
  for (let j = 0; j < Ny; j++) for (let i = 0; i < Nx + 1; i++)
    out.obs_u[i + j * (Nx + 1)] = isPointInObstacle(i * dx, (j + 0.5) * dy) ? 1 : 0;
  for (let j = 0; j < Ny + 1; j++) for (let i = 0; i < Nx; i++)
    out.obs_v[i + j * Nx] = isPointInObstacle((i + 0.5) * dx, j * dy) ? 1 : 0;
  for (let j = 0; j < Ny; j++) {
    const t = ((j + 0.5) * dy - Ly / 2) / (Ly / 2);
    out.pow_ok[j] = Math.pow(t, 2) === t * t ? 1 : 0;
  }
  pisoStep(dt_sub);
  out.u_star = uStar; out.v_star = vStar; out.rhs = rhs; out.p_prime = pPrime;
  out.res = lastPResidual;`);
const u = f32('u.bin', (Nx + 1) * Ny), v = f32('v.bin', Nx * (Ny + 1)), p = f32('p.bin', Nx * Ny);
const out = { obs_u: new Uint8Array((Nx + 1) * Ny), obs_v: new Uint8Array(Nx * (Ny + 1)),
              pow_ok: new Uint8Array(Ny) };
run(Nx, Ny, job.dx, job.dy, job.lx, job.ly, job.nu, u, v, p, job.cx, job.cy, job.cr, job.scheme,
    job.solver, job.inlet, { value: job.profile }, job.dt_sub, out);
for (const k of ['u_star', 'v_star', 'rhs', 'p_prime', 'obs_u', 'obs_v', 'pow_ok']) wr(k + '.bin', out[k]);
wr('u_out.bin', u); wr('v_out.bin', v); wr('p_out.bin', p);
wr('res.bin', new Float64Array([out.res]));
"""


def _function_text(html, name):
    c0 = html.index("function " + name + "(")
    k = html.index("{", c0)
    depth = 0
    while True:
        if html[k] == "{":
            depth += 1
        elif html[k] == "}":
            depth -= 1
            if depth == 0:
                return html[c0:k + 1]
        k += 1


def extract():
    html = open(REF_HTML).read()
    consts = []
    for pat in (r"const dx2 = dx \* dx;", r"const dy2 = dy \* dy;",
                r"const denom = 2 / dx2 \+ 2 / dy2;", r"const iterations = \d+;"):
        m = re.search(pat, html)
        assert m, pat
        consts.append(m.group(0))
    assert consts[3] == f"const iterations = {ITERS};"
    fns = [_function_text(html, n) for n in
           ("isPointInObstacle", "mgSmooth", "mgRestrict", "mgProlongate", "mgVcycle", "pisoStep",
            "applyBoundaryConditions")]
    return "\n".join(consts + fns)


def make_inputs(g, rng, dt_sub, cfl):
    nx, ny = g.nx, g.ny
    au, av = cfl * g.dx / dt_sub, cfl * g.dy / dt_sub
    u = (rng.uniform(-1, 1, (ny, nx + 1)) * au).astype(np.float32)
    v = (rng.uniform(-1, 1, (ny + 1, nx)) * av).astype(np.float32)
    p = rng.uniform(-1, 1, (ny, nx)).astype(np.float32)
    # 3x3 blocks (clipped to the grid) of +0 and of -0 at the same place in u and v
    for z in (np.float32(0.0), np.float32(-0.0)):
        for _ in range(max(2, nx * ny // 160)):
            j, i = int(rng.integers(0, ny)), int(rng.integers(0, nx))
            u[j:j + 3, i:i + 3] = z
            v[j:j + 3, i:i + 3] = z
    return u, v, p


def run_node(text, g, u, v, p, scheme, solver, profile, inlet, dt_sub):
    nx, ny = g.nx, g.ny
    cx, cy, cr = g.cyl if g.cyl else (0.0, 0.0, -1.0)
    with tempfile.TemporaryDirectory() as d:
        for fn, txt in (("step.js", text), ("harness.js", HARNESS)):
            open(os.path.join(d, fn), "w").write(txt)
        u.tofile(os.path.join(d, "u.bin"))
        v.tofile(os.path.join(d, "v.bin"))
        p.tofile(os.path.join(d, "p.bin"))
        json.dump({"nx": nx, "ny": ny, "dx": g.dx, "dy": g.dy, "lx": g.lx, "ly": g.ly, "nu": g.nu,
                   "cx": cx, "cy": cy, "cr": cr, "scheme": ref.SCHEME_NAMES[scheme],
                   "solver": SOLVER_NAMES[solver], "profile": ref.PROFILE_NAMES[profile],
                   "inlet": inlet, "dt_sub": dt_sub}, open(os.path.join(d, "job.json"), "w"))
        subprocess.run(["node", os.path.join(d, "harness.js"), os.path.join(d, "step.js"),
                        os.path.join(d, "job.json"), d], check=True)

        def rd(name, shape, dt=np.float32):
            return np.fromfile(os.path.join(d, name + ".bin"), dt).reshape(shape)
        out = {"u_star": rd("u_star", (ny, nx + 1)), "v_star": rd("v_star", (ny + 1, nx)),
               "rhs": rd("rhs", (ny, nx)), "p_prime": rd("p_prime", (ny, nx)),
               "u": rd("u_out", (ny, nx + 1)), "v": rd("v_out", (ny + 1, nx)),
               "p": rd("p_out", (ny, nx)),
               "obs_u": rd("obs_u", (ny, nx + 1), np.uint8).astype(bool),
               "obs_v": rd("obs_v", (ny + 1, nx), np.uint8).astype(bool),
               "pow_ok": rd("pow_ok", (ny,), np.uint8),
               "lastPResidual": rd("res", (1,), np.float64)}
    return out


def check_host_data(name, g, node, profile, inlet):
    """Obstacle faces, their interval form and the inlet column against node."""
    ou, ov = ref.obstacle_faces(g)
    assert np.array_equal(ou, node["obs_u"]) and np.array_equal(ov, node["obs_v"]), (name, "obstacle")
    for m in (ou, ov):
        assert np.array_equal(ref.intervals_to_mask(ref.obstacle_intervals(m), m.shape[1]), m), name
    # Math.pow(t, 2) === t * t at every row's t; and after the boundary pass
    # u[0, j] is the inlet value on every row but the walls and obstacle faces
    assert node["pow_ok"].all(), (name, "Math.pow(t, 2) != t * t")
    col = ref.inlet_column(g, inlet, profile)
    rows = np.arange(1, g.ny - 1)
    rows = rows[~ou[rows, 0]]
    assert ref.bits_equal(node["u"][rows, 0], col[rows]), (name, "inlet column")


def main(only=()):
    unknown = [n for n in only if n not in CASES]
    if unknown:
        raise SystemExit(f"unknown fixture(s) {unknown}; CASES has {list(CASES)}")
    text = extract()
    assert "uStar.set(u)" in text and "v[idx+2] - 2*v[idx] + v[idx]" in text
    assert "Math.pow((y-center)/radius, 2)" in text
    mpath = os.path.join(HERE, "js_step_manifest.json")
    if os.path.exists(mpath):
        manifest = json.load(open(mpath))
    else:
        manifest = {"generator": "tests/golden/make_js_script_step_golden.py",
                    "source": "reference index.html:366-867 (pisoStep), :870-930 "
                              "(applyBoundaryConditions), :212-215, :1344-1470 (mg*), :181-184, "
                              "executed by node " +
                              subprocess.run(["node", "--version"], capture_output=True,
                                             text=True).stdout.strip(),
                    "iters": ITERS, "p_tol": P_TOL, "viscosity": NU, "fixtures": {}}
    for k, (name, case) in enumerate(CASES.items()):
        nx, ny, lx, ly, cyl, scheme, solver, profile, inlet, dt_sub, cfl = case
        if only and name not in only:
            continue
        if os.path.exists(os.path.join(HERE, name + ".npz")):
            assert name in manifest["fixtures"], f"{name}.npz has no manifest entry"
            print(name, "kept")
            continue
        g = ref.Grid(nx, ny, lx, ly, NU, cyl)
        dt_sub = float(np.float32(dt_sub))
        inlet = float(np.float32(inlet))
        rng = np.random.default_rng(9191 + k)
        u, v, p = make_inputs(g, rng, dt_sub, cfl)
        node = run_node(text, g, u, v, p, scheme, solver, profile, inlet, dt_sub)
        check_host_data(name, g, node, profile, inlet)
        counters = {}
        us, vs, rhs = ref.predict(g, u, v, dt_sub, scheme, counters)
        for nm, a in (("u_star", us), ("v_star", vs), ("rhs", rhs)):
            assert ref.bits_equal(a, node[nm]), (name, nm)
        un, vn, pn = ref.correct(g, node["u_star"], node["v_star"], node["p_prime"], p, dt_sub,
                                 inlet, profile)
        for nm, a in (("u", un), ("v", vn), ("p", pn)):
            assert ref.bits_equal(a, node[nm]), (name, nm)
        for nm in ("u_star", "v_star", "rhs", "p_prime", "u", "v", "p"):
            assert np.isfinite(node[nm]).all(), (name, nm, "non-finite")
        sor_iters = None
        if solver == 4:
            pp, sor_iters, errs = sor.sor_lex_diag(node["rhs"], nx, ny, g.dx, g.dy, ITERS, True, P_TOL)
            assert sor.slivers(errs, P_TOL) == [], (name, "maxError in the sliver below 1e-4")
            assert ref.bits_equal(pp, node["p_prime"]), (name, "p_prime vs _sor_lex_ref")
            assert errs[-1] == float(node["lastPResidual"][0]), (name, "lastPResidual")
        np.savez_compressed(os.path.join(HERE, name + ".npz"), in_u=u, in_v=v, in_p=p,
                            **{nm: node[nm] for nm in ("u_star", "v_star", "rhs", "p_prime", "u",
                                                       "v", "p", "lastPResidual")})
        manifest["fixtures"][name] = {
            "nx": nx, "ny": ny, "lx": lx, "ly": ly, "cylinder": list(cyl) if cyl else None,
            "scheme": scheme, "solver": solver, "profile": profile, "inlet_velocity": inlet,
            "dt_sub": dt_sub, "seed": 9191 + k, "sor_iterations": sor_iters,
            "branches": {c: n for c, n in sorted(counters.items())}}
        print(name, "residual", float(node["lastPResidual"][0]), "sor iters", sor_iters)
    if not only and set(CASES) <= set(manifest["fixtures"]):
        for scheme in ref.SCHEME_NAMES:
            tot = {c: 0 for c in ref.counter_names(scheme)}
            for fx in manifest["fixtures"].values():
                if fx["scheme"] == scheme:
                    assert set(fx["branches"]) == set(tot), (scheme, "counter names")
                    for c, n in fx["branches"].items():
                        tot[c] += n
            missed = sorted(c for c, n in tot.items() if n == 0)
            assert not missed, (ref.SCHEME_NAMES[scheme], "the set never takes", missed)
        combos = {(fx["scheme"], fx["solver"]) for fx in manifest["fixtures"].values()}
        assert combos == {(s, q) for s in (0, 1, 2) for q in (2, 4)}, combos
        assert {fx["profile"] for fx in manifest["fixtures"].values()} == {0, 1}
    json.dump(manifest, open(mpath, "w"), indent=1)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
