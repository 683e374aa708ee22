"""Golden vectors for the script's Jacobi solver (pressure_solver 5), produced
by the reference's OWN JavaScript (test infrastructure).

The Jacobi branch of the reference's JavaScript variant (index.html:796-838) is
a plain loop nest over typed arrays.  This script reads its text from the
reference at generation time, runs it under node on seeded right-hand sides
(p' pre-filled with 7: the branch zeroes it itself) and stores only the
numbers, as tests/golden/js_jac_*.npz plus a manifest.  No reference source is
written to the repository.  Each .npz holds in_rhs, out_solve, the iteration
count `iters_run` and `max_errors_f64`, the script's double maxError of every
iteration run.  The script reports only the last iteration's: iteration k's is
what the branch returns when it is run with `iterations` = k, so the branch is
run once per count.  The iteration count is taken from the restatement
(tests/_jacobi_script_ref.py), whose p' must equal the script's bit for bit --
which confirms the count, as a further iteration would change p'.

The library compares (float)maxError with the float p_tol where the script
compares doubles (include/cfd.h): the generator asserts that no iteration of
any fixture lies where the two comparisons differ.

Shapes: the kernel (cfd_jacobi_script.hip) gives a wave 124 columns and 4
interior rows, a workgroup 16 interior rows; the case names say which seam a
shape crosses.

    python tests/golden/make_js_jacobi_golden.py [NAME ...]

Only fixtures whose .npz is missing are generated; the seed of a case is
6161 + its position in CASES.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _jacobi_script_ref as ref   # noqa: E402

REF_HTML = "/root/reference/index.html"

# name -> (nx, ny, lx, ly, iterations, rhs scale (None: searched, see exit
# parity; 0: rhs = 0), expected exit: None no early exit, 0 / 1 early exit at
# an even / odd count)
CASES = {
    "js_jac_16x4": (16, 4, 30.0, 10.0, 5, 100.0, None),                    # the interior is two rows
    "js_jac_16x5": (16, 5, 30.0, 10.0, 9, 100.0, None),
    "js_jac_24x7_p2": (24, 7, 24 / 128.0, 7 / 128.0, 50, 100.0, None),     # power-of-two spacing
    "js_jac_32x12_it1": (32, 12, 30.0, 10.0, 1, 100.0, None),              # jacobi_iters = 1
    "js_jac_16x5_zero": (16, 5, 30.0, 10.0, 50, 0.0, 1),                   # rhs = 0: exit after one
    "js_jac_32x12_exit_odd": (32, 12, 30.0, 10.0, 50, None, 1),
    "js_jac_40x24_exit_even": (40, 24, 30.0, 10.0, 50, None, 0),
    "js_jac_64x20_fixed": (64, 20, 4.0, 1.25, 12, 100.0, None),            # fixed count (run with the tolerance off too)
    "js_jac_16x10_yseam_wave": (16, 10, 30.0, 10.0, 7, 100.0, None),       # interior rows 1-4 | 5-8: a wave seam
    "js_jac_16x22_yseam_block": (16, 22, 30.0, 10.0, 7, 100.0, None),      # interior rows 1-16 | 17-20: a workgroup seam
    "js_jac_136x7_xseam": (136, 7, 30.0, 10.0, 7, 100.0, None),            # columns 0-123 | 124-135: a wave seam in x
    "js_jac_136x24_xyseam": (136, 24, 30.0, 10.0, 8, 100.0, None),         # both, IEEE division
}

HARNESS = r"""
'use strict';
const fs = require('fs');
const branchText = fs.readFileSync(process.argv[2], 'utf8');
const job = JSON.parse(fs.readFileSync(process.argv[3], 'utf8'));
const dir = process.argv[4];
const nx = job.nx, ny = job.ny, dx = job.dx, dy = job.dy;
const b = fs.readFileSync(dir + '/rhs.bin');
const rhs = new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + 4 * nx * ny));
// the Jacobi branch with the script's own names; denom as index.html:181-183 forms it
const dx2 = dx * dx, dy2 = dy * dy;
const denom = 2 / dx2 + 2 / dy2;
const branch = new Function('pPrime', 'pPrime_new', 'rhs', 'Nx', 'Ny', 'dx', 'dy', 'denom', 'iterations',
  'let lastPResidual;\n' + branchText + '\nreturn lastPResidual;');
const errs = [];
let pPrime;
for (let n = 1; n <= job.iterations; n++) {
  pPrime = new Float32Array(nx * ny).fill(7);   // the branch zeroes it itself
  const pNew = new Float32Array(nx * ny).fill(9);
  errs.push(branch(pPrime, pNew, rhs, nx, ny, dx, dy, denom, n));
}
fs.writeFileSync(dir + '/solve.bin', Buffer.from(pPrime.buffer));
fs.writeFileSync(dir + '/residual.json', JSON.stringify({ errs: errs }));
"""


def extract():
    html = open(REF_HTML).read()
    c0 = html.index("} else { // Default: Pressure Correction using Jacobi Iteration")
    c0 = html.index("{", c0) + 1
    c1 = html.index("// ----------------- Corrector Step", c0)
    return html[c0:html.rindex("}", c0, c1)]


def run_node(branch, rhs, nx, ny, dx, dy, iters):
    with tempfile.TemporaryDirectory() as d:
        for fn, txt in (("branch.js", branch), ("harness.js", HARNESS)):
            open(os.path.join(d, fn), "w").write(txt)
        rhs.tofile(os.path.join(d, "rhs.bin"))
        json.dump({"nx": nx, "ny": ny, "dx": float(dx), "dy": float(dy), "iterations": iters},
                  open(os.path.join(d, "job.json"), "w"))
        subprocess.run(["node", os.path.join(d, "harness.js"), os.path.join(d, "branch.js"),
                        os.path.join(d, "job.json"), d], check=True)
        solve = np.fromfile(os.path.join(d, "solve.bin"), np.float32)
        errs = json.load(open(os.path.join(d, "residual.json")))["errs"]
    return solve, errs


def main(only=()):
    unknown = [n for n in only if n not in CASES]
    if unknown:
        raise SystemExit(f"unknown fixture(s) {unknown}; CASES has {list(CASES)}")
    branch = extract()
    assert "pPrime.fill(0)" in branch and "jacobiOmega = 0.7" in branch
    assert "pressureTolerance = 1e-6" in branch and "pPrime_new.fill(0)" in branch
    mpath = os.path.join(HERE, "js_jac_manifest.json")
    if os.path.exists(mpath):
        manifest = json.load(open(mpath))
    else:
        manifest = {"generator": "tests/golden/make_js_jacobi_golden.py",
                    "source": "reference index.html:796-838 (Jacobi branch), executed by node " +
                              subprocess.run(["node", "--version"], capture_output=True,
                                             text=True).stdout.strip(),
                    "p_tol": ref.P_TOL, "fixtures": {}}
    for k, (name, (nx, ny, lx, ly, iters, scale, exit_parity)) in enumerate(CASES.items()):
        if only and name not in only:
            continue
        if os.path.exists(os.path.join(HERE, name + ".npz")):
            assert name in manifest["fixtures"], f"{name}.npz has no manifest entry"
            print(name, "kept")
            continue
        dx = np.float32(lx) / np.float32(nx)
        dy = np.float32(ly) / np.float32(ny)
        rng = np.random.default_rng(6161 + k)
        base = rng.uniform(-1, 1, nx * ny)
        if scale is None:
            # the first scale of a fixed ladder whose early exit has the wanted
            # parity after at least 3 iterations, outside the sliver
            for t in range(200):
                scale = 4e-6 * 1.03 ** t
                _, n_run, errs = ref.jacobi_script((base * scale).astype(np.float32), nx, ny, dx, dy, iters)
                if 3 <= n_run < iters and n_run % 2 == exit_parity and not ref.slivers(errs):
                    break
            else:
                raise SystemExit(f"{name}: no scale gives the exit parity")
        rhs = (base * scale).astype(np.float32)
        solve, node_errs = run_node(branch, rhs, nx, ny, dx, dy, iters)
        P, n_run, errs = ref.jacobi_script(rhs, nx, ny, dx, dy, iters, True, ref.P_TOL)
        assert np.array_equal(P.reshape(-1).view(np.uint32), solve.view(np.uint32)), name
        # runs with `iterations` beyond the exit repeat the exit's value
        assert node_errs[:n_run] == errs, (name, node_errs, errs)
        assert all(e == errs[-1] for e in node_errs[n_run:]), name
        assert not ref.slivers(errs), (name, "an iteration's maxError lies in the f32/f64 sliver")
        if exit_parity is None:
            assert n_run == iters and not errs[-1] < ref.P_TOL, (name, n_run)
        else:
            assert n_run < iters and n_run % 2 == exit_parity, (name, n_run)
        if scale == 0.0:
            assert n_run == 1 and errs == [0.0] and not solve.any(), name
        np.savez_compressed(os.path.join(HERE, name + ".npz"), in_rhs=rhs, out_solve=solve,
                            max_errors_f64=np.array(errs, np.float64),
                            iters_run=np.array([n_run], np.int64))
        manifest["fixtures"][name] = {"nx": nx, "ny": ny, "lx": lx, "ly": ly, "dx": float(dx),
                                      "dy": float(dy), "iterations": iters, "rhs_scale": scale,
                                      "iters_run": n_run, "seed": 6161 + k}
        print(name, "iterations run", n_run, "residual", errs[-1])
    json.dump(manifest, open(mpath, "w"), indent=1)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
