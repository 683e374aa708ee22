"""Golden vectors for the script-order SOR solver (pressure_solver 4),
produced by the reference's OWN JavaScript (test infrastructure).

The SOR branch of the reference's JavaScript variant (index.html:741-774) is a
plain loop nest over typed arrays.  This script reads its text from the
reference at generation time, runs it under node on seeded right-hand sides
(p' pre-filled with 7: the branch zeroes it itself) and stores only the
numbers, as tests/golden/js_sor_*.npz plus a manifest.  No reference source is
written to the repository.  Each .npz holds in_rhs, out_solve,
out_residual_f64 and the iteration count `iters_run`.  The script does not
report that count: it is taken from the restatement (tests/_sor_lex_ref.py),
whose p' must equal the script's bit for bit -- which confirms the count, as a
further iteration would change p'.

The library compares (float)maxError with the float p_tol where the script
compares doubles (include/cfd.h): the generator asserts that no iteration of
any fixture lies where the two comparisons differ.

    python tests/golden/make_js_sor_golden.py [NAME ...]

Only fixtures whose .npz is missing are generated; the seed of a case is
5151 + its position in CASES, unless the case names a row of the seam tests'
table (tests/_sor_lex_cases.py), whose rhs recipe (seed, scale, rows kept) it
then takes.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _sor_lex_cases as seams   # noqa: E402
import _sor_lex_ref as ref   # noqa: E402

REF_HTML = "/root/reference/index.html"

# name -> (nx, ny, lx, ly, iterations, rhs scale, expected exit: None no early
# exit, 0 / 1 early exit at an even / odd count[, the seam table's case])
CASES = {
    "js_sor_16x4": (16, 4, 30.0, 10.0, 5, 100.0, None),
    "js_sor_16x5": (16, 5, 30.0, 10.0, 9, 100.0, None),
    "js_sor_24x7_p2": (24, 7, 24 / 128.0, 7 / 128.0, 50, 100.0, None),     # power-of-two spacing
    "js_sor_40x24_exit_even": (40, 24, 30.0, 10.0, 100, 1e-2, 0),
    "js_sor_32x12_exit_odd": (32, 12, 30.0, 10.0, 50, 1e-3, 1),
    "js_sor_72x66": (72, 66, 30.0, 10.0, 12, 100.0, None),                 # exactly one 64-row band
    "js_sor_72x67": (72, 67, 30.0, 10.0, 12, 100.0, None),                 # one band plus one row
    "js_sor_136x132": (136, 132, 30.0, 10.0, 6, 100.0, None),              # IEEE division, three bands
    "js_sor_128x128_p2": (128, 128, 1.0, 1.0, 6, 100.0, None),             # power-of-two spacing
    "js_sor_16x200": (16, 200, 30.0, 10.0, 10, 100.0, None),               # skew longer than a row
    "js_sor_64x48_it1": (64, 48, 4.0 / 3.0, 1.0, 1, 100.0, None),
    "js_sor_64x48_it2": (64, 48, 4.0 / 3.0, 1.0, 2, 100.0, None),
    # exits on more than one band (test_sor_lex_seams_cpu.py says what each is built for)
    "js_sor_24x132_exit_first_band": (24, 132, 30.0, 10.0, 100, 0.03, 1, "first_band"),
    "js_sor_24x132_exit_last_band": (24, 132, 30.0, 10.0, 100, 0.03, 1, "last_band_s0.03"),
    "js_sor_32x195_exit_it1": (32, 195, 30.0, 10.0, 100, 0.01, 1, "four_bands_first_iteration"),
    "js_sor_16x67_exit_one_row_band": (16, 67, 30.0, 10.0, 100, 0.01, 0,
                                       "one_row_band_tests_first_band"),
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
// the SOR branch with the script's own names; denom as index.html:181-183 forms it
const dx2 = dx * dx, dy2 = dy * dy;
const denom = 2 / dx2 + 2 / dy2;
const branch = new Function('pPrime', 'rhs', 'Nx', 'Ny', 'dx', 'dy', 'denom', 'iterations',
  'let lastPResidual;\n' + branchText + '\nreturn lastPResidual;');
const pPrime = new Float32Array(nx * ny).fill(7);   // the branch zeroes it itself
const res = branch(pPrime, rhs, nx, ny, dx, dy, denom, job.iterations);
fs.writeFileSync(dir + '/solve.bin', Buffer.from(pPrime.buffer));
fs.writeFileSync(dir + '/residual.json', JSON.stringify({ residual: res }));
"""


def extract():
    html = open(REF_HTML).read()
    c0 = html.index('if (currentPressureSolver === "sor") {')
    c0 = html.index("{", c0) + 1
    c1 = html.index('} else if (currentPressureSolver === "multigrid") {', c0)
    return html[c0:c1]


def main(only=()):
    unknown = [n for n in only if n not in CASES]
    if unknown:
        raise SystemExit(f"unknown fixture(s) {unknown}; CASES has {list(CASES)}")
    branch = extract()
    assert "pPrime.fill(0)" in branch and "sorOmega = 1.7" in branch
    assert "pressureTolerance = 1e-4" in branch
    mpath = os.path.join(HERE, "js_sor_manifest.json")
    if os.path.exists(mpath):
        manifest = json.load(open(mpath))
    else:
        manifest = {"generator": "tests/golden/make_js_sor_golden.py",
                    "source": "reference index.html:741-774 (SOR branch), executed by node " +
                              subprocess.run(["node", "--version"], capture_output=True,
                                             text=True).stdout.strip(),
                    "fixtures": {}}
    for k, (name, case) in enumerate(CASES.items()):
        nx, ny, lx, ly, iters, scale, exit_parity = case[:7]
        if only and name not in only:
            continue
        if os.path.exists(os.path.join(HERE, name + ".npz")):
            assert name in manifest["fixtures"], f"{name}.npz has no manifest entry"
            print(name, "kept")
            continue
        dx = np.float32(lx) / np.float32(nx)
        dy = np.float32(ly) / np.float32(ny)
        seed, rows = 5151 + k, None
        if len(case) > 7:
            row = seams.BY_NAME[case[7]]
            assert (row.nx, row.ny, row.lx, row.ly, row.iters, row.scale, row.tol, seams.P_TOL) == \
                (nx, ny, lx, ly, iters, scale, True, 1e-4), name
            seed, rows = row.seed, row.rows
        rhs = seams.make_rhs(nx, ny, seed, scale, rows)
        with tempfile.TemporaryDirectory() as d:
            for fn, txt in (("branch.js", branch), ("harness.js", HARNESS)):
                open(os.path.join(d, fn), "w").write(txt)
            rhs.tofile(os.path.join(d, "rhs.bin"))
            json.dump({"nx": nx, "ny": ny, "dx": float(dx), "dy": float(dy), "iterations": iters},
                      open(os.path.join(d, "job.json"), "w"))
            subprocess.run(["node", os.path.join(d, "harness.js"), os.path.join(d, "branch.js"),
                            os.path.join(d, "job.json"), d], check=True)
            solve = np.fromfile(os.path.join(d, "solve.bin"), np.float32)
            res = json.load(open(os.path.join(d, "residual.json")))["residual"]
        # the iteration count, from the restatement the script's p' confirms
        P, n_run, errs = ref.sor_lex_loop(rhs, nx, ny, dx, dy, iters, True, 1e-4)
        assert np.array_equal(P.reshape(-1).view(np.uint32), solve.view(np.uint32)), name
        assert errs[-1] == res, (name, errs[-1], res)
        assert not ref.slivers(errs), (name, "an iteration's maxError lies in the f32/f64 sliver")
        if exit_parity is None:
            assert n_run == iters and not errs[-1] < 1e-4, (name, n_run)
        else:
            assert n_run < iters and n_run % 2 == exit_parity, (name, n_run)
        np.savez_compressed(os.path.join(HERE, name + ".npz"), in_rhs=rhs, out_solve=solve,
                            out_residual_f64=np.array([res], np.float64),
                            iters_run=np.array([n_run], np.int64))
        manifest["fixtures"][name] = {"nx": nx, "ny": ny, "lx": lx, "ly": ly, "dx": float(dx),
                                      "dy": float(dy), "iterations": iters, "rhs_scale": scale,
                                      "iters_run": n_run, "seed": seed}
        if rows is not None:
            manifest["fixtures"][name]["rhs_rows"] = list(rows)
        print(name, "iterations run", n_run, "residual", res)
    json.dump(manifest, open(mpath, "w"), indent=1)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
