"""Golden vectors for the tracer particles (cfd_tracers_*), produced by the
reference's OWN JavaScript (test infrastructure).

initTracers, updateTracers, getVelocityAt, injectTracers and
tracerInjectionInterval (index.html:1472-1543) are plain functions over typed
arrays and a list.  This script reads their text from the reference at
generation time, runs them under node at simulationLoop's cadence (:1231-1238)
on seeded f32 velocity fields and stores only the numbers, as
tests/golden/js_tracers_*.npz plus a manifest.  No reference source is written
to the repository.

Each .npz holds in_u, in_v (f32), the start list start_x / start_y / start_i
(initTracers' output followed by a few finite tracers outside the domain, which
exercise the clamps of :1504-1507), and the script's list after every step:
out_n[s] tracers, concatenated in out_x / out_y / out_i.  Step s (1-based) runs
updateTracers(dt) and then injectTracers() iff (step0 + s) % interval == 0.

Velocities are scaled so a tracer moves up to about two cells per step.  The
generator asserts, with counters kept by the restatement (tests/_tracers_ref.py,
itself asserted equal to node bit for bit on every list): over the set, and for
each fixture that claims it in the manifest, a tracer left through each of
x < 0, x > Lx, y < 0, y > Ly; an evaluation hit each of the four clamps; an
injection happened with survivors present; and the final list is neither empty
nor everything ever injected.

    python tests/golden/make_js_tracers_golden.py [NAME ...]

Only fixtures whose .npz is missing are generated; the seed of a case is
7171 + its position in CASES.
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
import _tracers_ref as ref   # noqa: E402

REF_HTML = "/root/reference/index.html"

# name -> (nx, ny, lx, ly, dt, step0, steps, drift): step0 = simulationStepCount
# before the first step; drift = mean of u in units of its random amplitude
CASES = {
    "js_tracers_16x5": (16, 5, 30.0, 10.0, 0.05, 94, 12, 0.3),
    "js_tracers_24x7": (24, 7, 24 / 128.0, 7 / 128.0, 0.004, 195, 12, 0.5),   # power-of-two spacing
    "js_tracers_64x48": (64, 48, 4.0 / 3.0, 1.0, 0.01, 97, 8, 0.6),
}
CLAIMS = ("exit_x_lo", "exit_x_hi", "exit_y_lo", "exit_y_hi", "clamp_i_lo", "clamp_i_hi",
          "clamp_j_lo", "clamp_j_hi", "inject_with_survivors")

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
function f64(name, n) {
  const b = fs.readFileSync(dir + '/' + name);
  return new Float64Array(b.buffer.slice(b.byteOffset, b.byteOffset + 8 * n));
}
const Nx = job.nx, Ny = job.ny;
const u = f32('u.bin', (Nx + 1) * Ny), v = f32('v.bin', Nx * (Ny + 1));
const extra = f64('extra.bin', 3 * job.n_extra);
// the script's functions with the script's own global names
const run = new Function('Nx', 'Ny', 'dx', 'dy', 'Lx', 'Ly', 'u', 'v', 'dt', 'job', 'extra',
  'let tracers = [];\n' + text + `
  initTracers();
  for (let k = 0; k < job.n_extra; k++)
    tracers.push({ x: extra[3 * k], y: extra[3 * k + 1], initialY: extra[3 * k + 2] });
  const lists = [tracers.map(t => [t.x, t.y, t.initialY])];
  let simulationStepCount = job.step0;
  for (let s = 0; s < job.steps; s++) {
    simulationStepCount++;
    updateTracers(dt);
    if (simulationStepCount % tracerInjectionInterval === 0) {
      injectTracers();
    }
    lists.push(tracers.map(t => [t.x, t.y, t.initialY]));
  }
  return { lists: lists, interval: tracerInjectionInterval };`);
const res = run(Nx, Ny, job.dx, job.dy, job.lx, job.ly, u, v, job.dt, job, extra);
const counts = res.lists.map(l => l.length);
const flat = new Float64Array(3 * counts.reduce((a, b) => a + b, 0));
let o = 0;
for (const l of res.lists) for (const t of l) { flat[o++] = t[0]; flat[o++] = t[1]; flat[o++] = t[2]; }
fs.writeFileSync(dir + '/lists.bin', Buffer.from(flat.buffer));
fs.writeFileSync(dir + '/counts.json', JSON.stringify({ counts: counts, interval: res.interval }));
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
    parts = [_function_text(html, n) for n in
             ("initTracers", "updateTracers", "getVelocityAt", "injectTracers")]
    m = re.search(r"const tracerInjectionInterval = \d+;", html)
    assert m, "tracerInjectionInterval not found"
    return "\n".join(parts + [m.group(0)])


def _extras(dom):
    """Finite tracers outside the domain (cfd_tracers_set accepts them): one
    beyond each wall, near enough that the extrapolating interpolation may
    bring it back, and one far outside; initialY numbers them."""
    dx, dy, lx, ly = dom.dx, dom.dy, dom.lx, dom.ly
    pts = [(-0.75 * dx, 0.4 * ly), (lx + 0.6 * dx, 0.6 * ly), (0.3 * lx, -0.8 * dy),
           (0.7 * lx, ly + 0.7 * dy), (-1e9 * lx, -1e9 * ly), (1e9 * lx, 1e9 * ly)]
    return np.array([(x, y, -1.0 - k) for k, (x, y) in enumerate(pts)], np.float64)


def main(only=()):
    unknown = [n for n in only if n not in CASES]
    if unknown:
        raise SystemExit(f"unknown fixture(s) {unknown}; CASES has {list(CASES)}")
    text = extract()
    assert "tracers.push({ x: x, y: y, initialY: y })" in text and "Math.floor(x / dx)" in text
    mpath = os.path.join(HERE, "js_tracers_manifest.json")
    if os.path.exists(mpath):
        manifest = json.load(open(mpath))
    else:
        manifest = {"generator": "tests/golden/make_js_tracers_golden.py",
                    "source": "reference index.html:1472-1543 (tracer functions) at the cadence "
                              "of :1231-1238, executed by node " +
                              subprocess.run(["node", "--version"], capture_output=True,
                                             text=True).stdout.strip(),
                    "fixtures": {}}
    for k, (name, (nx, ny, lx, ly, dt, step0, steps, drift)) in enumerate(CASES.items()):
        if only and name not in only:
            continue
        if os.path.exists(os.path.join(HERE, name + ".npz")):
            assert name in manifest["fixtures"], f"{name}.npz has no manifest entry"
            print(name, "kept")
            continue
        dom = ref.Domain(nx, ny, lx, ly)
        dt = float(np.float32(dt))
        rng = np.random.default_rng(7171 + k)
        # up to about two cells per step: |u| dt <= ~2 dx, |v| dt <= ~2 dy
        au, av = 2 * dom.dx / dt / (1 + abs(drift)), 2 * dom.dy / dt
        u = ((rng.uniform(-1, 1, (nx + 1) * ny) + drift) * au).astype(np.float32)
        v = (rng.uniform(-1, 1, nx * (ny + 1)) * av).astype(np.float32)
        extra = _extras(dom)
        with tempfile.TemporaryDirectory() as d:
            for fn, txt in (("tracers.js", text), ("harness.js", HARNESS)):
                open(os.path.join(d, fn), "w").write(txt)
            u.tofile(os.path.join(d, "u.bin"))
            v.tofile(os.path.join(d, "v.bin"))
            extra.tofile(os.path.join(d, "extra.bin"))
            json.dump({"nx": nx, "ny": ny, "dx": dom.dx, "dy": dom.dy, "lx": dom.lx, "ly": dom.ly,
                       "dt": dt, "step0": step0, "steps": steps, "n_extra": len(extra)},
                      open(os.path.join(d, "job.json"), "w"))
            subprocess.run(["node", os.path.join(d, "harness.js"), os.path.join(d, "tracers.js"),
                            os.path.join(d, "job.json"), d], check=True)
            flat = np.fromfile(os.path.join(d, "lists.bin"), np.float64).reshape(-1, 3)
            meta = json.load(open(os.path.join(d, "counts.json")))
        counts, interval = meta["counts"], meta["interval"]
        offs = np.concatenate([[0], np.cumsum(counts)])
        lists = [tuple(np.ascontiguousarray(flat[offs[s]:offs[s + 1], c]) for c in range(3))
                 for s in range(steps + 1)]
        # the restatement, step by step, against node; its counters give the claims
        tr = ref.init(dom)
        tr = tuple(np.concatenate([a, extra[:, c]]) for c, a in enumerate(tr))
        assert ref.bits_equal(tr, lists[0]), (name, "start list")
        clamps, exits = [0] * 4, [0] * 4
        injected, with_survivors = ny, False
        for s in range(1, steps + 1):
            tr = ref.advance(dom, u, v, dt, tr, clamps=clamps, exits=exits)
            if (step0 + s) % interval == 0:
                with_survivors |= tr[0].size > 0
                tr = ref.inject(dom, tr)
                injected += ny
            assert ref.bits_equal(tr, lists[s]), (name, "step", s)
        assert 0 < counts[-1] < injected, (name, counts[-1], injected)
        assert injected > ny, (name, "no injection crossed")
        facts = dict(zip(CLAIMS, [e > 0 for e in exits] + [c > 0 for c in clamps] + [with_survivors]))
        np.savez_compressed(os.path.join(HERE, name + ".npz"), in_u=u, in_v=v,
                            start_x=lists[0][0], start_y=lists[0][1], start_i=lists[0][2],
                            out_n=np.array(counts[1:], np.int64),
                            out_x=flat[offs[1]:, 0].copy(), out_y=flat[offs[1]:, 1].copy(),
                            out_i=flat[offs[1]:, 2].copy())
        manifest["fixtures"][name] = {"nx": nx, "ny": ny, "lx": lx, "ly": ly, "dx": dom.dx,
                                      "dy": dom.dy, "dt": dt, "step0": step0, "steps": steps,
                                      "interval": interval, "seed": 7171 + k,
                                      "claims": [c for c in CLAIMS if facts[c]],
                                      "exits": exits, "clamp_hits": clamps,
                                      "final_count": counts[-1], "injected": injected}
        print(name, "counts", counts, "exits", exits, "clamps", clamps)
    have = set()
    for fx in manifest["fixtures"].values():
        have |= set(fx["claims"])
    if not only and set(CASES) <= set(manifest["fixtures"]):
        assert have == set(CLAIMS), ("the set misses", sorted(set(CLAIMS) - have))
    json.dump(manifest, open(mpath, "w"), indent=1)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
