"""The node-generated tracer fixtures (tests/golden/js_tracers_*.npz, written by
tests/golden/make_js_tracers_golden.py), loaded for the CPU and GPU tests."""
import json
import os

import numpy as np

import _tracers_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "js_tracers_manifest.json")))
FIXTURES = sorted(MANIFEST["fixtures"])
CLAIMS = ("exit_x_lo", "exit_x_hi", "exit_y_lo", "exit_y_hi", "clamp_i_lo", "clamp_i_hi",
          "clamp_j_lo", "clamp_j_hi", "inject_with_survivors")


def load_fixture(name):
    """(meta, domain, u, v, start list, [script's list after step 1, 2, ...])"""
    meta = MANIFEST["fixtures"][name]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    dom = ref.Domain(meta["nx"], meta["ny"], meta["lx"], meta["ly"])
    offs = np.concatenate([[0], np.cumsum(z["out_n"])])
    lists = [tuple(np.ascontiguousarray(z[k][offs[s]:offs[s + 1]]) for k in ("out_x", "out_y", "out_i"))
             for s in range(len(z["out_n"]))]
    return meta, dom, z["in_u"], z["in_v"], (z["start_x"], z["start_y"], z["start_i"]), lists
