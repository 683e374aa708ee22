"""The node-generated substep fixtures (tests/golden/js_step_*.npz, written by
tests/golden/make_js_script_step_golden.py), loaded for the CPU and GPU tests."""
import json
import os

import numpy as np

import _script_step_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MANIFEST = json.load(open(os.path.join(GOLDEN, "js_step_manifest.json")))
FIXTURES = sorted(MANIFEST["fixtures"])
FIELDS = ("in_u", "in_v", "in_p", "u_star", "v_star", "rhs", "p_prime", "u", "v", "p")


def load_fixture(name):
    """(meta, restatement grid, arrays by name)"""
    meta = MANIFEST["fixtures"][name]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = ref.Grid(meta["nx"], meta["ny"], meta["lx"], meta["ly"], MANIFEST["viscosity"], meta["cylinder"])
    return meta, g, {k: z[k] for k in FIELDS + ("lastPResidual",)}
