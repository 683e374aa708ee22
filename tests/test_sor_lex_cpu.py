"""CPU: the restatement of the script-order SOR (tests/_sor_lex_ref.py) is
pinned to the reference script's own results under node
(tests/golden/js_sor_*.npz, make_js_sor_golden.py), and its anti-diagonal
numpy form to the plain loops.  The GPU tests (test_gpu_sor_lex.py) compare
pressure_solver 4 with the fixtures directly and with the anti-diagonal form
on larger grids."""
import json
import os

import numpy as np
import pytest

import _sor_lex_ref as ref
from _util import assert_bitwise

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
JS = json.load(open(os.path.join(GOLD, "js_sor_manifest.json")))["fixtures"]

REQUIRED = {"js_sor_16x4", "js_sor_16x5", "js_sor_24x7_p2", "js_sor_40x24_exit_even",
            "js_sor_32x12_exit_odd", "js_sor_72x66", "js_sor_72x67", "js_sor_136x132",
            "js_sor_128x128_p2", "js_sor_16x200", "js_sor_64x48_it1", "js_sor_64x48_it2",
            # exits on more than one band (tests/_sor_lex_cases.py)
            "js_sor_24x132_exit_first_band", "js_sor_24x132_exit_last_band",
            "js_sor_32x195_exit_it1", "js_sor_16x67_exit_one_row_band"}


def test_fixture_set_is_complete():
    assert REQUIRED <= set(JS)
    for name in JS:
        assert os.path.getsize(os.path.join(GOLD, name + ".npz")) < 400 * 1024
    assert JS["js_sor_40x24_exit_even"]["iters_run"] % 2 == 0
    assert JS["js_sor_40x24_exit_even"]["iters_run"] < JS["js_sor_40x24_exit_even"]["iterations"]
    assert JS["js_sor_32x12_exit_odd"]["iters_run"] % 2 == 1
    assert JS["js_sor_32x12_exit_odd"]["iters_run"] < JS["js_sor_32x12_exit_odd"]["iterations"]


@pytest.mark.parametrize("name", sorted(JS))
def test_loop_form_matches_reference_javascript(name):
    meta = JS[name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    nx, ny = meta["nx"], meta["ny"]
    P, n, errs = ref.sor_lex_loop(fx["in_rhs"], nx, ny, meta["dx"], meta["dy"], meta["iterations"])
    assert_bitwise(f"{name}: p'", P.reshape(-1), fx["out_solve"])
    assert errs[-1] == fx["out_residual_f64"][0]
    assert n == int(fx["iters_run"][0]) == meta["iters_run"]
    # the library's float exit test and the script's double one agree on every iteration
    assert not ref.slivers(errs)


@pytest.mark.parametrize("name", sorted(n for n in JS if JS[n]["nx"] * JS[n]["ny"] <= 72 * 67))
@pytest.mark.parametrize("tol", [True, False])
def test_diagonal_form_matches_loop_form(name, tol):
    meta = JS[name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    nx, ny = meta["nx"], meta["ny"]
    iters = min(meta["iterations"], 20) if not tol else meta["iterations"]
    a = ref.sor_lex_loop(fx["in_rhs"], nx, ny, meta["dx"], meta["dy"], iters, tol)
    b = ref.sor_lex_diag(fx["in_rhs"], nx, ny, meta["dx"], meta["dy"], iters, tol)
    assert_bitwise(f"{name} tol={tol}: p'", b[0].reshape(-1), a[0].reshape(-1))
    assert a[1] == b[1] and a[2] == b[2]


def test_diagonal_form_matches_fixture_on_three_bands():
    """The anti-diagonal form against the script itself on the largest fixtures."""
    for name in ("js_sor_136x132", "js_sor_128x128_p2"):
        meta = JS[name]
        fx = np.load(os.path.join(GOLD, name + ".npz"))
        P, n, errs = ref.sor_lex_diag(fx["in_rhs"], meta["nx"], meta["ny"], meta["dx"], meta["dy"],
                                      meta["iterations"])
        assert_bitwise(name, P.reshape(-1), fx["out_solve"])
        assert errs[-1] == fx["out_residual_f64"][0] and n == meta["iters_run"]


def test_sharded_models_refuse_script_order_sor():
    """cfd_create_sharded* with pressure_solver 4: CFD_EINVAL before any device call."""
    import cfdamd as c
    hub = c.LocalHub(2)
    try:
        with pytest.raises(c.CfdError) as e:
            c.Model(c.Grid(64, 64, 1.0, 1.0),
                    c.SimulationParams(pressure_solver=c.PressureSolver.SorLex),
                    n_ranks=2, rank=0, local_hub=hub)
        assert e.value.code == -1 and "one domain" in str(e.value)
        with pytest.raises(c.CfdError) as e:
            c.Model(c.Grid(64, 64, 1.0, 1.0),
                    c.SimulationParams(pressure_solver=c.PressureSolver.SorLex),
                    n_ranks=2, rank=1, unique_id=b"\0" * 128)
        assert e.value.code == -1 and "one domain" in str(e.value)
    finally:
        hub.close()
