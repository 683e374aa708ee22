"""CPU: the script's Jacobi solver (pressure_solver 5) and the script's time
step (cfd_script_update) without a device.

* the restatements (tests/_jacobi_script_ref.py, tests/_script_update_ref.py)
  reproduce every committed fixture of the script's own numbers under node
  (tests/golden/js_jac_*.npz, js_jacstep_*.npz, js_update_*.npz) bit for bit;
* the manifests and the .npz files agree;
* the new entry points are declared and exported, reject null handles with
  CFD_EINVAL, and pressure_solver 5 on a sharded creation is CFD_EINVAL before
  any device call.
"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import _jacobi_script_ref as jac
import _script_step_ref as step
import _script_update_ref as upd
import _tracers_ref as trc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
JAC = json.load(open(os.path.join(GOLD, "js_jac_manifest.json")))
JSTEP = json.load(open(os.path.join(GOLD, "js_jacstep_manifest.json")))
UPD = json.load(open(os.path.join(GOLD, "js_update_manifest.json")))
NEW = ("cfd_script_begin", "cfd_script_get_state", "cfd_script_set_state", "cfd_script_update",
       "cfd_script_update_n")


def _bits(a, b):
    return step.bits_equal(np.ravel(a), np.ravel(b))


@pytest.mark.parametrize("name", sorted(JAC["fixtures"]))
def test_jacobi_restatement_reproduces_node(name):
    meta = JAC["fixtures"][name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    P, n, errs = jac.jacobi_script(fx["in_rhs"], meta["nx"], meta["ny"], meta["dx"], meta["dy"],
                                   meta["iterations"], True, JAC["p_tol"])
    assert _bits(P, fx["out_solve"])
    assert n == int(fx["iters_run"][0]) == meta["iters_run"]
    assert errs == list(fx["max_errors_f64"])
    assert not jac.slivers(errs, JAC["p_tol"])
    if n == meta["iterations"]:   # never met: the fixed-count solve is the same
        P2, n2, _ = jac.jacobi_script(fx["in_rhs"], meta["nx"], meta["ny"], meta["dx"], meta["dy"],
                                      meta["iterations"], False)
        assert n2 == n and _bits(P2, P)


def test_jacobi_manifest_covers_the_cases():
    fxs = JAC["fixtures"]
    assert JAC["p_tol"] == 1e-6
    assert {(16, 4), (16, 5), (24, 7)} <= {(f["nx"], f["ny"]) for f in fxs.values()}
    exits = [f["iters_run"] for f in fxs.values() if f["iters_run"] < f["iterations"]]
    assert any(n % 2 == 1 and n > 1 for n in exits) and any(n % 2 == 0 for n in exits)
    assert any(f["iterations"] == 1 for f in fxs.values())
    assert any(f["rhs_scale"] == 0 and f["iters_run"] == 1 for f in fxs.values())
    # the kernel's seams: 124 columns per wave, 4 interior rows per wave, 16 per workgroup
    assert any(f["nx"] > 124 for f in fxs.values())
    assert any(4 < f["ny"] - 2 <= 16 for f in fxs.values()) and any(f["ny"] - 2 > 16 for f in fxs.values())
    for name in fxs:
        assert os.path.getsize(os.path.join(GOLD, name + ".npz")) < 200 * 1024


@pytest.mark.parametrize("name", sorted(JSTEP["fixtures"]))
def test_substep_with_the_jacobi_solve_reproduces_node(name):
    meta = JSTEP["fixtures"][name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    g = step.Grid(meta["nx"], meta["ny"], meta["lx"], meta["ly"], JSTEP["viscosity"], meta["cylinder"])
    us, vs, rhs = step.predict(g, fx["in_u"], fx["in_v"], meta["dt_sub"], meta["scheme"])
    pp, res = upd.solve(g, rhs, 5)
    u, v, p = step.correct(g, us, vs, pp, fx["in_p"], meta["dt_sub"], meta["inlet_velocity"],
                           meta["profile"])
    for nm, a in (("u_star", us), ("v_star", vs), ("rhs", rhs), ("p_prime", pp), ("u", u), ("v", v),
                  ("p", p)):
        assert _bits(a, fx[nm]), nm
    assert res == float(fx["lastPResidual"][0])


def _start(meta, fx):
    return dict(u=fx["start_u"], v=fx["start_v"], p=fx["start_p"], u_prev=fx["start_u_prev"],
                v_prev=fx["start_v_prev"], dt=meta["start_dt"],
                substep_count=meta["start_substep_count"], step_count=meta["start_step_count"])


@pytest.mark.parametrize("name", sorted(UPD["fixtures"]))
def test_update_restatement_reproduces_node(name):
    meta = UPD["fixtures"][name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    g = step.Grid(meta["nx"], meta["ny"], meta["lx"], meta["ly"], UPD["viscosity"], meta["cylinder"])
    st = _start(meta, fx)
    dom = trc.Domain(g.nx, g.ny, g.lx, g.ly)
    tr = trc.init(dom) if meta["tracers"] else None
    toff = 0
    for s in range(meta["steps"]):
        st, rep = upd.update(g, st, meta["scheme"], meta["profile"], meta["target"], meta["dt_user"],
                             meta["solver"])
        assert (rep["residual_u"], rep["residual_v"], rep["residual_p_f64"]) == \
            (fx["res_u"][s], fx["res_v"][s], fx["res_p"][s]), s
        assert (rep["substep_count_next"], rep["dt_next"], rep["inlet_velocity"]) == \
            (fx["substeps"][s], fx["dt"][s], fx["inlet"][s]), s
        assert rep["script_decisions"] == (rep["substep_count_next"], rep["dt_next"]), s
        assert rep["branches"] == meta["branches"][s]
        if meta["fields"] == "steps":
            for f in ("u", "v", "p"):
                assert _bits(st[f], fx["steps_" + f][s]), (s, f)
        if tr is not None:
            tr = trc.step(dom, st["u"].ravel(), st["v"].ravel(), st["dt"], st["step_count"],
                          meta["tracers"], tr)
            n = int(fx["trc_n"][s])
            for c, key in enumerate(("trc_x", "trc_y", "trc_i")):
                assert trc.bits_equal(tr[c], fx[key][toff:toff + n]), (s, key)
            toff += n
    if meta["fields"] == "final":
        for f in ("u", "v", "p"):
            assert _bits(st[f], fx["final_" + f]), f
    assert _bits(st["u_prev"], fx["final_u_prev"]) and _bits(st["v_prev"], fx["final_v_prev"])


def test_update_manifest_covers_every_branch():
    fxs = UPD["fixtures"].values()
    seen = {b for fx in fxs for bs in fx["branches"] for b in bs}
    assert seen == {"step0", "extrapolated", "ramp", "ramp_done", "sub_grown", "sub_capped",
                    "sub_halved", "sub_floored", "sub_unchanged", "maxvel_zero", "dt_cfl", "dt_user",
                    "dt_limited", "dt_is_cfl", "cfl_from_u", "cfl_from_v"}
    assert {fx["scheme"] for fx in fxs} == {0, 1, 2} and {fx["profile"] for fx in fxs} == {0, 1}
    assert {fx["solver"] for fx in fxs} == {2, 4, 5}
    assert {fx["cylinder"] is None for fx in fxs} == {True, False}
    assert [fx["tracers"] for fx in fxs if fx["tracers"]] == [2]
    assert any(fx["start_step_count"] == 998 for fx in fxs)
    # max(|u|, |v|) reaches a result by value: steps whose dt is the CFL quotient itself,
    # neither dt_user nor 1.1 x the previous dt, with dx < dy and with dy < dx
    free = {}
    for name, fx in UPD["fixtures"].items():
        dts = [fx["start_dt"]] + list(np.load(os.path.join(GOLD, name + ".npz"))["dt"])
        n = sum(1 for a, b in zip(dts, dts[1:]) if b != fx["dt_user"] and b != a * 1.1)
        assert n == sum("dt_is_cfl" in bs for bs in fx["branches"]), name
        if n:
            free[name] = fx["lx"] / fx["nx"] < fx["ly"] / fx["ny"]
    assert set(free.values()) == {True, False}, free
    for name in UPD["fixtures"]:
        assert os.path.getsize(os.path.join(GOLD, name + ".npz")) < 200 * 1024


# ---- host-only ABI checks
def test_new_symbols_are_declared_and_exported():
    from cfdamd import _lib
    L = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cfd.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(rf"\b{s}\s*\(", text), s
        assert s in _lib.EXPORTS and hasattr(L, s), s
    assert re.search(r"CFD_SOLVER_JACOBI_SCRIPT\s*=\s*5\b", text)
    import cfdamd
    assert int(cfdamd.PressureSolver.JacobiScript) == 5
    assert L.cfd_abi_version() == 1


def test_null_handles_are_einval():
    from cfdamd import _lib
    L = _lib.load()
    cfg = _lib.CfdScriptConfig(0, 0, 1.0, 0.5)
    rep = _lib.CfdScriptReport()
    st = _lib.CfdScriptState()
    assert L.cfd_script_begin(None, None) == _lib.CFD_EINVAL
    assert L.cfd_script_begin(None, C.byref(st)) == _lib.CFD_EINVAL
    assert L.cfd_script_get_state(None, C.byref(st)) == _lib.CFD_EINVAL
    assert L.cfd_script_set_state(None, C.byref(st)) == _lib.CFD_EINVAL
    assert L.cfd_script_update(None, C.byref(cfg), C.byref(rep)) == _lib.CFD_EINVAL
    assert L.cfd_script_update_n(None, C.byref(cfg), 3, None) == _lib.CFD_EINVAL
    assert b"null model" in L.cfd_last_error()
    assert rep.step_count == 0


def test_sharded_creation_with_solver_5_is_einval_before_the_device():
    import cfdamd as c
    hub = c.LocalHub(2)
    try:
        for kw in (dict(local_hub=hub), dict(unique_id=bytes(128))):
            with pytest.raises(c.CfdError) as e:
                c.Model(c.Grid(64, 64, 1.0, 1.0),
                        c.SimulationParams(pressure_solver=c.PressureSolver.JacobiScript),
                        n_ranks=2, rank=0, **kw)
            assert e.value.code == -1 and "pressure_solver 5" in str(e.value)
    finally:
        hub.close()
