"""CPU: the restatement of the script's time step with the double pressure
residual and residualScalingEnabled (tests/_script_scaling_ref.py) against the
script's own numbers under node (tests/golden/js_update_scaling_*.npz,
make_js_update_scaling_golden.py), the four conditions the fixtures were chosen
for, and, with scaling off, its decisions against the script's on the existing
js_update_* fixtures.
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
sys.path.insert(0, GOLD)

import _script_scaling_ref as scal            # noqa: E402
import _script_step_ref as step               # noqa: E402
import _script_update_ref as upd              # noqa: E402
import make_js_update_scaling_golden as mk    # noqa: E402

SCAL = json.load(open(os.path.join(GOLD, "js_update_scaling_manifest.json")))
UPD = json.load(open(os.path.join(GOLD, "js_update_manifest.json")))


def _start(meta, fx):
    return dict(u=fx["start_u"], v=fx["start_v"], p=fx["start_p"], u_prev=fx["start_u_prev"],
                v_prev=fx["start_v_prev"], dt=meta["start_dt"], substep_count=meta["start_substep_count"],
                step_count=meta["start_step_count"])


def _case(meta):
    return dict(nx=meta["nx"], ny=meta["ny"], lx=meta["lx"], ly=meta["ly"],
                cyl=tuple(meta["cylinder"]) if meta["cylinder"] else None, scheme=meta["scheme"],
                solver=meta["solver"], profile=meta["profile"], target=meta["target"],
                dt_user=meta["dt_user"], K=meta["steps"])


_RESTATED = {}


def _restated(name):
    """(states, reports with slivers) of a scaling fixture, computed once."""
    if name not in _RESTATED:
        meta = SCAL["fixtures"][name]
        fx = np.load(os.path.join(GOLD, name + ".npz"))
        _RESTATED[name] = mk.restate(_case(meta), _start(meta, fx))
    return _RESTATED[name]


def test_fixture_set_is_the_makers():
    assert set(SCAL["fixtures"]) == set(mk.CASES)
    assert {m["solver"] for m in SCAL["fixtures"].values()} == {2, 4, 5}
    for m in SCAL["fixtures"].values():
        assert m["nx"] <= 40 and m["ny"] <= 12 and m["steps"] <= 6


@pytest.mark.parametrize("name", sorted(SCAL["fixtures"]))
def test_restatement_reproduces_node(name):
    meta = SCAL["fixtures"][name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    states, reps = _restated(name)
    nsub = meta["start_substep_count"]
    for s, (st, rep) in enumerate(zip(states, reps)):
        tag = f"{name} step {s}"
        for f in ("u", "v", "p"):
            assert step.bits_equal(st[f], fx["steps_" + f][s]), (tag, f)
        got = np.array([rep["residual_u"], rep["residual_v"], rep["residual_p"], rep["dt_next"],
                        rep["inlet_velocity"]])
        want = np.array([fx["res_u"][s], fx["res_v"][s], fx["res_p"][s], fx["dt"][s], fx["inlet"][s]])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (tag, got, want)
        assert rep["substeps_run"] == nsub and rep["substep_count_next"] == fx["substeps"][s], tag
        nsub = int(fx["substeps"][s])
    assert step.bits_equal(states[-1]["u_prev"], fx["final_u_prev"]), name
    assert step.bits_equal(states[-1]["v_prev"], fx["final_v_prev"]), name


def test_the_four_conditions_hold():
    mk.conditions({name: _restated(name)[1] for name in SCAL["fixtures"]})


@pytest.mark.parametrize("name", sorted(SCAL["fixtures"]))
def test_manifest_branches_are_the_restatements(name):
    assert SCAL["fixtures"][name]["branches"] == [r["branches"] for r in _restated(name)[1]]


@pytest.mark.parametrize("name", ["js_update_16x4_rest_first_jac", "js_update_16x5_rest_quick_sor",
                                  "js_update_24x7_ramp_second_mg_p2", "js_update_40x12_cyl_quick_jac"])
def test_double_decisions_without_scaling_are_the_scripts(name):
    """Scaling off, the double in use: the decisions are script_decisions of
    _script_update_ref, and node's substepCount and dt."""
    meta = UPD["fixtures"][name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    g = step.Grid(meta["nx"], meta["ny"], meta["lx"], meta["ly"], UPD["viscosity"],
                  tuple(meta["cylinder"]) if meta["cylinder"] else None)
    st = _start(meta, fx)
    ref_st = dict(st)
    for s in range(meta["steps"]):
        st, rep = scal.update(g, st, meta["scheme"], meta["profile"], meta["target"], meta["dt_user"],
                              meta["solver"], scaling=False)
        ref_st, ref_rep = upd.update(g, ref_st, meta["scheme"], meta["profile"], meta["target"],
                                     meta["dt_user"], meta["solver"])
        assert (rep["substep_count_next"], rep["dt_next"]) == ref_rep["script_decisions"], (name, s)
        assert (rep["substep_count_next"], rep["dt_next"]) == (fx["substeps"][s], fx["dt"][s]), (name, s)
        assert rep["residual_p"] == fx["res_p"][s], (name, s)
