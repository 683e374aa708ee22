"""GPU: cfd_script_update, one updateSimulation() of the JavaScript variant
(index.html:261-363) on the device, bit for bit against the script itself run
by node (tests/golden/js_update_*.npz, make_js_update_golden.py): step by step
and through script_update_n, across a checkpoint, with the tracer tail, one
step on the default 800 x 264 channel against the restatement
(tests/_script_update_ref.py), and the rejections.
"""
import json
import os

import numpy as np
import pytest

import _script_step_ref as step
import _script_update_ref as upd
from _util import assert_bitwise

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
UPD = json.load(open(os.path.join(GOLD, "js_update_manifest.json")))
FX = UPD["fixtures"]


def _cfd():
    import cfdamd
    return cfdamd


def _model(c, meta, solver=None):
    solver = meta["solver"] if solver is None else solver
    cyl = c.Cylinder(*meta["cylinder"]) if meta["cylinder"] else None
    return c.Model(c.Grid(meta["nx"], meta["ny"], meta["lx"], meta["ly"], cyl),
                   c.SimulationParams(viscosity=UPD["viscosity"], pressure_solver=c.PressureSolver(solver),
                                      jacobi_iters=UPD["iters"], tol_enabled=True,
                                      p_tol=UPD["p_tol"][str(solver)]))


def _begin(m, meta, fx):
    m.set_state(u=fx["start_u"].ravel(), v=fx["start_v"].ravel(), p=fx["start_p"].ravel())
    m.script_begin(dict(dt=meta["start_dt"], substep_count=meta["start_substep_count"],
                        step_count=meta["start_step_count"], u_prev=fx["start_u_prev"],
                        v_prev=fx["start_v_prev"]))


def _cfg(c, meta):
    return (c.ScriptScheme(meta["scheme"]), meta["target"], meta["dt_user"], c.InletProfile(meta["profile"]))


def _check_report(tag, r, meta, fx, s, nsub_before):
    assert r.step_count == meta["start_step_count"] + s + 1, tag
    assert r.substeps_run == nsub_before, tag
    assert (r.residual_u, r.residual_v) == (fx["res_u"][s], fx["res_v"][s]), tag
    assert r.residual_p == float(np.float32(fx["res_p"][s])), tag
    assert (r.substep_count_next, r.dt_next, r.inlet_velocity) == \
        (fx["substeps"][s], fx["dt"][s], fx["inlet"][s]), tag


def _check_fields(tag, m, meta, fx, s):
    last = s == meta["steps"] - 1
    if meta["fields"] != "steps" and not last:
        return
    st = m.get_state()
    for f in ("u", "v", "p"):
        want = fx["steps_" + f][s] if meta["fields"] == "steps" else fx["final_" + f]
        assert_bitwise(f"{tag}: {f}", st[f], want.ravel())


def _check_final_state(tag, m, meta, fx):
    ss = m.script_state()
    assert_bitwise(f"{tag}: u_prev", ss["u_prev"], fx["final_u_prev"].ravel())
    assert_bitwise(f"{tag}: v_prev", ss["v_prev"], fx["final_v_prev"].ravel())
    assert (ss["dt"], ss["substep_count"], ss["step_count"]) == \
        (fx["dt"][-1], fx["substeps"][-1], meta["start_step_count"] + meta["steps"]), tag


def _check_tracers(tag, m, fx, s):
    off = int(fx["trc_n"][:s].sum())
    n = int(fx["trc_n"][s])
    x, y, iy = m.tracers()
    assert len(x) == n, tag
    for a, key in ((x, "trc_x"), (y, "trc_y"), (iy, "trc_i")):
        assert np.array_equal(np.asarray(a, np.float64).view(np.uint64),
                              fx[key][off:off + n].view(np.uint64)), (tag, key)


@pytest.mark.parametrize("name", sorted(FX))
def test_update_matches_reference_javascript(name):
    """Every fixture step by step, then again through script_update_n: the same
    fields, reports and final script_state."""
    c = _cfd()
    meta = FX[name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    K = meta["steps"]
    nsubs = [meta["start_substep_count"]] + [int(x) for x in fx["substeps"][:-1]]
    # one call per step
    m = _model(c, meta)
    _begin(m, meta, fx)
    if meta["tracers"]:
        m.tracers_enable(4096, meta["tracers"])
    rust0 = m.get_state()
    for s in range(K):
        r = m.script_update(*_cfg(c, meta))
        _check_report(f"{name} step {s}", r, meta, fx, s, nsubs[s])
        _check_fields(f"{name} step {s}", m, meta, fx, s)
        if meta["tracers"]:
            _check_tracers(f"{name} step {s}", m, fx, s)
    _check_final_state(name, m, meta, fx)
    rust1 = m.get_state()
    for key in ("dt", "simulation_time", "simulation_step", "last_u_residual", "last_v_residual"):
        assert rust0[key] == rust1[key], f"{name}: the Rust path's {key} moved"
    single = m.get_state()
    m.close()
    # one call for all steps
    m = _model(c, meta)
    _begin(m, meta, fx)
    if meta["tracers"]:
        m.tracers_enable(4096, meta["tracers"])
    reps = m.script_update_n(K, *_cfg(c, meta))
    assert len(reps) == K
    for s, r in enumerate(reps):
        _check_report(f"{name} update_n step {s}", r, meta, fx, s, nsubs[s])
    _check_fields(f"{name} update_n", m, meta, fx, K - 1)
    _check_final_state(f"{name} update_n", m, meta, fx)
    if meta["tracers"]:
        _check_tracers(f"{name} update_n", m, fx, K - 1)
    st = m.get_state()
    for f in ("u", "v", "p", "p_prime", "rhs", "u_star", "v_star"):
        assert_bitwise(f"{name}: {f}, one call per step vs update_n", st[f], single[f])
    m.close()


@pytest.mark.parametrize("name", ["js_update_16x5_rest_quick_sor", "js_update_40x12_cyl_quick_jac"])
def test_checkpoint_resumes_bitwise(name):
    """k steps, script_state + get_state into a fresh model, the remaining steps."""
    c = _cfd()
    meta = FX[name]
    fx = np.load(os.path.join(GOLD, name + ".npz"))
    K, k = meta["steps"], 3
    a = _model(c, meta)
    _begin(a, meta, fx)
    a.script_update_n(k, *_cfg(c, meta))
    ss, st = a.script_state(), a.get_state()
    a.close()
    b = _model(c, meta)
    b.set_state(u=st["u"], v=st["v"], p=st["p"])
    b.script_begin(ss)
    nsubs = [int(x) for x in fx["substeps"]]
    for s in range(k, K):
        r = b.script_update(*_cfg(c, meta))
        _check_report(f"{name} resumed step {s}", r, meta, fx, s, nsubs[s - 1])
        _check_fields(f"{name} resumed step {s}", b, meta, fx, s)
    _check_final_state(f"{name} resumed", b, meta, fx)
    b.close()


def test_one_step_on_the_default_channel_matches_restatement():
    """800 x 264 with the cylinder, substep_count 2, a seeded state at step 7,
    the script's default solver; dt above the CFL value, so dt_next is
    0.5 min(dx, dy) / maxVel."""
    c = _cfd()
    nx, ny, lx, ly, cyl = 800, 264, 30.0, 10.0, (7.5, 5.0, 0.75)
    g = step.Grid(nx, ny, lx, ly, UPD["viscosity"], cyl)
    rng = np.random.default_rng(20260)
    y = (np.arange(ny) + 0.5) / ny
    u = ((4 * y * (1 - y))[:, None] + 0.02 * rng.uniform(-1, 1, (ny, nx + 1))).astype(np.float32)
    v = (0.02 * rng.uniform(-1, 1, (ny + 1, nx))).astype(np.float32)
    p = rng.uniform(-1, 1, (ny, nx)).astype(np.float32)
    st0 = dict(u=u, v=v, p=p, u_prev=(u * np.float32(0.99)).astype(np.float32),
               v_prev=(v * np.float32(0.99)).astype(np.float32), dt=0.02, substep_count=2, step_count=7)
    want, rep = upd.update(g, st0, step.QUICK, step.PARABOLIC, 1.0, 0.5, 5)
    # the new dt is the CFL quotient itself: the device's max(|u|, |v|) is checked by value
    assert "dt_is_cfl" in rep["branches"] and np.isfinite(want["u"]).all()
    meta = dict(nx=nx, ny=ny, lx=lx, ly=ly, cylinder=cyl, solver=5)
    m = _model(c, meta)
    m.set_state(u=u.ravel(), v=v.ravel(), p=p.ravel())
    m.script_begin(st0)
    r = m.script_update(c.ScriptScheme.Quick, 1.0, 0.5, c.InletProfile.Parabolic)
    st = m.get_state()
    for f in ("u", "v", "p"):
        assert_bitwise(f"800x264: {f}", st[f], want[f].ravel())
    assert (r.residual_u, r.residual_v, r.residual_p) == (rep["residual_u"], rep["residual_v"], rep["residual_p"])
    assert (r.substeps_run, r.substep_count_next, r.dt_next, r.inlet_velocity, r.step_count) == \
        (2, rep["substep_count_next"], rep["dt_next"], rep["inlet_velocity"], 8)
    ss = m.script_state()
    assert_bitwise("800x264: u_prev", ss["u_prev"], want["u_prev"].ravel())
    assert_bitwise("800x264: v_prev", ss["v_prev"], want["v_prev"].ravel())
    m.close()


def _raises(c, code, word, fn):
    with pytest.raises(c.CfdError) as e:
        fn()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_rejections():
    c = _cfd()
    grid = c.Grid(32, 16, 30.0, 10.0)
    ok = (c.ScriptScheme.First, 1.0, 0.5)
    m = c.Model(grid, c.SimulationParams(pressure_solver=c.PressureSolver.JacobiScript))
    _raises(c, -4, "cfd_script_begin", lambda: m.script_update(*ok))            # before begin
    _raises(c, -4, "cfd_script_begin", lambda: m.script_state())
    m.script_begin()
    for bad, word in (((3, 1.0, 0.5), "scheme"), ((0, 1.0, 0.5, 2), "profile"),
                      ((0, 1.0, 0.0), "dt_user"), ((0, 1.0, float("nan")), "dt_user"),
                      ((0, float("inf"), 0.5), "target_inlet_velocity")):
        _raises(c, -1, word, lambda bad=bad: m.script_update(*bad))
    _raises(c, -1, "n must be", lambda: m.script_update_n(0, *ok))
    _raises(c, -1, "substep_count", lambda: m.set_script_state(dict(dt=0.1, substep_count=21)))
    _raises(c, -1, "dt", lambda: m.set_script_state(dict(dt=float("inf"), substep_count=2)))
    assert m.script_state()["step_count"] == 0
    m.close()
    for solver in (0, 1):
        m = c.Model(grid, c.SimulationParams(pressure_solver=c.PressureSolver(solver)))
        _raises(c, -1, "pressure_solver", lambda: m.script_begin())
        _raises(c, -1, "pressure_solver", lambda: m.script_update(*ok))
        m.close()
    m = c.Model(c.cavity_grid(32), c.SimulationParams.cavity(100.0, 50, pressure_solver=c.PressureSolver.Multigrid))
    _raises(c, -1, "channel", lambda: m.script_begin())
    _raises(c, -1, "channel", lambda: m.script_update(*ok))
    m.close()


def test_sharded_model_rejects_the_update():
    c = _cfd()
    from _slabs import run_slabs

    def fn(m, rank):
        out = []
        for call in (m.script_begin, lambda: m.script_update(c.ScriptScheme.First, 1.0, 0.5)):
            try:
                call()
                out.append((0, ""))
            except c.CfdError as e:
                out.append((e.code, str(e)))
        return out

    res = run_slabs(2, c.Grid(64, 64, 2.0, 2.0),
                    c.SimulationParams(pressure_solver=c.PressureSolver.Multigrid), None, None, fn,
                    join=120.0)
    for calls in res:
        for code, msg in calls:
            assert code == -1 and "one domain" in msg, (code, msg)


def test_nonfinite_is_returned_not_a_fault():
    """A start state holding an Inf: the update returns CFD_ENONFINITE with the
    report filled, and stays refused until script_begin."""
    c = _cfd()
    nx, ny = 32, 16
    g = step.Grid(nx, ny, 30.0, 10.0, UPD["viscosity"], None)
    u = np.full((ny, nx + 1), 0.5, np.float32)
    u[ny // 2, 0] = np.inf   # an inlet face: the boundary pass overwrites it, so |u - uOld| is Inf there
    v = np.zeros((ny + 1, nx), np.float32)
    p = np.zeros((ny, nx), np.float32)
    st0 = dict(u=u, v=v, p=p, u_prev=u.copy(), v_prev=v.copy(), dt=0.1, substep_count=1, step_count=0)
    _, rep = upd.update(g, st0, step.FIRST, step.UNIFORM, 1.0, 0.5, 5)
    vals = [rep["residual_u"], rep["residual_v"], rep["residual_p"], rep["dt_next"]]
    assert not np.isfinite(vals).all() or not rep["dt_next"] > 0, "the start must blow the step up"
    m = _model(c, dict(nx=nx, ny=ny, lx=30.0, ly=10.0, cylinder=None, solver=5))
    m.set_state(u=u.ravel(), v=v.ravel(), p=p.ravel())
    m.script_begin(dict(dt=0.1, substep_count=1, step_count=0))
    with pytest.raises(c.CfdError) as e:
        m.script_update(c.ScriptScheme.First, 1.0, 0.5)
    assert e.value.code == c.CFD_ENONFINITE
    (r,) = e.value.reports
    got = [r.residual_u, r.residual_v, r.residual_p, r.dt_next]
    assert np.array_equal(np.array(got).view(np.uint64), np.array(vals).view(np.uint64))
    _raises(c, c.CFD_ENONFINITE, "cfd_script_begin", lambda: m.script_update(c.ScriptScheme.First, 1.0, 0.5))
    m.set_state(u=np.zeros_like(u).ravel(), v=v.ravel(), p=p.ravel())
    m.script_begin()
    assert m.script_update(c.ScriptScheme.First, 1.0, 0.5).step_count == 1
    m.close()
