"""GPU: the script's substep on the device (cfd_script_piso_step,
cfd_script_phase; cfd_script_step.hip) against the script's own fields under
node (tests/golden/js_step_*.npz) and the restatement
(tests/_script_step_ref.py).

Every comparison is bitwise on the u32 views of the fields; there are no
tolerances.  No test skips when a symbol is missing."""
import numpy as np
import pytest

import _script_step_ref as ref
from _util import assert_bitwise
from _script_step_golden import FIXTURES, MANIFEST, load_fixture

pytestmark = pytest.mark.gpu

FLOW = ("u", "v", "p", "u_star", "v_star", "p_prime", "rhs")
SCALARS = ("dt", "simulation_time", "simulation_step", "last_p_residual", "last_u_residual",
           "last_v_residual", "jacobi_sweeps_total")


def _model(g, solver, **kw):
    import cfdamd
    cyl = cfdamd.Cylinder(*g.cyl) if g.cyl else None
    params = cfdamd.SimulationParams(viscosity=g.nu, pressure_solver=cfdamd.PressureSolver(solver),
                                     jacobi_iters=MANIFEST["iters"], tol_enabled=True,
                                     p_tol=MANIFEST["p_tol"], **kw)
    return cfdamd.Model(cfdamd.Grid(g.nx, g.ny, g.lx, g.ly, cyl), params)


def _args(meta):
    return (meta["dt_sub"], meta["scheme"], meta["inlet_velocity"], meta["profile"])


# ---------------------------------------------------------------- node fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_predict_phase_matches_reference_javascript(name):
    import cfdamd
    meta, g, a = load_fixture(name)
    m = _model(g, meta["solver"])
    try:
        m.set_state(u=a["in_u"], v=a["in_v"], p=a["in_p"])
        m.script_phase(cfdamd.ScriptPhase.Predict, *_args(meta))
        st = m.get_state()
        for f in ("u_star", "v_star", "rhs"):
            assert_bitwise(f"{name}:{f}", st[f].reshape(a[f].shape), a[f])
        for f, src in (("u", "in_u"), ("v", "in_v"), ("p", "in_p")):   # inputs untouched
            assert_bitwise(f"{name}:{f}", st[f].reshape(a[src].shape), a[src])
    finally:
        m.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_correct_phase_matches_reference_javascript(name):
    import cfdamd
    meta, g, a = load_fixture(name)
    m = _model(g, meta["solver"])
    try:
        m.set_state(u=a["in_u"], v=a["in_v"], p=a["in_p"], u_star=a["u_star"], v_star=a["v_star"],
                    p_prime=a["p_prime"], rhs=a["rhs"])
        m.script_phase(cfdamd.ScriptPhase.Correct, *_args(meta))
        st = m.get_state()
        for f in ("u", "v", "p"):
            assert_bitwise(f"{name}:{f}", st[f].reshape(a[f].shape), a[f])
    finally:
        m.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_substep_matches_reference_javascript(name):
    meta, g, a = load_fixture(name)
    m = _model(g, meta["solver"])
    try:
        m.set_state(u=a["in_u"], v=a["in_v"], p=a["in_p"])
        before = m.get_state()
        m.script_piso_step(*_args(meta))
        st = m.get_state()
        for f in FLOW:
            assert_bitwise(f"{name}:{f}", st[f].reshape(a[f].shape), a[f])
        assert np.float32(st["last_p_residual"]) == np.float32(a["lastPResidual"][0]), name
        grown = st["jacobi_sweeps_total"] - before["jacobi_sweeps_total"]
        assert grown == (meta["sor_iterations"] if meta["solver"] == 4 else 1), (name, grown)
        for k in ("dt", "simulation_time", "simulation_step", "last_u_residual", "last_v_residual"):
            assert np.asarray(st[k]).tobytes() == np.asarray(before[k]).tobytes(), (name, k)
    finally:
        m.close()


# ------------------------------------------------- restatement, device's own p'
def _random_state(g, seed, dt_sub, cfl=0.6):
    rng = np.random.default_rng(seed)
    u = (rng.uniform(-1, 1, (g.ny, g.nx + 1)) * cfl * g.dx / dt_sub).astype(np.float32)
    v = (rng.uniform(-1, 1, (g.ny + 1, g.nx)) * cfl * g.dy / dt_sub).astype(np.float32)
    p = rng.uniform(-1, 1, (g.ny, g.nx)).astype(np.float32)
    for z in (np.float32(0.0), np.float32(-0.0)):
        for _ in range(8):
            j, i = int(rng.integers(0, g.ny)), int(rng.integers(0, g.nx))
            u[j:j + 3, i:i + 3] = z
            v[j:j + 3, i:i + 3] = z
    return u, v, p


def _check_against_restatement(tag, g, m, before, st, dt_sub, scheme, inlet, profile):
    """st = the model's state after one substep from `before`."""
    sh = {"u": (g.ny, g.nx + 1), "v": (g.ny + 1, g.nx), "p": (g.ny, g.nx)}
    us, vs, rhs = ref.predict(g, before["u"], before["v"], dt_sub, scheme)
    assert_bitwise(f"{tag}:u_star", st["u_star"].reshape(sh["u"]), us)
    assert_bitwise(f"{tag}:v_star", st["v_star"].reshape(sh["v"]), vs)
    assert_bitwise(f"{tag}:rhs", st["rhs"].reshape(sh["p"]), rhs)
    u, v, p = ref.correct(g, us, vs, st["p_prime"], before["p"], dt_sub, inlet, profile)
    assert_bitwise(f"{tag}:u", st["u"].reshape(sh["u"]), u)
    assert_bitwise(f"{tag}:v", st["v"].reshape(sh["v"]), v)
    assert_bitwise(f"{tag}:p", st["p"].reshape(sh["p"]), p)
    assert st["p_prime"].any(), tag


@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_default_channel_matches_restatement(scheme):
    g = ref.Grid(800, 264, 30.0, 10.0, 1e-6, (7.5, 5.0, 0.75))
    dt_sub = float(np.float32(0.0025))
    m = _model(g, 2)
    try:
        u, v, p = _random_state(g, 4100 + scheme, dt_sub)
        m.set_state(u=u, v=v, p=p)
        before = m.get_state()
        m.script_piso_step(dt_sub, scheme, 0.8, 1)
        _check_against_restatement(f"800x264 scheme {scheme}", g, m, before, m.get_state(), dt_sub,
                                   scheme, 0.8, 1)
    finally:
        m.close()


def test_three_wave_columns_match_restatement():
    g = ref.Grid(520, 40, 13.0, 1.0, 0.01, (3.0, 0.5, 0.2))   # chunks 0..130: wave seams at 248, 496
    dt_sub = float(np.float32(0.002))
    m = _model(g, 4)
    try:
        u, v, p = _random_state(g, 4200, dt_sub)
        m.set_state(u=u, v=v, p=p)
        before = m.get_state()
        m.script_piso_step(dt_sub, 2, 1.0, 0)
        _check_against_restatement("520x40", g, m, before, m.get_state(), dt_sub, 2, 1.0, 0)
    finally:
        m.close()


def test_three_consecutive_substeps_match_restatement():
    g = ref.Grid(264, 20, 30.0, 10.0, 0.01, (7.5, 5.0, 1.75))
    dt_sub = float(np.float32(0.01))
    steps = [(2, 0.5, 1), (1, 0.75, 1), (2, 0.75, 0)]   # scheme, inlet velocity (the ramp), profile
    m, probe = _model(g, 2), _model(g, 2)
    try:
        u, v, p = _random_state(g, 4300, dt_sub, cfl=0.3)
        m.set_state(u=u, v=v, p=p)
        for scheme, inlet, profile in steps:     # enqueued back to back, nothing read between
            m.script_piso_step(dt_sub, scheme, inlet, profile)
        got = m.get_state()
        # the same three, one at a time, each checked against the restatement
        probe.set_state(u=u, v=v, p=p)
        for k, (scheme, inlet, profile) in enumerate(steps):
            before = probe.get_state()
            probe.script_piso_step(dt_sub, scheme, inlet, profile)
            st = probe.get_state()
            _check_against_restatement(f"substep {k}", g, probe, before, st, dt_sub, scheme, inlet,
                                       profile)
        for f in FLOW:
            assert_bitwise(f"three substeps:{f}", got[f], st[f])
        for k in SCALARS:
            assert np.asarray(got[k]).tobytes() == np.asarray(st[k]).tobytes(), k
    finally:
        m.close()
        probe.close()


# ------------------------------------------- bookkeeping around the call
@pytest.mark.parametrize("solver", [2, 4])
def test_substep_between_rust_updates(solver):
    """update, script substep, update == update, set_state(restated substep), update."""
    g = ref.Grid(64, 24, 30.0, 10.0, 0.01, (7.5, 5.0, 1.5))
    dt_sub, scheme, inlet, profile = float(np.float32(0.004)), 2, 0.6, 1
    a, b, probe = (_model(g, solver, corrector_passes=0) for _ in range(3))
    try:
        u, v, p = _random_state(g, 4400, 0.02, cfl=0.2)
        for m in (a, b, probe):
            m.set_state(u=u, v=v, p=p)
        a.update()
        a.script_piso_step(dt_sub, scheme, inlet, profile)
        a.update()
        got = a.get_state()
        # the solve's p' and residual of that substep, from a model of its own
        probe.update()
        before = probe.get_state()
        probe.script_piso_step(dt_sub, scheme, inlet, profile)
        mid = probe.get_state()
        _check_against_restatement("between updates", g, probe, before, mid, dt_sub, scheme, inlet,
                                   profile)
        us, vs, rhs = ref.predict(g, before["u"], before["v"], dt_sub, scheme)
        un, vn, pn = ref.correct(g, us, vs, mid["p_prime"], before["p"], dt_sub, inlet, profile)
        b.update()
        b.set_state(u=un, v=vn, p=pn, u_star=us, v_star=vs, rhs=rhs, p_prime=mid["p_prime"],
                    last_p_residual=mid["last_p_residual"],
                    jacobi_sweeps_total=mid["jacobi_sweeps_total"])
        b.update()
        want = b.get_state()
        for f in FLOW:
            assert_bitwise(f"update/substep/update:{f}", got[f], want[f])
        for k in SCALARS:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    finally:
        for m in (a, b, probe):
            m.close()


# ------------------------------------------------------------------ rejections
def _einval(call, needle=None):
    import cfdamd
    with pytest.raises(cfdamd.CfdError) as e:
        call()
    assert e.value.code == -1, e.value
    if needle:
        assert needle in str(e.value), e.value


def test_rejections():
    import cfdamd
    g = ref.Grid(32, 16, 2.0, 1.0, 0.01)
    ok = _model(g, 2)
    try:
        ok.script_piso_step(0.01, 2, 1.0)
        ok.synchronize()
        for bad_dt in (0.0, -0.01, np.nan, np.inf):
            _einval(lambda: ok.script_piso_step(bad_dt, 2, 1.0), "dt_sub")
        for bad_iv in (np.nan, np.inf, -np.inf):
            _einval(lambda: ok.script_piso_step(0.01, 2, bad_iv), "inlet_velocity")
        for bad_scheme in (-1, 3):
            _einval(lambda: ok.script_piso_step(0.01, bad_scheme, 1.0), "scheme")
        for bad_profile in (-1, 2):
            _einval(lambda: ok.script_piso_step(0.01, 2, 1.0, bad_profile), "profile")
        _einval(lambda: ok.script_phase(2, 0.01, 2, 1.0), "phase")
        _einval(lambda: ok.script_phase(0, 0.0, 2, 1.0), "dt_sub")
    finally:
        ok.close()
    for solver in (0, 1):
        m = _model(g, solver)
        try:
            _einval(lambda: m.script_piso_step(0.01, 2, 1.0), "pressure_solver")
            _einval(lambda: m.script_phase(0, 0.01, 2, 1.0), "pressure_solver")
        finally:
            m.close()
    cav = cfdamd.Model(cfdamd.cavity_grid(32), cfdamd.SimulationParams.cavity(
        100.0, 50, pressure_solver=cfdamd.PressureSolver.Multigrid))
    try:
        _einval(lambda: cav.script_piso_step(0.01, 2, 1.0), "channel")
    finally:
        cav.close()


def test_sharded_model_rejects_the_substep():
    import cfdamd
    from _slabs import run_slabs

    def fn(m, rank):
        try:
            m.script_piso_step(0.01, 2, 1.0)
        except cfdamd.CfdError as e:
            return e.code, str(e)
        return 0, ""

    out = run_slabs(2, cfdamd.Grid(64, 64, 2.0, 2.0),
                    cfdamd.SimulationParams(pressure_solver=cfdamd.PressureSolver.Multigrid), None,
                    None, fn, join=120.0)
    for code, msg in out:
        assert code == -1 and "one domain" in msg, (code, msg)


def test_velocity_scheme_2_is_still_rejected():
    import cfdamd
    params = cfdamd.SimulationParams()
    params.velocity_scheme = 2
    _einval(lambda: cfdamd.Model(cfdamd.Grid(32, 16, 2.0, 1.0), params), "velocity_scheme")
