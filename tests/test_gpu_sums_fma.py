"""GPU: the fma form of the per-launch Jacobi march (LdsMarch SUMS == 2:
fma(h + v, 1/dx^2, -rhs), 9 VALU per update instead of 11) and its
whole-solve guard, whose maxima the corrector finish (max |p'|) and the
predictor march (max |rhs|) publish in Ctl.

Grids: cavity_grid(128) and cavity_grid(256, 128): power-of-two spacing,
reciprocal multiply, kind 5 at T = 8 with column-edge and row-edge waves in a
handful of workgroups.  24 sweeps per step: three T = 8 launches, the last
one with the residual (MODE 1).  Everything is bitwise against the oracle;
Model.sums_launches tells which body ran."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _util import ADV_FIELDS, assert_bitwise, same_f32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(128, 128), (256, 128)]
ITERS = 24
LAUNCHES = 3   # T = 8 launches of a 24-sweep solve


def _pair(nx, ny, **kw):
    import cfdamd
    from oracle import OracleModel
    kw = dict(dict(jacobi_iters=ITERS, corrector_passes=0, tol_enabled=False), **kw)
    params = cfdamd.SimulationParams.cavity(
        100.0, kw["jacobi_iters"], corrector_passes=kw["corrector_passes"],
        tol_enabled=kw["tol_enabled"], pressure_solver=cfdamd.PressureSolver(kw.get("pressure_solver", 0)))
    m = cfdamd.Model(cfdamd.cavity_grid(nx, ny), params, device=0)
    o = OracleModel(nx, ny, float(nx) / float(ny), 1.0, bc_kind=1, viscosity=0.01, **kw)
    return m, o, params


def _compare(tag, m, o, nan_equal=False):
    st = m.get_state()
    for f in ADV_FIELDS:
        assert_bitwise(f"{tag}: {f}", st[f], o.field(f), nan_equal=nan_equal)
    s = o.scalars()
    assert st["simulation_step"] == s.step, tag
    assert st["jacobi_sweeps_total"] == s.jacobi_sweeps_total, tag
    for k, want in (("dt", s.dt), ("simulation_time", s.time), ("last_p_residual", s.p),
                    ("last_u_residual", s.u), ("last_v_residual", s.v)):
        assert same_f32(st[k], want) or (nan_equal and np.isnan(st[k]) and np.isnan(want)), (tag, k)


def _state_words(m):
    st = m.get_state()
    return np.concatenate([np.ascontiguousarray(st[f], np.float32).view(np.uint32).ravel()
                           for f in ADV_FIELDS])


def _load(m, o, fields):
    """The model's current state with `fields` replaced, into both models."""
    st = m.get_state()
    st.update(fields)
    m.set_state(**st)
    for f in ADV_FIELDS:
        o.field(f)[:] = st[f]


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_form_runs_from_step_two_and_matches_oracle(nx, ny):
    m, o, _ = _pair(nx, ny)
    try:
        for step in range(1, 7):
            m.update()
            o.update()
            _compare(f"{nx}x{ny} step {step}", m, o)
            # step 1 has no valid max |p'|: the reference's body
            assert m.sums_launches == LAUNCHES * (step - 1), (step, m.sums_launches)
    finally:
        m.close()


_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [{pkg!r}, {tests!r}]
import cfdamd
from _util import ADV_FIELDS
params = cfdamd.SimulationParams.cavity(100.0, {iters}, corrector_passes=0, tol_enabled=False)
m = cfdamd.Model(cfdamd.cavity_grid({nx}, {ny}), params, device=0)
for _ in range(6):
    m.update()
st = m.get_state()
w = np.concatenate([np.ascontiguousarray(st[f], np.float32).view(np.uint32).ravel() for f in ADV_FIELDS])
np.save({out!r}, w)
print("launches", m.sums_launches)
"""


def test_knob_off_gives_identical_words_and_counter_zero(tmp_path):
    nx, ny = SHAPES[1]
    m, _, _ = _pair(nx, ny)
    try:
        for _ in range(6):
            m.update()
        want = _state_words(m)
        assert m.sums_launches == LAUNCHES * 5
    finally:
        m.close()
    out = str(tmp_path / "off.npy")
    code = _CHILD.format(pkg=os.path.join(ROOT, "cfd-demo_amd"), tests=os.path.join(ROOT, "tests"),
                         iters=ITERS, nx=nx, ny=ny, out=out)
    env = dict(os.environ, CFD_JACOBI_SUMS="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "launches 0" in r.stdout, r.stdout
    assert np.array_equal(np.load(out), want)


def _fallback_case(name, nx, ny):
    n = nx * ny
    if name == "huge":
        # p' = 2^110 everywhere: R max|p'| = 2^124 (R = 2^14) is above the
        # guard's 2^123.  The first step after set_state runs the reference's
        # body anyway (the maxima were dropped) and stays finite; the second
        # finds the finish's max |p'| and must refuse the form.
        return {"p_prime": np.full(n, 2.0 ** 110, np.float32)}
    pp = np.random.default_rng([nx, ny, 8]).uniform(-1e-3, 1e-3, n).astype(np.float32)
    if name == "nan":
        pp[nx * (ny // 2) + nx // 3] = np.nan
    elif name == "inf":
        pp[nx * (ny // 3) + nx // 2] = np.inf
    return {"p_prime": pp}


@pytest.mark.parametrize("name", ["huge", "nan", "inf"])
def test_guard_falls_back(name):
    """huge: the finish's max |p'| alone refuses the form (the rhs term has its
    own tests below).  nan / inf: the first step after set_state runs the
    reference's body whatever the maxima, and after it the model refuses to
    step on (non-finite velocities), so the kernel's own answer to NaN / Inf
    maxima -- `bound < 2^123` is false for a NaN or Inf sum -- is not seen
    through update() and the counter alone; these two cases pin the step the
    model still runs and that the counter stands still.  What the publishers
    answer to a NaN or Inf in p' is read back (Model.sums_bounds) in
    test_gpu_sums_fma_shapes.py::test_finish_maximum_sees_the_planted_cell."""
    import cfdamd
    nx, ny = SHAPES[0]
    m, o, _ = _pair(nx, ny)
    try:
        for _ in range(2):
            m.update()
            o.update()
        base = m.sums_launches
        assert base == LAUNCHES
        _load(m, o, _fallback_case(name, nx, ny))
        refused = 0
        for step in range(3):
            # after a step that left non-finite velocities the model refuses
            # the next one (nothing runs): the comparison ends there
            try:
                m.update()
            except cfdamd.CfdError:
                assert step > 0, "the first step after set_state must run"
                break
            o.update()
            _compare(f"{name} step {step}", m, o, nan_equal=True)
            assert m.sums_launches == base, (name, step, m.sums_launches)
            refused += step > 0   # step 0 never has valid maxima
        if name == "huge":
            assert refused >= 1, "no step reached the guard with its maxima valid"
    finally:
        m.close()


def test_subnormal_p_prime_runs_the_form():
    nx, ny = SHAPES[0]
    m, o, _ = _pair(nx, ny)
    try:
        for _ in range(2):
            m.update()
            o.update()
        rng = np.random.default_rng([nx, ny, 9])
        pp = rng.integers(0, 1 << 23, nx * ny, dtype=np.uint32)          # subnormals and +0
        pp |= rng.integers(0, 2, nx * ny, dtype=np.uint32) << np.uint32(31)   # mixed signs, -0
        pp[::5] &= np.uint32(0x80000000)                                  # signed zeros
        _load(m, o, {"p_prime": pp.view(np.float32)})
        base = m.sums_launches
        m.update()   # set_state dropped the maxima: the reference's body
        o.update()
        _compare("subnormal step 0", m, o)
        assert m.sums_launches == base
        m.update()
        o.update()
        _compare("subnormal step 1", m, o)
        assert m.sums_launches == base + LAUNCHES
    finally:
        m.close()


@pytest.mark.parametrize("how", ["set_state", "pressure_solve", "piso_step", "params"])
def test_invalidation(how):
    import cfdamd
    nx, ny = SHAPES[0]
    m, o, params = _pair(nx, ny)
    try:
        for _ in range(3):
            m.update()
            o.update()
        assert m.sums_launches == 2 * LAUNCHES
        if how == "set_state":
            pp = np.random.default_rng([nx, ny, 10]).uniform(-1, 1, nx * ny).astype(np.float32)
            _load(m, o, {"p_prime": pp})
        elif how == "pressure_solve":
            m.pressure_solve()
            o.pressure_solve()
        elif how == "piso_step":
            m.piso_step(0.001)
            o.piso_step(0.001)
        else:
            tol = cfdamd.SimulationParams.cavity(100.0, ITERS, corrector_passes=0, tol_enabled=True)
            m.set_parameters(tol)
            m.set_parameters(params)
        base = m.sums_launches
        assert base == 2 * LAUNCHES, (how, base)   # none of these ran the form
        m.update()
        o.update()
        _compare(f"{how}: first step after", m, o)
        assert m.sums_launches == base, (how, m.sums_launches)
        m.update()
        o.update()
        _compare(f"{how}: second step after", m, o)
        assert m.sums_launches == base + LAUNCHES
    finally:
        m.close()


@pytest.mark.parametrize("solver", [1, 2])
def test_other_solvers_never_take_the_form(solver):
    nx, ny = SHAPES[0]
    m, _, _ = _pair(nx, ny, pressure_solver=solver)
    try:
        m.update()
        m.update()
        assert m.sums_launches == 0
    finally:
        m.close()


# ------------------------------------------------- the guard's rhs term (Rm)

def _scale_velocities(m, o, e):
    """u, v of the developed state times 2^e, into both models.  The CFL time
    step shrinks with it, so from the second step on the divergence / dt of
    the predicted velocities -- the rhs the predictor march forms and measures
    -- grows like 2^(2 e) while the fields stay smooth and finite."""
    st = m.get_state()
    s = np.float32(2.0 ** e)
    _load(m, o, {"u": st["u"] * s, "v": st["v"] * s})


def test_guard_refuses_on_rhs_alone():
    """Rm alone decides: max |p'| R stays far below 2^123 (p' is zero, then
    about 2^102, R = 2^14) while 0.1875 * 4096 * max |rhs| is above it (|rhs|
    about 2^118).  The premises are read back from the state and asserted, so
    the case cannot pass for another reason; a march that published no, or too
    small, a maximum would let the form run and the counter advance."""
    nx, ny = SHAPES[0]
    R, lim = 2.0 ** 14, 2.0 ** 123
    m, o, _ = _pair(nx, ny)
    try:
        for _ in range(2):
            m.update()
            o.update()
        base = m.sums_launches
        _scale_velocities(m, o, 58)
        m.update()   # set_state dropped the maxima: the reference's body
        o.update()
        _compare("rhs-alone step 0", m, o)
        assert m.sums_launches == base
        for step in (1, 2):
            pp_before = np.float64(np.max(np.abs(m.get_state()["p_prime"])))
            m.update()
            o.update()
            _compare(f"rhs-alone step {step}", m, o)
            st = m.get_state()
            assert all(np.all(np.isfinite(st[f])) for f in ADV_FIELDS), step
            rm = np.float64(np.max(np.abs(st["rhs"])))
            print(f"step {step}: max|p'| before 2^{np.log2(max(pp_before, 1e-300)):.1f} max|rhs| 2^{np.log2(rm):.1f}")
            assert pp_before * R < lim / 16, "max |p'| must not decide"
            assert 0.1875 * 4096 * rm >= 2 * lim, "max |rhs| must decide"
            assert m.sums_launches == base, (step, m.sums_launches)
    finally:
        m.close()


def test_moderate_rhs_keeps_the_form():
    """The same construction two hundred binades lower (|rhs| about 2^62): both
    terms pass and the form runs on large, smooth, developed fields."""
    nx, ny = SHAPES[0]
    m, o, _ = _pair(nx, ny)
    try:
        for _ in range(2):
            m.update()
            o.update()
        base = m.sums_launches
        _scale_velocities(m, o, 30)
        for step in range(3):
            m.update()
            o.update()
            _compare(f"moderate step {step}", m, o)
            assert m.sums_launches == base + LAUNCHES * step, (step, m.sums_launches)
        rm = float(np.max(np.abs(m.get_state()["rhs"])))
        assert 2.0 ** 50 < rm < 2.0 ** 100, rm
    finally:
        m.close()


# --------------------------------------------- a developed golden state

def test_developed_golden_state():
    """tests/golden/run_cavity_128x128_fixed50: the 128 x 128 cavity after 20
    fixed-count steps (50 sweeps, no corrector passes).  Loaded into both
    models; the first step after set_state runs the reference's body, the
    next three the fma body, on a developed field, bitwise vs the oracle."""
    import json
    import cfdamd
    from oracle import OracleModel
    gold = os.path.join(ROOT, "tests", "golden")
    name = "run_cavity_128x128_fixed50"
    meta = json.load(open(os.path.join(gold, "manifest.json")))["fixtures"][name]
    g, p = meta["grid"], meta["params"]
    assert (g["nx"], g["ny"], g["cylinder"]) == (128, 128, None) and p["corrector_passes"] == 0
    assert p["bc_kind"] == 1 and not p.get("tol_enabled", 0) and p["jacobi_iters"] == 50
    fx = np.load(os.path.join(gold, name + ".npz"))
    params = cfdamd.SimulationParams.cavity(1.0 / p["viscosity"], 50, corrector_passes=0, tol_enabled=False)
    assert np.float32(params.viscosity) == np.float32(p["viscosity"])
    m = cfdamd.Model(cfdamd.cavity_grid(128), params, device=0)
    o = OracleModel(128, 128, 1.0, 1.0, bc_kind=1, viscosity=p["viscosity"], jacobi_iters=50,
                    corrector_passes=0, tol_enabled=False)
    try:
        t, dt, rp, ru, rv = fx["scalars_f32"]
        step, sweeps = (int(x) for x in fx["scalars_i64"])
        m.set_state(**{f: fx[f] for f in ADV_FIELDS}, dt=dt, simulation_time=t, simulation_step=step,
                    jacobi_sweeps_total=sweeps, last_p_residual=rp, last_u_residual=ru,
                    last_v_residual=rv)
        for f in ADV_FIELDS:
            o.field(f)[:] = fx[f]
        s = o.scalars()
        s.step, s.time, s.dt, s.jacobi_sweeps_total, s.p, s.u, s.v = step, t, dt, sweeps, rp, ru, rv
        o.set_scalars(s)
        per_step = None
        for k in range(4):
            m.update()
            o.update()
            _compare(f"golden step {k}", m, o)
            n = m.sums_launches
            if k == 0:
                assert n == 0, n        # no valid max |p'| after set_state
            elif k == 1:
                per_step = n            # 50 sweeps: six T = 8 launches and the short last one
                assert per_step >= 6, per_step
            else:
                assert n == k * per_step, (k, n, per_step)
    finally:
        m.close()


def test_run_phase_drops_the_maxima():
    """cfd_run_phase can change rhs, u*, v* outside a step: the next step's
    solve must not trust the finish's max |p'| (no solve finalize lies between,
    so only the host-side invalidation makes the counter stand still; after
    cfd_pressure_solve and cfd_piso_step, test_invalidation above, the solve's
    own finalize has dropped the maxima as well)."""
    nx, ny = SHAPES[0]
    m, o, _ = _pair(nx, ny)
    try:
        for _ in range(3):
            m.update()
            o.update()
        base = m.sums_launches
        assert base == 2 * LAUNCHES
        m.run_phase(4, 0.0)   # CFD_PHASE_BOUNDARY
        o.boundary()
        m.update()
        o.update()
        _compare("run_phase: first step after", m, o)
        assert m.sums_launches == base
        m.update()
        o.update()
        _compare("run_phase: second step after", m, o)
        assert m.sums_launches == base + LAUNCHES
    finally:
        m.close()
