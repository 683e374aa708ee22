"""GPU: the fixed-count step that keeps u*, v* out of memory (CFD_UV_FUSED).

k_predict_march<.., true> stores rhs only; after the solve k_finish_march
forms u*, v* again from the old u, v, runs the corrector finish's row work and
stores the new u, v into the other pair of arrays, which the host then makes
the current pair; u*, v* are materialised from the old pair when something
reads them.  Every case runs with the knob on and off, and every field word
and scalar of both runs is compared with oracle/cfd_oracle.c.

Shapes (a model takes nx % 8 == 0, nx >= 16): 16 x 8 is one wave column and
one 8-row segment; ny = 15, 16, 17, 33 put the segment seams (8 rows, the last
segment overlapping its neighbour) everywhere they can fall; nx = 248 / 256
are 62 chunks -- one wave column whose outflow chunk opens the next -- and
62 + 2; nx = 1024 / 1032 straddle 256 threads x 4 columns, five wave columns.
"""
import numpy as np
import pytest

from _util import (ADV_FIELDS, adversarial_state, assert_bitwise, load_state, nonfinite_share,
                   same_f32)

pytestmark = pytest.mark.gpu

P2 = 1.0 / 128.0
CHANNEL = dict(nx=64, ny=24, lx=8.0, ly=3.0, cylinder=(2.0, 1.5, 0.5))


def _pair(monkeypatch, knob, g, **kw):
    import cfdamd as c
    from oracle import OracleModel
    monkeypatch.setenv("CFD_UV_FUSED", knob)
    cyl = g.get("cylinder")
    kw.setdefault("tol_enabled", 0)
    kw.setdefault("corrector_passes", 0)
    kw.setdefault("jacobi_iters", 4)
    params = c.SimulationParams(
        viscosity=kw.get("viscosity", 1e-6), velocity_scheme=c.VelocityScheme(kw.get("scheme", 0)),
        inlet_profile=c.InletProfile(kw.get("inlet_profile", 0)),
        jacobi_iters=kw.get("jacobi_iters", 4), corrector_passes=kw["corrector_passes"],
        tol_enabled=bool(kw["tol_enabled"]), p_tol=kw.get("p_tol", 1e-4),
        bc_kind=c.BoundaryKind(kw.get("bc_kind", 0)))
    m = c.Model(c.Grid(g["nx"], g["ny"], g["lx"], g["ly"], c.Cylinder(*cyl) if cyl else None), params)
    o = OracleModel(g["nx"], g["ny"], g["lx"], g["ly"], cylinder=cyl, **kw)
    m.oracle_kw = kw
    return m, o, params


def _grid(nx, ny):
    return dict(nx=nx, ny=ny, lx=nx * P2, ly=ny * P2)


def _compare(tag, m, o, nan_equal=False):
    st = m.get_state()
    for f in ADV_FIELDS:
        assert_bitwise(f"{tag}: {f}", st[f], o.field(f), nan_equal=nan_equal)
    s = o.scalars()
    assert st["simulation_step"] == s.step, tag
    assert st["jacobi_sweeps_total"] == s.jacobi_sweeps_total, tag
    for k, want in (("dt", s.dt), ("simulation_time", s.time), ("last_p_residual", s.p),
                    ("last_u_residual", s.u), ("last_v_residual", s.v)):
        assert same_f32(st[k], want) or (nan_equal and np.isnan(st[k]) and np.isnan(want)), \
            (tag, k, st[k], want)
    return st


SHAPES = [(16, 8), (16, 15), (16, 16), (16, 17), (16, 33), (248, 9), (256, 9), (1032, 20), (1024, 9)]


@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_steps_from_rest_and_random(monkeypatch, nx, ny, scheme, knob):
    """3 steps of 4 sweeps from rest (the inlet ramp from step 0), then 2 more
    from a random state of both signs, compared after every step."""
    m, o, _ = _pair(monkeypatch, knob, _grid(nx, ny), scheme=scheme)
    for k in range(3):
        m.update()
        o.update()
        _compare(f"{nx}x{ny} s{scheme} knob{knob} step {k}", m, o)
    st = adversarial_state(nx, ny, 11, "signs")
    load_state(st, model=m, oracle=o)
    for k in range(2):
        m.update()
        o.update()
        _compare(f"{nx}x{ny} s{scheme} knob{knob} random step {k}", m, o)


@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("profile", [0, 1])
@pytest.mark.parametrize("scheme", [0, 1])
def test_channel_with_cylinder(monkeypatch, scheme, profile, knob):
    """The channel with the cylinder (both masks live), inlet ramp active from
    step 0, several steps in one call."""
    m, o, _ = _pair(monkeypatch, knob, CHANNEL, scheme=scheme, inlet_profile=profile, jacobi_iters=9)
    for n in (1, 3):
        m.update_n(n)
        for _ in range(n):
            o.update()
        _compare(f"channel s{scheme} p{profile} knob{knob} after {n}", m, o)


@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("scheme", [0, 1])
def test_star_fields_stay_observable(monkeypatch, scheme, knob):
    """update_n(3), two reads (equal, u* / v* the oracle's), two more steps;
    set_state then one step; a switch to two corrector passes and back."""
    g = _grid(64, 17)
    m, o, params = _pair(monkeypatch, knob, g, scheme=scheme)
    m.update_n(3)
    for _ in range(3):
        o.update()
    a = _compare("first read", m, o)
    b = _compare("second read", m, o)
    for f in ADV_FIELDS:
        assert_bitwise(f"reads: {f}", a[f], b[f])
    m.update_n(2)
    for _ in range(2):
        o.update()
    _compare("after two more", m, o)
    # a state that names only u and v: u*, v* keep the last step's values
    st = adversarial_state(g["nx"], g["ny"], 5, "signs")
    m.set_state(u=st["u"], v=st["v"])
    o.field("u")[:] = st["u"]
    o.field("v")[:] = st["v"]
    _compare("after set_state(u, v)", m, o)
    m.update()
    o.update()
    _compare("set_state + 1", m, o)
    # two corrector passes mid-run, and back
    import dataclasses
    m.set_parameters(dataclasses.replace(params, corrector_passes=2))
    o.set_params(**dict(m.oracle_kw, corrector_passes=2))
    m.update()
    o.update()
    _compare("two passes", m, o)
    m.set_parameters(params)
    o.set_params(**m.oracle_kw)
    m.update_n(2)
    for _ in range(2):
        o.update()
    _compare("back to none", m, o)


@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("flavour", ["range", "nonfinite"])
@pytest.mark.parametrize("scheme", [0, 1])
def test_adversarial_state(monkeypatch, scheme, flavour, knob):
    """NaN, Inf, -0 and subnormals in u, v, p' before a step (64 x 33: five
    segments, 2112 cells, one planted non-finite word; a model steps once
    from a state that turns non-finite, then reports it)."""
    nx, ny = 64, 33
    m, o, _ = _pair(monkeypatch, knob, _grid(nx, ny), scheme=scheme, jacobi_iters=3)
    st = adversarial_state(nx, ny, 3, flavour)
    load_state(st, model=m, oracle=o)
    nonfinite = flavour == "nonfinite"
    for k in range(1 if nonfinite else 2):
        m.update()
        o.update()
        _compare(f"{flavour} s{scheme} knob{knob} step {k}", m, o, nan_equal=nonfinite)
    if nonfinite:
        import cfdamd as c
        assert 0.0 < nonfinite_share([o.field(f) for f in ADV_FIELDS]) <= 0.20
        with pytest.raises(c.CfdError) as ei:
            m.get_residuals()
        assert ei.value.code == c.CFD_ENONFINITE, ei.value


@pytest.mark.parametrize("knob", ["1", "0"])
def test_graph_replay(monkeypatch, knob):
    """CFD_GRAPH=1: steps replayed from the captured graph equal plain steps,
    from either arrangement of the u / v pairs (3 plain steps leave them
    swapped when the graph is captured and replayed next)."""
    g = _grid(64, 17)
    monkeypatch.setenv("CFD_GRAPH", "1")
    mg, o, _ = _pair(monkeypatch, knob, g)
    monkeypatch.setenv("CFD_GRAPH", "0")
    mp, _, _ = _pair(monkeypatch, knob, g)
    done = 0
    for n in (5, 3, 6, 1, 10):
        mg.update_n(n)
        mp.update_n(n)
        for _ in range(n):
            o.update()
        done += n
        a = _compare(f"graph after {done}", mg, o)
        b = mp.get_state()
        for f in ADV_FIELDS:
            assert_bitwise(f"graph vs plain after {done}: {f}", a[f], b[f])
