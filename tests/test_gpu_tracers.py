"""GPU: the device-side tracer particles (cfd_tracers_*, cfd_tracers.hip)
against the script's own lists under node (tests/golden/js_tracers_*.npz) and
the restatement (tests/_tracers_ref.py).

Every comparison is bitwise on the u64 views of x, y and initialY, plus exact
equality of counts and order; there are no tolerances.  No test skips when a
symbol is missing."""
import time

import numpy as np
import pytest

import _tracers_ref as ref
from _util import assert_bitwise
from _tracers_golden import FIXTURES, load_fixture

pytestmark = pytest.mark.gpu

B = 256   # kTrcBlock (cfd_internal.h): the workgroup, and the tile of the compaction
FLOW = ("u", "v", "p", "u_star", "v_star", "p_prime", "rhs")
SCALARS = ("dt", "simulation_time", "simulation_step", "last_p_residual", "last_u_residual",
           "last_v_residual", "jacobi_sweeps_total")


def assert_list(tag, got, want):
    assert got[0].size == want[0].size, (tag, "count", got[0].size, want[0].size)
    for name, a, b in zip(("initial_y", "x", "y"), (got[2], got[0], got[1]), (want[2], want[0], want[1])):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (tag, name)


def assert_flow_equal(tag, a, b):
    for f in FLOW:
        assert_bitwise(f"{tag}:{f}", a[f], b[f])
    for k in SCALARS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (tag, k)


# ---------------------------------------------------------------- node fixtures
@pytest.mark.parametrize("name", FIXTURES)
def test_lists_match_reference_javascript(name):
    import cfdamd
    meta, dom, u, v, start, lists = load_fixture(name)
    m = cfdamd.Model(cfdamd.Grid(meta["nx"], meta["ny"], meta["lx"], meta["ly"]),
                     cfdamd.SimulationParams())
    try:
        m.set_state(u=u, v=v)
        m.tracers_enable(meta["injected"] + 16)
        assert_list(f"{name} initTracers", m.tracers(), ref.init(dom))
        m.set_tracers(*start)
        for s, want in enumerate(lists, 1):
            m.tracers_advance(meta["dt"])
            if (meta["step0"] + s) % meta["interval"] == 0:
                m.tracers_inject()
            assert_list(f"{name} step {s}", m.tracers(), want)
            assert m.tracer_count() == want[0].size
    finally:
        m.close()


# ------------------------------------------------------------ compaction seams
PATTERNS = ("all", "none", "alternating", "first", "last", "last_lane_of_each_wave")
SEAM_DT = 0.05


def _pattern(kind, n):
    k = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": k % 2 == 0,
            "first": k == 0, "last": k == n - 1, "last_lane_of_each_wave": k % 64 == 63}[kind]


def _seam_case(dom, n, kind):
    """n tracers in a uniform flow u = 1 that moves each by about dt: those
    meant to stay end just inside the wall x = Lx, the others just outside."""
    keep = _pattern(kind, n)
    k = np.arange(n, dtype=np.float64)
    x = np.where(keep, dom.lx - 1.5 * SEAM_DT - 1e-3 * (k % 7), dom.lx - 0.5 * SEAM_DT + 1e-3 * (k % 5))
    y = (0.37 + (k * 0.6180339887) % 1.0 * (dom.ny - 0.74)) * dom.dy
    return (x, y, k.copy()), keep


@pytest.fixture(scope="module")
def seam_fields():
    dom = ref.Domain(16, 5, 30.0, 10.0)
    u = np.ones((dom.nx + 1) * dom.ny, np.float32)
    v = np.zeros(dom.nx * (dom.ny + 1), np.float32)
    return dom, u, v


def _seam_model(dom, u, v, cap):
    import cfdamd
    m = cfdamd.Model(cfdamd.Grid(dom.nx, dom.ny, 30.0, 10.0), cfdamd.SimulationParams())
    m.set_state(u=u, v=v)
    m.tracers_enable(cap)
    return m


def _run_seams(m, dom, u, v, lengths, kind):
    for n in lengths:
        start, keep = _seam_case(dom, n, kind)
        want = ref.advance(dom, u, v, SEAM_DT, start)
        # the restatement keeps exactly the tracers the pattern names
        assert want[2].tolist() == np.flatnonzero(keep).astype(np.float64).tolist(), (kind, n)
        m.set_tracers(*start)
        m.tracers_advance(SEAM_DT)
        assert_list(f"{kind} n={n}", m.tracers(), want)
        # and once more from the compacted list (the other buffer)
        m.tracers_advance(-SEAM_DT)
        assert_list(f"{kind} n={n} back", m.tracers(), ref.advance(dom, u, v, -SEAM_DT, want))


@pytest.mark.parametrize("kind", PATTERNS)
def test_compaction_seams(seam_fields, kind):
    dom, u, v = seam_fields
    m = _seam_model(dom, u, v, 2 * B + 1)
    try:
        _run_seams(m, dom, u, v, (0, 1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1), kind)
    finally:
        m.close()


@pytest.mark.parametrize("kind", PATTERNS)
def test_compaction_grid_stride_wraps(seam_fields, kind, monkeypatch):
    """Five tiles on a launch capped at two workgroups: each strides over
    several tiles, and the tile order still decides the output order."""
    monkeypatch.setenv("CFD_TRACER_WGS", "2")
    dom, u, v = seam_fields
    m = _seam_model(dom, u, v, 4 * B + 5)
    try:
        _run_seams(m, dom, u, v, (4 * B + 5, 2 * B + 1), kind)
    finally:
        m.close()


# ------------------------------------------------------------- in-step cadence
def _channel():
    import cfdamd
    return cfdamd.Grid(64, 48, 3.0, 2.0, cfdamd.Cylinder(1.0, 1.0, 0.3)), cfdamd.SimulationParams()


@pytest.mark.parametrize("first_step_injects", [False, True])
def test_in_step_cadence(first_step_injects):
    """update_n(7) == 7 x update() == the restatement fed each step's snapshot
    and dt, at interval 3; once from step 0 and once from simulation_step 2, so
    that the first step injects."""
    import cfdamd
    grid, params = _channel()
    dom = ref.Domain(grid.nx, grid.ny, grid.lx, grid.ly)
    interval, cap = 3, 48 * 6
    a, b = cfdamd.Model(grid, params), cfdamd.Model(grid, params)
    try:
        for m in (a, b):
            if first_step_injects:
                m.update_n(40)   # a developed inflow, then the step counter set back
                m.set_state(simulation_step=2)
            m.tracers_enable(cap, interval)
        tr = ref.init(dom)
        assert_list("initTracers", b.tracers(), tr)
        counts = []
        for k in range(7):
            b.update()
            snap, res = b.get_snapshot(), b.get_residuals()
            tr = ref.step(dom, snap.u, snap.v, snap.dt, res.simulation_step, interval, tr)
            assert_list(f"step {res.simulation_step}", b.tracers(), tr)
            counts.append(tr[0].size)
        first = 3 if first_step_injects else 1
        assert res.simulation_step == first + 6
        injections = sum(1 for s in range(first, first + 7) if s % interval == 0)
        assert injections == (3 if first_step_injects else 2)
        assert (counts[0] > 48) == first_step_injects
        a.update_n(7)
        assert_list("update_n(7) against 7 x update()", a.tracers(), tr)
        assert_flow_equal("update_n(7) against 7 x update()", a.get_state(), b.get_state())
    finally:
        a.close()
        b.close()


def test_flow_is_the_same_disabled_and_enabled():
    import cfdamd
    grid, params = _channel()
    never, off, on = (cfdamd.Model(grid, params) for _ in range(3))
    try:
        off.tracers_enable(480, 2)
        off.tracers_disable()
        on.tracers_enable(480, 2)
        for m in (never, off, on):
            m.update_n(5)
            m.update()
        ref_state = never.get_state()
        assert_flow_equal("enabled then disabled", off.get_state(), ref_state)
        assert_flow_equal("enabled", on.get_state(), ref_state)
        assert on.tracer_count() > 48   # steps 2, 4 and 6 injected
        with pytest.raises(cfdamd.CfdError) as e:
            off.tracer_count()
        assert e.value.code == -4
    finally:
        for m in (never, off, on):
            m.close()


# -------------------------------------------------------------------- overflow
def test_overflow_is_sticky_until_set():
    import cfdamd
    grid, params = _channel()
    m, plain = cfdamd.Model(grid, params), cfdamd.Model(grid, params)
    try:
        m.tracers_enable(grid.ny + 1, 1)   # the first step's injection cannot fit
        before = m.tracers()
        m.update()
        plain.update()
        for call in (m.tracer_count, m.tracers, m.tracer_density):
            with pytest.raises(cfdamd.CfdError) as e:
                call()
            assert e.value.code == -4 and "overflow" in str(e.value)
        m.update()   # stepping goes on; the word stays set
        plain.update()
        with pytest.raises(cfdamd.CfdError):
            m.tracer_count()
        m.set_tracers(*before)
        assert_list("after cfd_tracers_set", m.tracers(), before)
        assert_flow_equal("overflowed", m.get_state(), plain.get_state())
        for bad in (np.nan, np.inf):
            x = before[0].copy()
            x[3] = bad
            with pytest.raises(cfdamd.CfdError) as e:
                m.set_tracers(x, before[1], before[2])
            assert e.value.code == -1
        with pytest.raises(cfdamd.CfdError) as e:
            m.set_tracers(*(np.zeros(grid.ny + 2) for _ in range(3)))
        assert e.value.code == -1
        with pytest.raises(cfdamd.CfdError) as e:
            m.tracers_enable(grid.ny - 1)
        assert e.value.code == -1
    finally:
        m.close()
        plain.close()


# -------------------------------------------------------------------- recovery
def test_tracers_survive_a_recovered_timeout(monkeypatch):
    """The forced-deadline pattern of test_gpu_spec.py, with tracers enabled:
    the replay after the recovery must not move the tracers twice."""
    import cfdamd
    from cfdamd._lib import CFD_ETIMEOUT, CfdError
    monkeypatch.setenv("CFD_RESIDENT", "1")
    grid = cfdamd.cavity_grid(256, 128)
    params = cfdamd.SimulationParams.cavity(400.0, 50, p_tol=2e-4)
    rng = np.random.default_rng(11)
    start = (rng.uniform(0.05, 0.95, 700) * grid.lx, rng.uniform(0.05, 0.95, 700) * grid.ly,
             np.arange(700.0))

    def fresh():
        m = cfdamd.Model(grid, params, device=0)
        m.tracers_enable(4096, 2)
        m.set_tracers(*start)
        return m

    m = fresh()
    try:
        m.update_n(3)
        m.synchronize()
        monkeypatch.setenv("CFD_PERSIST_DEADLINE_US", "0")
        monkeypatch.setenv("CFD_PERSIST_LATE", "3")   # workgroups 1, 4, ... arrive 2 ms late
        steps = 0
        with pytest.raises(CfdError) as ei:
            for _ in range(5):   # the first barrier wait faults
                m.update()
                steps += 1
                m.synchronize()
        assert ei.value.code == CFD_ETIMEOUT, ei.value
        assert "recovered" in str(ei.value), ei.value
        assert m.recoveries == 1
        monkeypatch.delenv("CFD_PERSIST_DEADLINE_US")
        monkeypatch.delenv("CFD_PERSIST_LATE")
        m.update_n(2)
        got, got_state = m.tracers(), m.get_state()
    finally:
        m.close()
    o = fresh()
    try:
        o.update_n(3 + steps + 2)
        want = o.tracers()
        assert o.recoveries == 0
        assert want[0].size > 700   # injections happened on the way
        assert_list("recovered", got, want)
        assert_flow_equal("recovered", got_state, o.get_state())
    finally:
        o.close()


# --------------------------------------------------------------------- density
def test_density_equals_histogram():
    import cfdamd
    dom = ref.Domain(16, 5, 30.0, 10.0)
    m = cfdamd.Model(cfdamd.Grid(16, 5, 30.0, 10.0), cfdamd.SimulationParams())
    try:
        rng = np.random.default_rng(5)
        n = 3 * B + 17
        x = rng.uniform(0, dom.lx, n)
        y = rng.uniform(0, dom.ly, n)
        x[:4] = [dom.lx, dom.lx, 0.0, 3 * dom.dx]   # on the walls and on a cell edge
        y[:4] = [dom.ly, 1.0, dom.ly, 2 * dom.dy]
        x[4:6], y[4:6] = [-2.0, dom.lx + 5.0], [-1.0, dom.ly + 3.0]   # outside: clipped
        tr = (x, y, np.arange(float(n)))
        m.tracers_enable(n)
        m.set_tracers(*tr)
        d = m.tracer_density()
        assert d.dtype == np.uint32 and d.shape == (5, 16) and int(d.sum()) == n
        assert np.array_equal(d, ref.density(dom, tr))
        assert d[4, 15] >= 2 and d[0, 0] >= 1
    finally:
        m.close()


# --------------------------------------------------------------------- runtime
def _wait(pred, limit=30.0):
    t0 = time.time()
    while not pred():
        if time.time() - t0 > limit:
            raise AssertionError("timed out")
        time.sleep(0.005)


def _paused_snapshot(h):
    h.pause()
    h.request_snapshot()
    snap = []
    _wait(lambda: snap.append(h.get_last_available_snapshot()) or snap[-1] is not None)
    assert snap[-1].paused
    return snap[-1]


def test_runtime_snapshots_carry_the_tracers():
    import cfdamd
    grid, params = _channel()
    dom = ref.Domain(grid.nx, grid.ny, grid.lx, grid.ly)
    m = cfdamd.Model(grid, params)
    h = m.run()
    try:
        _wait(lambda: h.steps >= 2)
        _paused_snapshot(h)
        assert h.get_last_available_tracers() is None   # not enabled yet
        s0 = h.steps                                    # paused: enabled at exactly this step
        h.set_tracers(480, 3)
        h.resume()
        _wait(lambda: h.steps >= s0 + 7)
        _paused_snapshot(h)
        s1 = h.steps
        tr = h.get_last_available_tracers()
        assert tr is not None and h.get_last_available_tracers() is None   # taken once
        x, y, iy = tr
        inlet = (np.arange(dom.ny) + 0.5) * dom.dy
        assert np.all(np.isin(iy.view(np.uint64), inlet.view(np.uint64)))
        # the list is initTracers' batch and one batch per injection up to the
        # snapshot's step, each in rising initialY (the cull keeps the order):
        # a few tracers may have left, a whole batch cannot within ten steps,
        # so initialY falls exactly once per injection
        injections = sum(1 for s in range(s0 + 1, s1 + 1) if s % 3 == 0)
        assert injections >= 2
        assert dom.ny * injections < x.size <= dom.ny * (1 + injections)
        assert int(np.count_nonzero(np.diff(iy) <= 0)) == injections
        if s1 % 3 == 0:   # the snapshot's own step injected: its batch is untouched
            assert np.array_equal(iy[-dom.ny:].view(np.uint64), inlet.view(np.uint64))
            assert not x[-dom.ny:].any()
        h.set_tracers(0)
        h.resume()
        _wait(lambda: h.steps >= s1 + 1)
        _paused_snapshot(h)
        assert h.get_last_available_tracers() is None
    finally:
        h.stop()
        m.close()


# --------------------------------------------------------------------- sharded
def test_sharded_model_rejects_tracers():
    import cfdamd
    from _slabs import run_slabs

    def fn(m, rank):
        try:
            m.tracers_enable(1024)
        except cfdamd.CfdError as e:
            return e.code, str(e)
        return 0, ""

    out = run_slabs(2, cfdamd.Grid(64, 64, 2.0, 2.0), cfdamd.SimulationParams(), None, None, fn,
                    join=120.0)
    for code, msg in out:
        assert code == -1 and "one domain" in msg, (code, msg)
