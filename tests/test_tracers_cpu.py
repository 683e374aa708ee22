"""CPU: the tracer restatement (tests/_tracers_ref.py) against the script's own
lists under node (tests/golden/js_tracers_*.npz), its edge cases, and the new
symbols of the C ABI.  Every comparison is on the u64 views: no tolerances."""
import numpy as np
import pytest

import _tracers_ref as ref
from _tracers_golden import CLAIMS, FIXTURES, MANIFEST, load_fixture


def test_fixture_set():
    assert FIXTURES == ["js_tracers_16x5", "js_tracers_24x7", "js_tracers_64x48"]
    have = set()
    for fx in MANIFEST["fixtures"].values():
        have |= set(fx["claims"])
        assert 0 < fx["final_count"] < fx["injected"]
    assert have == set(CLAIMS)


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_node(name):
    meta, dom, u, v, start, lists = load_fixture(name)
    assert (dom.dx, dom.dy) == (meta["dx"], meta["dy"])
    # the start list: initTracers, then the outside tracers
    init = ref.init(dom)
    assert ref.bits_equal(tuple(a[:dom.ny] for a in start), init)
    tr = start
    clamps, exits, with_survivors = [0] * 4, [0] * 4, False
    assert len(lists) == meta["steps"]
    for s, want in enumerate(lists, 1):
        tr = ref.advance(dom, u, v, meta["dt"], tr, clamps=clamps, exits=exits)
        if (meta["step0"] + s) % meta["interval"] == 0:
            with_survivors |= tr[0].size > 0
            tr = ref.inject(dom, tr)
        assert ref.bits_equal(tr, want), (name, s)
    facts = dict(zip(CLAIMS, [e > 0 for e in exits] + [c > 0 for c in clamps] + [with_survivors]))
    for c in meta["claims"]:
        assert facts[c], (name, c)


def _flat(dom, uval=0.0, vval=0.0):
    return (np.full((dom.nx + 1) * dom.ny, uval, np.float32),
            np.full(dom.nx * (dom.ny + 1), vval, np.float32))


def test_minus_zero_and_exact_wall_are_kept():
    dom = ref.Domain(16, 5, 30.0, 10.0)
    u, v = _flat(dom)
    x = np.array([-0.0, dom.lx, 1.0, 2.0])
    y = np.array([1.0, 2.0, -0.0, dom.ly])
    out = ref.advance(dom, u, v, 0.05, (x, y, np.arange(4.0)))
    assert out[2].tolist() == [0.0, 1.0, 2.0, 3.0]
    # x + 0 * dt: -0 + 0 = +0 in round-to-nearest, as in the script
    assert out[0].view(np.uint64)[0] == 0 and out[0][1] == dom.lx
    # one ulp past a wall is dropped
    x = np.array([np.nextafter(dom.lx, np.inf), -5e-324, 1.0])
    out = ref.advance(dom, u, v, 0.05, (x, np.ones(3), np.arange(3.0)))
    assert out[2].tolist() == [2.0]


def test_nan_velocity_drops_the_tracer_and_keeps_the_order():
    dom = ref.Domain(16, 5, 30.0, 10.0)
    u, v = _flat(dom, 1.0, 0.0)
    u.reshape(dom.ny, dom.nx + 1)[2, 8] = np.nan   # read by cells (7..8, 1..2) and their neighbours
    x = np.array([0.5, 8.2, 15.1, 7.6]) * dom.dx
    y = np.array([0.5, 2.4, 4.2, 1.7]) * dom.dy
    out = ref.advance(dom, u, v, 0.05, (x, y, np.arange(4.0)))
    assert out[2].tolist() == [0.0, 2.0]
    assert np.all(np.isfinite(out[0]))


def test_far_outside_positions_take_the_clamps():
    dom = ref.Domain(16, 5, 30.0, 10.0)
    rng = np.random.default_rng(3)
    u = rng.uniform(-1, 1, (dom.nx + 1) * dom.ny).astype(np.float32)
    v = rng.uniform(-1, 1, dom.nx * (dom.ny + 1)).astype(np.float32)
    x = np.array([-1e300, 1e300, 3.0, 4.0, 1e308])
    y = np.array([2.0, 3.0, -1e300, 1e300, -1e308])
    clamps = [0] * 4
    i, j = ref.cell_index(dom, x, y, clamps)
    assert clamps == [1, 2, 2, 1]
    assert i.tolist() == [0, dom.nx - 2, 1, 2, dom.nx - 2]   # dx = 1.875
    assert j.tolist() == [1, 1, 0, dom.ny - 2, 0]   # dy = 2
    # the extrapolated velocity is huge but every index stayed in bounds; all are culled
    out = ref.advance(dom, u, v, 0.05, (x, y, np.arange(5.0)))
    assert out[0].size == 0


def test_density_counts_wall_tracers_in_the_last_cell():
    dom = ref.Domain(16, 5, 30.0, 10.0)
    x = np.array([dom.lx, 0.0, 0.0, dom.lx])
    y = np.array([dom.ly, 0.0, 0.0, 1.0])
    d = ref.density(dom, (x, y, x))
    assert d.shape == (5, 16) and d.sum() == 4
    assert d[4, 15] == 1 and d[0, 0] == 2 and d[0, 15] == 1


def test_new_symbols_resolve():
    from cfdamd import _lib
    L = _lib.load()
    for s in ("cfd_tracers_enable", "cfd_tracers_disable", "cfd_tracers_count", "cfd_tracers_get",
              "cfd_tracers_set", "cfd_tracers_advance", "cfd_tracers_inject", "cfd_tracers_density",
              "cfd_run_set_tracers", "cfd_run_last_tracers"):
        assert s in _lib.EXPORTS
        assert getattr(L, s).argtypes is not None, s
    assert L.cfd_abi_version() == 1
    # argument errors come back before any device is touched
    assert L.cfd_tracers_enable(None, 100, 0) == _lib.CFD_EINVAL
    assert L.cfd_tracers_count(None, None) == _lib.CFD_EINVAL
