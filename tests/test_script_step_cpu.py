"""CPU: the substep restatement (tests/_script_step_ref.py) against the script's
own fields under node (tests/golden/js_step_*.npz), the manifest's branch
claims, and the host's obstacle form.  Every comparison is bitwise."""
import numpy as np
import pytest

import _script_step_ref as ref
from _script_step_golden import FIXTURES, MANIFEST, load_fixture


def test_fixture_set():
    fx = MANIFEST["fixtures"]
    assert len(FIXTURES) == 9
    assert {(f["scheme"], f["solver"]) for f in fx.values()} == {(s, q) for s in (0, 1, 2) for q in (2, 4)}
    assert {f["profile"] for f in fx.values()} == {0, 1}
    assert {(16, 4), (16, 5), (24, 7)} <= {(f["nx"], f["ny"]) for f in fx.values()}
    assert any(f["nx"] == 264 and f["ny"] > 8 for f in fx.values())   # a wave seam and a row seam
    for scheme in ref.SCHEME_NAMES:
        tot = {c: 0 for c in ref.counter_names(scheme)}
        for f in fx.values():
            if f["scheme"] == scheme:
                assert f["cylinder"] is None or f["branches"]["u_obstacle"] > 0
                for c, n in f["branches"].items():
                    tot[c] += n
        assert all(n > 0 for n in tot.values()), (scheme, [c for c, n in tot.items() if n == 0])


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_node(name):
    meta, g, a = load_fixture(name)
    counters = {}
    us, vs, rhs = ref.predict(g, a["in_u"], a["in_v"], meta["dt_sub"], meta["scheme"], counters)
    for nm, got in (("u_star", us), ("v_star", vs), ("rhs", rhs)):
        assert ref.bits_equal(got, a[nm]), (name, nm)
    assert counters == meta["branches"], name
    u, v, p = ref.correct(g, a["u_star"], a["v_star"], a["p_prime"], a["in_p"], meta["dt_sub"],
                          meta["inlet_velocity"], meta["profile"])
    for nm, got in (("u", u), ("v", v), ("p", p)):
        assert ref.bits_equal(got, a[nm]), (name, nm)


def _grids():
    out = [load_fixture(n)[1] for n in FIXTURES]
    out.append(ref.Grid(800, 264, 30.0, 10.0, 1e-6, (7.5, 5.0, 0.75)))   # the default grid
    return out


def test_obstacle_intervals_equal_per_face_evaluation():
    for g in _grids():
        for m in ref.obstacle_faces(g):
            iv = ref.obstacle_intervals(m)
            assert np.array_equal(ref.intervals_to_mask(iv, m.shape[1]), m), (g.nx, g.ny)
            assert (g.cyl is not None) == bool(m.any())


def test_unvisited_faces_keep_their_values_and_walls_are_zero():
    meta, g, a = load_fixture("js_step_16x5_quick_mg")
    assert ref.bits_equal(a["u_star"][[0, -1]], a["in_u"][[0, -1]])
    assert ref.bits_equal(a["u_star"][:, [0, -1]], a["in_u"][:, [0, -1]])
    assert ref.bits_equal(a["v_star"][[0, -1]], a["in_v"][[0, -1]])
    assert ref.bits_equal(a["v_star"][:, [0, -1]], a["in_v"][:, [0, -1]])
    assert not a["u"][[0, -1]].any() and not a["v"][[0, -1]].any()


def test_abi_symbols():
    from cfdamd import _lib
    assert {"cfd_script_piso_step", "cfd_script_phase"} <= set(_lib.EXPORTS)
    import cfdamd
    assert [int(s) for s in cfdamd.ScriptScheme] == [0, 1, 2]
