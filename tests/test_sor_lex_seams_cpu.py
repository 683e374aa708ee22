"""CPU: the premises of the script-order SOR's seam tests
(test_gpu_sor_lex_seams.py), checked with the restatement alone
(tests/_sor_lex_ref.py; pinned to the script itself by test_sor_lex_cpu.py):
the anti-diagonal form the device is compared with equals the plain loops on
the table's cases, no case sits where the float and the double exit tests
differ, every exit case exits where the table says, and the band-confined
cases are able to fail -- the band that takes the exit test is below the
tolerance one iteration before the exit while the named band is not."""
import numpy as np
import pytest

import _sor_lex_cases as t
import _sor_lex_ref as ref
from _util import assert_bitwise

NAMES = [c.name for c in t.CASES]
CONFINED = [c.name for c in t.CASES if c.band is not None]


def _loop_sized(c):
    """The plain loops cost a millisecond per row: small grids, or few iterations."""
    return c.nx * c.ny <= 72 * 67 or c.iters <= 20 or (c.n is not None and c.n <= 20)


@pytest.mark.parametrize("name", NAMES)
def test_case_exits_where_the_table_says(name):
    c = t.BY_NAME[name]
    rhs, P, n, errs = t.restated(c)
    assert len(errs) == n and ref.slivers(errs, t.P_TOL) == []
    below = [bool(np.float32(e) < np.float32(t.P_TOL)) for e in errs]
    assert not any(below[:-1])
    if c.exit == "none":
        assert n == c.iters and (not c.tol or not below[-1])
    elif c.exit == "mid":
        assert 1 < n < c.iters and below[-1]
    elif c.exit == "last":
        assert n == c.iters and below[-1]
    else:
        assert c.exit == "first" and n == 1 and below[-1]
    if c.n is not None:
        assert n == c.n
    if c.scale == 0.0:
        assert errs == [0.0] and not P.any()
    else:
        assert P.any()


@pytest.mark.parametrize("name", [c.name for c in t.CASES if _loop_sized(c)])
def test_diagonal_form_matches_loop_form(name):
    c = t.BY_NAME[name]
    rhs, P, n, errs = t.restated(c)
    dx, dy = t.spacings(c)
    L, ln, lerrs = ref.sor_lex_loop(rhs, c.nx, c.ny, dx, dy, c.iters, c.tol, t.P_TOL)
    assert_bitwise(f"{name}: p'", P, L)
    assert ln == n and lerrs == errs


def test_every_grid_has_a_loop_form_check():
    """The bound above leaves no grid of the table without a loop-form case."""
    checked = {(c.nx, c.ny) for c in t.CASES if _loop_sized(c)}
    assert checked == {(c.nx, c.ny) for c in t.CASES}


@pytest.mark.parametrize("name", CONFINED)
def test_confined_cases_can_fail(name):
    """One iteration before the exit the named band is still at or above the
    tolerance; where that is not the last band, the last band -- the one that
    takes the test -- is below it, so a kernel testing the band's own maximum
    would exit early."""
    c = t.BY_NAME[name]
    n = t.restated(c)[2]
    m = t.band_maxima(c, n - 1)
    tol = np.float32(t.P_TOL)
    assert len(m) == t.bands(c.ny)
    assert np.float32(m[c.band]) >= tol, m
    assert np.float32(max(m)) == np.float32(t.restated(c)[3][n - 2])
    if c.band != len(m) - 1:
        assert np.float32(m[-1]) < tol, m


def test_table_covers_the_seams():
    ny2 = {c.ny - 2 for c in t.GEOMETRY_CASES}
    assert {2, 63, 64, 65, 128, 129} <= ny2
    assert {c.nx for c in t.GEOMETRY_CASES} >= {16, 17, 18, 19, 34, 35}
    # on the device both remainders of the last chunk, at the smallest width too
    assert {(c.nx + 62) % 16 for c in t.DEVICE_CASES} == {14, 6}
    assert {(c.nx + 62) % 16 for c in t.CASES if not c.device} >= {0, 1, 15}
    for nx, ny in {(c.nx, c.ny) for c in t.GEOMETRY_CASES}:
        kinds = {(c.tol, c.exit) for c in t.GEOMETRY_CASES if (c.nx, c.ny) == (nx, ny)}
        assert kinds == {(False, "none"), (True, "mid")}, (nx, ny)
    # a one-row last band takes the exit test, once with the maximum in another band
    assert any(c.device and c.exit == "mid" for c in t.ONE_ROW_LAST_BAND)
    assert any(c.device and c.band == 0 for c in t.ONE_ROW_LAST_BAND)
    # multi-band exits of both parities that a model can run
    par = {t.restated(c)[2] % 2 for c in t.DEVICE_CASES
           if c.exit == "mid" and t.bands(c.ny) > 1}
    assert par == {0, 1}
    assert max(c.nx * c.ny for c in t.CASES) <= 40 * 195 and max(c.iters for c in t.CASES) <= 100


def test_widths_off_the_8_grid_are_refused_by_the_constructor():
    """Why those cases stay with the restatement: CFD_EINVAL before any device call."""
    import cfdamd as c
    for nx, ny in sorted({(k.nx, k.ny) for k in t.CASES if not k.device}):
        with pytest.raises(c.CfdError) as e:
            c.Model(c.Grid(nx, ny, 30.0, 10.0),
                    c.SimulationParams(pressure_solver=c.PressureSolver.SorLex))
        assert e.value.code == -1 and "multiple of 8" in str(e.value)
    with pytest.raises(c.CfdError) as e:     # and no grid has fewer than two interior rows
        c.Model(c.Grid(16, 3, 30.0, 10.0), c.SimulationParams(pressure_solver=c.PressureSolver.SorLex))
    assert e.value.code == -1


@pytest.mark.parametrize("k", range(len(t.NONFINITE_CASES)))
def test_nonfinite_cases(k):
    c, word = t.NONFINITE_CASES[k]
    rhs, P, n, errs = t.nonfinite_restated(c, word)
    i, j = t.NONFINITE_CELL
    assert not np.isfinite(rhs[i + j * c.nx]) and np.count_nonzero(~np.isfinite(rhs)) == 1
    bad = ~np.isfinite(P)
    # the word crossed the seam between the last two bands (rows 128 | 129) ...
    assert (c.ny - 2 - 1) // t.BAND == 2 and j > 128 and bad[128].any() and n >= 3
    # ... and the comparison hides little
    assert 0 < bad.mean() <= t.NONFINITE_SHARE
    assert ref.slivers(errs, t.P_TOL) == []
    if c.tol:
        assert n == c.n and 1 < n < c.iters and np.isnan(P).any()
        assert np.isfinite(errs[-1]) and np.float32(errs[-1]) < np.float32(t.P_TOL)
    else:
        assert n == c.iters
        # the script's `error > maxError` ignores NaN and takes +inf
        assert np.isfinite(errs[-1]) if np.isnan(word) else errs[-1] == np.inf
