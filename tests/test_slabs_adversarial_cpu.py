"""CPU: the premises of tests/test_gpu_slabs_adversarial.py, with the oracle alone.

The GPU tests compare slabs started from adversarial single-domain states
with oracle/cfd_oracle.c and lean on facts about the oracle's side of those
inputs: how much of a `nonfinite` step's result is non-finite (nan_equal must
not hide the comparison), that `signs` and `range` stay finite, that no solve
of the tolerance-mode step exits early, where the tolerance list's spike
solves exit, that the spike tells the residual's last included column from
the first excluded one on the slab-boundary rows too, and -- what makes
these tests stronger than the from-rest ones -- that the rows either side of
every slab boundary carry non-zero data.  They are asserted here, wherever
the suite runs.
"""
import numpy as np
import pytest

from _slabs import (FIXED_FORMS, FIXED_SWEEPS, MAX_NONFINITE_SHARE, SOLVER_LAYOUTS, STEP_LAYOUTS,
                    STEP_ROWS, TOL_FORMS, TOL_GRID, TOL_KW, TOL_STEP_SWEEPS, boundary_rows,
                    clean_ranks, fixed_spikes, grid_of, has_clean_rank, layout_id, slab_bounds,
                    solver_kw, sor_refused, step_cases, step_count, step_kw, tol_spikes)
from _util import (ADV_FIELDS, adversarial_state, load_state, nonfinite_share, SPIKE_P_TOLS,
                   spike_state)
from oracle import OracleModel

MIN_NONZERO = 0.90


def _oracle(g, **kw):
    return OracleModel(g["nx"], g["ny"], g["lx"], g["ly"], cylinder=g.get("cylinder"), **kw)


def _nonzero_share(a, pitch, rows):
    return np.count_nonzero(a.reshape(-1, pitch)[rows]) / float(len(rows) * pitch)


def test_slab_plan_of_every_layout():
    """The row counts the layouts were chosen for, from cfd_plan_slab."""
    for name, n, depth, want_depth, _ in STEP_LAYOUTS:
        ny = grid_of(name)[0]["ny"]
        edges = [0] + slab_bounds(ny, n) + [ny]
        assert [b - a for a, b in zip(edges, edges[1:])] == STEP_ROWS[(name, n)], (name, n)
        assert want_depth == min(8 if depth is None else depth, ny // n - 2), (name, n)
    assert boundary_rows(37, 3) == [12, 13, 24, 25] and boundary_rows(16, 2) == [7, 8]
    # 128 x 64 on 4: boundaries that divide by 2, 4 and 8
    assert slab_bounds(64, 4) == [16, 32, 48]
    # SOR on slabs: 19 / 18 rows pass, the outer two of four 16-row slabs do not
    assert [sor_refused(grid_of(s[0])[0]["ny"], s[1]) for s in SOLVER_LAYOUTS] == [False, True]
    # the tolerance forms: speculative blocks need 16 rows a slab, 3 ranks have fewer
    ny = grid_of(TOL_GRID)[0]["ny"]
    for _, n, _, _ in TOL_FORMS:
        assert (ny // n >= 16) == (n == 2)


@pytest.mark.parametrize("passes", [0, 2])
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("layout,flavour", step_cases(),
                         ids=[f"{layout_id(lay)}-{fl}" for lay, fl in step_cases()])
def test_step_premises(layout, flavour, scheme, passes):
    """2a on the oracle: the non-finite share of a `nonfinite` step is above 0
    and within the cap, that of `signs` and `range` is 0; the boundary rows
    of the loaded state carry non-zero words in u, v and p', and p' still
    does after the first step."""
    name, n = layout[0], layout[1]
    g, _ = grid_of(name)
    nx, ny = g["nx"], g["ny"]
    o = _oracle(g, **step_kw(layout, flavour, scheme, passes))
    st = adversarial_state(nx, ny, 1, flavour)
    load_state(st, oracle=o)
    rows = boundary_rows(ny, n)
    for f, pitch in (("u", nx + 1), ("v", nx), ("p_prime", nx)):
        assert _nonzero_share(st[f], pitch, rows) >= MIN_NONZERO, (f, rows)
    for step in range(step_count(flavour)):
        o.update()
        if step == 0:
            assert _nonzero_share(o.field("p_prime"), nx, rows) >= MIN_NONZERO, rows
    share = nonfinite_share([o.field(f) for f in ADV_FIELDS])
    if flavour == "nonfinite":
        assert 0.0 < share <= MAX_NONFINITE_SHARE, share
        # slabs the non-finite words do not reach: where the table says, and some exist
        assert bool(clean_ranks(o, nx, ny, n)) == has_clean_rank(layout, scheme, passes)
    else:
        assert share == 0.0, share


@pytest.mark.parametrize("flavour", ["signs", "range"])
def test_tolerance_step_runs_every_sweep(flavour):
    """2b: three solves of 50 sweeps, none exits early, the result is finite."""
    g, _ = grid_of(TOL_GRID)
    o = _oracle(g, **TOL_KW)
    load_state(adversarial_state(g["nx"], g["ny"], 1, flavour), oracle=o)
    o.update()
    assert o.scalars().jacobi_sweeps_total == TOL_STEP_SWEEPS
    assert nonfinite_share([o.field(f) for f in ADV_FIELDS]) == 0.0
    for n in sorted({f[1] for f in TOL_FORMS}):
        assert _nonzero_share(o.field("p_prime"), g["nx"], boundary_rows(g["ny"], n)) >= MIN_NONZERO


def _solve(g, col, row, **kw):
    o = _oracle(g, **kw)
    pp, rhs = spike_state(g["nx"], g["ny"], 2, col, row)
    o.field("p_prime")[:] = pp
    o.field("rhs")[:] = rhs
    res = np.float32(o.jacobi())
    return res, int(o.scalars().jacobi_sweeps_total)


@pytest.mark.parametrize("form", FIXED_FORMS, ids=[f[0] for f in FIXED_FORMS])
def test_spike_discriminates_columns_on_boundary_rows(form):
    """2c, fixed counts: with the spike on a slab-boundary row, column nx-8
    (the last the residual covers) and nx-7 give different results at every
    sweep count, and the boundary rows are among the spikes."""
    g, _ = grid_of(TOL_GRID)
    nx, ny, n = g["nx"], g["ny"], form[1]
    spikes = fixed_spikes(nx, ny, n)
    for row in boundary_rows(ny, n):
        assert (nx - 8, row) in spikes and (nx - 7, row) in spikes
        for iters in FIXED_SWEEPS:
            a = _solve(g, nx - 8, row, bc_kind=1, jacobi_iters=iters, tol_enabled=0)
            b = _solve(g, nx - 7, row, bc_kind=1, jacobi_iters=iters, tol_enabled=0)
            assert a != b, (row, iters, a, b)


@pytest.mark.parametrize("n", sorted({f[1] for f in TOL_FORMS}))
def test_trimmed_tolerance_list_exit_sweeps(n):
    """2c, tolerance on: over the trimmed spike product the exit sweeps cover
    at least three residues mod 8, a non-zero one among them, one solve runs
    to the limit, and nx-8 differs from nx-7 on every row at every tolerance."""
    g, _ = grid_of(TOL_GRID)
    nx, ny = g["nx"], g["ny"]
    spikes = tol_spikes(nx, ny, n)
    b = slab_bounds(ny, n)[0]
    assert {r for _, r in spikes} == {b - 1, b, ny - 2}
    assert {nx - 8, nx - 7, 112, 113} <= {c for c, _ in spikes}
    exits = set()
    for p_tol in SPIKE_P_TOLS:
        res = {s: _solve(g, s[0], s[1], bc_kind=1, jacobi_iters=50, tol_enabled=1, p_tol=p_tol)
               for s in spikes}
        exits.update(sweeps for _, sweeps in res.values())
        for row in (b - 1, b, ny - 2):
            assert res[(nx - 8, row)] != res[(nx - 7, row)], (p_tol, row, res)
    residues = {e % 8 for e in exits}
    assert len(residues) >= 3 and residues - {0}, sorted(exits)
    assert 50 in exits and min(exits) < 8, sorted(exits)


@pytest.mark.parametrize("passes", [0, 2])
@pytest.mark.parametrize("flavour", ["signs", "range"])
@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("layout", SOLVER_LAYOUTS, ids=[f"{s[0]}-n{s[1]}" for s in SOLVER_LAYOUTS])
def test_solver_steps_stay_finite(layout, solver, flavour, passes):
    """2d: two SOR / multigrid steps from `signs` and `range` stay finite, and
    p' on the boundary rows is non-zero after the first."""
    g, _ = grid_of(layout[0])
    nx, ny = g["nx"], g["ny"]
    o = _oracle(g, **solver_kw(solver, passes))
    load_state(adversarial_state(nx, ny, 1, flavour), oracle=o)
    o.update()
    assert _nonzero_share(o.field("p_prime"), nx, boundary_rows(ny, layout[1])) >= MIN_NONZERO
    o.update()
    assert nonfinite_share([o.field(f) for f in ADV_FIELDS]) == 0.0
