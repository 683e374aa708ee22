"""CPU: the premises of tests/test_gpu_resident_seams.py, from the oracle alone.

The GPU file compares k_jacobi_resident with oracle/cfd_oracle.c bit for bit
on grids that sit on its tile seams.  A comparison only has teeth where the
oracle's own result depends on what the kernel could get wrong, so each
premise is asserted here with OracleModel.jacobi() and nothing else:

  * the per-shape tolerance lists (_util.RES_P_TOLS) put the reference's early
    exit (model.rs:816) on every sweep of the kernel's first 10-sweep block,
    on three stages of a later block and on the 50-sweep limit;
  * on the grids whose last tile row is the single row ny-1, row ny-2 at a
    solve's last sweep differs from that row one and two sweeps earlier, so a
    row ny-1 copied from a stale row ny-2 cannot match;
  * one NaN planted beside a tile seam spoils more than nothing and at most
    20 % of a 4-sweep result, so nan_equal comparisons still compare;
  * the whole-step cases break the corrector loop early at least once (the
    kernel's check_break path and its pass_off early return run).
"""
import numpy as np
import pytest

from _util import (ADV_FIELDS, adversarial_state, exit_stages_missing, exit_sweep, jacobi_history,
                   load_state, nonfinite_share, RES_ITERS, RES_LIMIT, RES_MID_EXITS,
                   RES_NAN_ITERS, RES_NAN_SHAPES, RES_P_TOLS, RES_SHAPES, RES_STEP_CASES, RES_STEP_LOOSE, RES_T, RES_WIDE,
                   RES_WIDE_BC, RES_WIDE_BR, RES_WIDE_P_TOLS, RES_WIDE_SPIKES, resident_spike_columns,
                   resident_spike_rows, resident_step_case, same_f32, seam_nan_cells,
                   seam_nan_state, spacing, SPACINGS, spike_state, stale_row_indistinct,
                   tol_exiting_at)
from oracle import OracleModel

MAX_NONFINITE_SHARE = 0.20   # as tests/test_gpu_adversarial.py
SINGLE_ROW = [(nx, ny) for nx, ny in RES_SHAPES if ny % 8 == 1]
NAN_SHAPES = RES_NAN_SHAPES


def _solve(nx, ny, kind, pp, rhs, **kw):
    lx, ly = spacing(nx, ny, kind)
    o = OracleModel(nx, ny, lx, ly, **kw)
    o.field("p_prime")[:] = pp
    o.field("rhs")[:] = rhs
    r = np.float32(o.jacobi())
    return r, int(o.scalars().jacobi_sweeps_total), o.field("p_prime").copy()


def test_history_is_the_solve():
    """jacobi_history's chained one-sweep solves are the 50-sweep solve, and
    exit_sweep() is where the tolerance-mode solve stops."""
    nx, ny = 96, 17
    for kind in SPACINGS:
        pp, rhs = spike_state(nx, ny, 2, 47, 8)
        fields, res = jacobi_history(nx, ny, kind, pp, rhs)
        for iters, tol, p_tol in ((50, 0, 1e-4), (19, 0, 1e-4), (50, 1, 0.009), (50, 1, 0.0012)):
            r, n, f = _solve(nx, ny, kind, pp, rhs, jacobi_iters=iters, tol_enabled=tol, p_tol=p_tol)
            want = exit_sweep(res, p_tol, iters) if tol else iters
            assert n == want and same_f32(r, res[n]), (kind, iters, tol, p_tol, n, want)
            assert np.array_equal(f.view(np.uint32), fields[n].view(np.uint32))


@pytest.mark.parametrize("kind", SPACINGS)
@pytest.mark.parametrize("nx,ny", RES_SHAPES)
def test_spike_tolerances_cover_every_exit_stage(nx, ny, kind):
    exits = set()
    for col in resident_spike_columns(nx):
        for row in resident_spike_rows(ny):
            pp, rhs = spike_state(nx, ny, 2, col, row)
            fields, res = jacobi_history(nx, ny, kind, pp, rhs)
            for p_tol in RES_P_TOLS[(nx, ny, kind)]:
                n = exit_sweep(res, p_tol)
                exits.add(n)
                if ny % 8 == 1:
                    assert not stale_row_indistinct(fields, n, nx, ny), (col, row, p_tol, n)
    assert not exit_stages_missing(exits), (sorted(exits), exit_stages_missing(exits))
    assert RES_T == 10 and RES_LIMIT == 50


def test_stage_rule_has_teeth():
    full = set(range(1, 11)) | {13, 27, 41, 50}
    assert not exit_stages_missing(full)
    for drop in (1, 9, 10, 50, 27):
        assert exit_stages_missing(full - {drop}), drop


@pytest.mark.parametrize("kind", SPACINGS)
def test_wide_grid_spikes(kind):
    """The 800-wide grid's short list: an exit in the first block, one in a
    later block and the limit; its last tile row is the single row ny-1 and a
    stale copy would show in every solve."""
    nx, ny = RES_WIDE
    assert ny % RES_WIDE_BR == 1 and RES_WIDE_BR != 8
    exits = set()
    for col, row in RES_WIDE_SPIKES:
        pp, rhs = spike_state(nx, ny, 2, col, row)
        fields, res = jacobi_history(nx, ny, kind, pp, rhs)
        for p_tol in RES_WIDE_P_TOLS:
            n = exit_sweep(res, p_tol)
            exits.add(n)
            assert not stale_row_indistinct(fields, n, nx, ny), (col, row, p_tol, n)
    assert [e for e in exits if e < RES_T and e % RES_T] and RES_LIMIT in exits, sorted(exits)
    assert [e for e in exits if RES_T < e < RES_LIMIT and e % RES_T], sorted(exits)
    assert {c for c, _ in RES_WIDE_SPIKES} >= {RES_WIDE_BC - 1, RES_WIDE_BC}


@pytest.mark.parametrize("flavour", ["signs", "range"])
@pytest.mark.parametrize("kind", SPACINGS)
@pytest.mark.parametrize("nx,ny", RES_SHAPES + [RES_WIDE])
def test_adversarial_solves(nx, ny, kind, flavour):
    """signs / range: 1e-4 runs every sweep count of RES_ITERS to its limit,
    the two loose tolerances exit in the middle of the first and of the second
    block, everything stays finite, and on the single-row-tile grids a stale
    row ny-2 would show after every sweep count."""
    st = adversarial_state(nx, ny, 1, flavour)
    fields, res = jacobi_history(nx, ny, kind, st["p_prime"], st["rhs"])
    assert all(np.isfinite(f).all() for f in fields)
    assert exit_sweep(res, 1e-4) == RES_LIMIT
    for k in RES_MID_EXITS:
        tol = tol_exiting_at(res, k)
        assert tol is not None and exit_sweep(res, tol) == k and k % RES_T, (k, tol)
    br = RES_WIDE_BR if (nx, ny) == RES_WIDE else 8
    if ny % br == 1:
        for n in set(RES_ITERS) | set(RES_MID_EXITS):
            assert not stale_row_indistinct(fields, n, nx, ny), n


def test_single_row_shapes():
    assert SINGLE_ROW == [(16, 9), (24, 9), (56, 9), (96, 17), (16, 65), (16, 257)]
    assert 37 % 8 == 5 and 72 % 8 == 0 and 16 % 8 == 0      # the controls


@pytest.mark.parametrize("nan_in", ["p_prime", "rhs"])
@pytest.mark.parametrize("kind", SPACINGS)
@pytest.mark.parametrize("nx,ny", NAN_SHAPES + [RES_WIDE])
def test_planted_nan_share(nx, ny, kind, nan_in):
    br, bc = (RES_WIDE_BR, RES_WIDE_BC) if (nx, ny) == RES_WIDE else (8, 48)
    cells = seam_nan_cells(nx, ny, br, bc)
    assert cells
    for cell in cells:
        pp, rhs = seam_nan_state(nx, ny, cell, nan_in)
        r, n, f = _solve(nx, ny, kind, pp, rhs, jacobi_iters=RES_NAN_ITERS, tol_enabled=1, p_tol=1e-4)
        assert n == RES_NAN_ITERS and np.isfinite(r) and r > 0.0, (cell, n, r)
        assert 0.0 < nonfinite_share([f]) <= MAX_NONFINITE_SHARE, (cell, nonfinite_share([f]))


def test_nan_cells_sit_on_the_seams():
    assert seam_nan_cells(96, 17) == [(48, 7), (48, 8), (47, 8), (48, 8)]
    assert seam_nan_cells(24, 9) == [(12, 7)]
    assert seam_nan_cells(48, 8) == [] and seam_nan_cells(16, 4) == []
    assert (16, 9) not in NAN_SHAPES and (24, 9) in NAN_SHAPES and (96, 17) in NAN_SHAPES
    pp, rhs = seam_nan_state(16, 9, (8, 7), "p_prime")
    _, _, f = _solve(16, 9, "pow2", pp, rhs, jacobi_iters=RES_NAN_ITERS, tol_enabled=1, p_tol=1e-4)
    assert nonfinite_share([f]) > MAX_NONFINITE_SHARE      # why 16 x 9 is left out


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("name", sorted(RES_STEP_CASES))
def test_whole_steps_break_the_corrector_loop(name, scheme):
    """Two steps from the `signs` state with 20 corrector passes stay finite;
    under the default tolerance every pass runs every sweep, under the loose
    one a step ends its corrector loop early: fewer sweeps than the first
    solve, 19 full passes and one more sweep need."""
    g, kw = resident_step_case(name)
    for p_tol, early in ((1e-4, False), (RES_STEP_LOOSE[name], True)):
        o = OracleModel(**g, scheme=scheme, corrector_passes=20, p_tol=p_tol, **kw)
        load_state(adversarial_state(g["nx"], g["ny"], 1, "signs"), oracle=o)
        per_step, before = [], 0
        for step in range(2):
            o.update()
            total = int(o.scalars().jacobi_sweeps_total)
            per_step.append(total - before)
            before = total
        assert nonfinite_share([o.field(f) for f in ADV_FIELDS]) == 0.0, (name, scheme)
        if early:
            assert min(per_step) < 1 + 19 * RES_LIMIT + 1, per_step
        else:
            assert per_step == [21 * RES_LIMIT] * 2, per_step
