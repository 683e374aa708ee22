"""GPU: k_jacobi_resident at its tile seams and at every exit stage.

The resident solve (cfd_jacobi_resident.hip) is what the reference's own
configuration runs: the tolerance on, Jacobi, one domain of at most 2^21
cells.  It cuts the grid into tiles of BR x BC output cells with a 10-cell
halo cone, recomputes boundary rows and columns in LDS, separates blocks of
10 sweeps by a two-level grid barrier and re-runs a block with exactly j + 1
sweeps on an early exit.  Everything here is bitwise against
oracle/cfd_oracle.c, through the default selection (CFD_RESIDENT unset); every
case asserts kind 6, the tile plan it relies on (Model.resident_geometry) and
the count of resident solves.  The premises -- exit stages covered, a stale
row ny-2 would show, the NaN share -- are pinned without a GPU in
tests/test_resident_seams_cpu.py.

shape        what it pins (tiles of 8 x 48 unless noted)
16x4         smallest grid: one tile touching all four edges, one workgroup
48x8         exactly one full tile
16x9, 24x9   one tile column; the last tile is the single row ny-1
56x9         an 8-column last tile column and a single-row last tile row
             (the corner tile is 8 x 1)
104x16       tile columns 48 + 48 + 8, no ragged row
96x17        two full columns, three tile rows, the last single
120x37       the control of test_gpu_adversarial.py (37 % 8 == 5)
16x65, 16x72, 16x257   9, 9 and 33 workgroups: barrier groups of unequal size
             (G % 8 != 0); 65 and 257 end in a single-row tile, 72 does not
800x248      8 x 48 no longer fits 256 CUs: tiles of 19 x 46, 248 % 19 == 1

A tile row of the single row ny-1 holds no interior row, and row ny-1 is a copy
of the same sweep's row ny-2: the kernel computes row ny-2 in that tile too
(before this file it copied a row two sweeps old; the single-row shapes here
failed on it).
"""
import numpy as np
import pytest

from _util import (ADV_FIELDS, adversarial_state, assert_bitwise, exit_stages_missing,
                   jacobi_history, load_state, nonfinite_share, RES_ITERS, RES_LIMIT, RES_MID_EXITS,
                   RES_NAN_ITERS, RES_NAN_SHAPES, RES_P_TOLS, RES_SHAPES, RES_STEP_CASES,
                   RES_STEP_LOOSE, RES_T, RES_WIDE, RES_WIDE_BC, RES_WIDE_BR, RES_WIDE_P_TOLS,
                   RES_WIDE_SPIKES, resident_spike_columns, resident_spike_rows,
                   resident_step_case, same_f32, seam_nan_cells, seam_nan_state, spacing, SPACINGS,
                   spike_state, tol_exiting_at)

pytestmark = pytest.mark.gpu

MAX_NONFINITE_SHARE = 0.20
SINGLE_ROW = {(16, 9), (24, 9), (56, 9), (96, 17), (16, 65), (16, 257), RES_WIDE}
ALL_SHAPES = RES_SHAPES + [RES_WIDE]


def _cfd():
    import cfdamd
    return cfdamd


def _params(**kw):
    c = _cfd()
    return c.SimulationParams(
        viscosity=kw.get("viscosity", 1e-6), velocity_scheme=c.VelocityScheme(kw.get("scheme", 0)),
        jacobi_iters=kw.get("jacobi_iters", 50), corrector_passes=kw.get("corrector_passes", 20),
        tol_enabled=True, p_tol=kw.get("p_tol", 1e-4), bc_kind=c.BoundaryKind(kw.get("bc_kind", 0)))


def _pair(g, **kw):
    """The cfdamd.Model and the OracleModel of one grid and parameter set."""
    c = _cfd()
    from oracle import OracleModel
    cyl = g.get("cylinder")
    m = c.Model(c.Grid(g["nx"], g["ny"], g["lx"], g["ly"], c.Cylinder(*cyl) if cyl else None),
                _params(**kw))
    o = OracleModel(g["nx"], g["ny"], g["lx"], g["ly"], cylinder=cyl, tol_enabled=1, **kw)
    return m, o


def _set_solve(m, o, **kw):
    """Another sweep limit and tolerance for both models of a pair."""
    m.set_parameters(_params(**kw))
    o.set_params(tol_enabled=1, **kw)


def _solve_pair(nx, ny, kind, **kw):
    lx, ly = spacing(nx, ny, kind)
    return _pair(dict(nx=nx, ny=ny, lx=lx, ly=ly), **kw)


def _assert_plan(m, nx, ny, kind=None):
    """Kind 6, the division form of the spacing and the tile plan the case
    relies on: the single-row last tile row where the shape claims one."""
    jk = m.jacobi_kernel
    assert jk["kind"] == 6, jk
    if kind is not None:
        assert jk["name"] == ("k_jacobi_resident<1>" if kind == "pow2" else "k_jacobi_resident<0>"), jk
    geo = m.resident_geometry
    br, bc = (RES_WIDE_BR, RES_WIDE_BC) if (nx, ny) == RES_WIDE else (8, 48)
    tiles = -(-nx // bc) * -(-ny // br)
    assert geo == dict(br=br, bc=bc, tiles=tiles, wgs=tiles), (nx, ny, geo)
    assert (ny % geo["br"] == 1) == ((nx, ny) in SINGLE_ROW), (nx, ny, geo)
    if (nx, ny) == RES_WIDE:
        assert geo["br"] != 8 and ny % geo["br"] == 1, geo
    return geo


def _solve_and_compare(tag, m, o, pp, rhs, nan_equal=False):
    """One jacobi_pressure() on (p', rhs): residual, sweep count and p'
    against the oracle.  Returns (residual, sweeps)."""
    o.field("p_prime")[:] = pp
    o.field("rhs")[:] = rhs
    s = o.scalars()
    s.jacobi_sweeps_total = 0
    o.set_scalars(s)
    m.set_state(p_prime=pp, rhs=rhs, jacobi_sweeps_total=0)
    want = np.float32(o.jacobi())
    got = np.float32(m.jacobi_pressure())
    sweeps = int(o.scalars().jacobi_sweeps_total)
    st = m.get_state()
    assert np.isfinite(want), tag
    assert same_f32(got, want), (tag, got, want)
    assert st["jacobi_sweeps_total"] == sweeps, (tag, st["jacobi_sweeps_total"], sweeps)
    assert_bitwise(tag, st["p_prime"], o.field("p_prime"), nan_equal=nan_equal)
    return want, sweeps


# ------------------------------------------------------------- the getter

def test_geometry_getter_refuses_other_solves():
    """CFD_ESTATE where the model would not take the resident solve: the
    tolerance off, and SOR."""
    c = _cfd()
    for params in (c.SimulationParams(tol_enabled=False),
                   c.SimulationParams(pressure_solver=c.PressureSolver(1))):
        m = c.Model(c.Grid(96, 17, 0.75, 17 / 128.0), params)
        try:
            assert m.jacobi_kernel["kind"] != 6
            with pytest.raises(c.CfdError) as ei:
                m.resident_geometry
            assert ei.value.code == -4, ei.value
        finally:
            m.close()


# ------------------------------------------------------------ spike solves

@pytest.mark.parametrize("kind", SPACINGS)
@pytest.mark.parametrize("nx,ny", ALL_SHAPES, ids=[f"{a}x{b}" for a, b in ALL_SHAPES])
def test_spike_solves_every_exit_stage(nx, ny, kind):
    """p' = 1 planted on noise of 1e-3 at the residual's column edges, both
    sides of the tile-column seams, and rows 1, 7, 8, ny-3, ny-2, under every
    tolerance of the shape's list: the exits the device reports cover every
    sweep of the first block (j = 0..9, j = 9 without a re-run), three stages
    of a later block and the 50-sweep limit.  The 800-wide grid takes its short
    list (_util.RES_WIDE_SPIKES): an exit in the first block, in a later one,
    and the limit."""
    wide = (nx, ny) == RES_WIDE
    spikes = RES_WIDE_SPIKES if wide else [(c, r) for c in resident_spike_columns(nx)
                                           for r in resident_spike_rows(ny)]
    exits = set()        # sweep counts the device reported (each equal to the oracle's)
    tols = RES_WIDE_P_TOLS if wide else RES_P_TOLS[(nx, ny, kind)]
    m, o = _solve_pair(nx, ny, kind, jacobi_iters=RES_LIMIT)
    try:
        for p_tol in tols:
            _set_solve(m, o, p_tol=p_tol, jacobi_iters=RES_LIMIT)
            _assert_plan(m, nx, ny, kind)
            for col, row in spikes:
                pp, rhs = spike_state(nx, ny, 2, col, row)
                _, sweeps = _solve_and_compare(f"{nx}x{ny} {kind} p_tol {p_tol} spike ({col},{row})",
                                               m, o, pp, rhs)
                exits.add(sweeps)
        assert m.resident_solves == len(spikes) * len(tols), m.resident_solves
    finally:
        m.close()
    if wide:
        assert [e for e in exits if e < RES_T] and RES_LIMIT in exits, sorted(exits)
        assert [e for e in exits if RES_T < e < RES_LIMIT and e % RES_T], sorted(exits)
    else:
        assert not exit_stages_missing(exits), (sorted(exits), exit_stages_missing(exits))


# --------------------------------------------------- signs and range solves

@pytest.mark.parametrize("flavour", ["signs", "range"])
@pytest.mark.parametrize("kind", SPACINGS)
@pytest.mark.parametrize("nx,ny", ALL_SHAPES, ids=[f"{a}x{b}" for a, b in ALL_SHAPES])
def test_adversarial_solves(nx, ny, kind, flavour):
    """Random p' and rhs of both signs / of 43 binades: jacobi_iters 1, 2, 3
    (blocks of 1, 2 and 3 sweeps), 9, 10, 11 (both sides of the block
    boundary), 19 (a ragged last block) and 50, each under 1e-4 (to the limit)
    and under two loose tolerances built from the oracle's residual history to
    exit at sweeps 4 and 14, the middle of the first and of the second block."""
    st = adversarial_state(nx, ny, 1, flavour)
    pp, rhs = st["p_prime"], st["rhs"]
    _, res = jacobi_history(nx, ny, kind, pp, rhs)
    tols = [(1e-4, None)] + [(tol_exiting_at(res, k), k) for k in RES_MID_EXITS]
    assert all(t is not None for t, _ in tols), tols
    m, o = _solve_pair(nx, ny, kind)
    try:
        solves = 0
        for iters in RES_ITERS:
            for p_tol, k in tols:
                if k is not None and k > iters:
                    continue        # the same solve as 1e-4's
                _set_solve(m, o, p_tol=p_tol, jacobi_iters=iters)
                _assert_plan(m, nx, ny, kind)
                _, sweeps = _solve_and_compare(f"{nx}x{ny} {kind} {flavour} iters {iters} p_tol {p_tol}",
                                               m, o, pp, rhs)
                solves += 1
                assert sweeps == (iters if k is None else k), (iters, p_tol, sweeps)
        assert m.resident_solves == solves, (m.resident_solves, solves)
    finally:
        m.close()


# ------------------------------------------------------------- planted NaN

NAN_SHAPES = RES_NAN_SHAPES + [RES_WIDE]


@pytest.mark.parametrize("nan_in", ["p_prime", "rhs"])
@pytest.mark.parametrize("kind", SPACINGS)
@pytest.mark.parametrize("nx,ny", NAN_SHAPES, ids=[f"{a}x{b}" for a, b in NAN_SHAPES])
def test_nan_beside_a_seam(nx, ny, kind, nan_in):
    """`signs` with one NaN beside a tile seam (rows br-1 and br, columns bc-1
    and bc), 4 sweeps: the NaN crosses the seam inside the halo cone; the
    residual ignores it (finite, equal), p' matches with any NaN for any NaN,
    and most of the oracle's field stays finite.  16 x 9 is left out: the NaN
    spoils more than 20 % of it (test_resident_seams_cpu.py)."""
    m, o = _solve_pair(nx, ny, kind, jacobi_iters=RES_NAN_ITERS)
    try:
        geo = _assert_plan(m, nx, ny, kind)
        cells = seam_nan_cells(nx, ny, geo["br"], geo["bc"])
        assert cells
        for cell in cells:
            pp, rhs = seam_nan_state(nx, ny, cell, nan_in)
            want, sweeps = _solve_and_compare(f"{nx}x{ny} {kind} NaN in {nan_in} at {cell}", m, o, pp,
                                              rhs, nan_equal=True)
            assert sweeps == RES_NAN_ITERS and want > 0.0, (sweeps, want)
            share = nonfinite_share([o.field("p_prime")])
            assert 0.0 < share <= MAX_NONFINITE_SHARE, share
        assert m.resident_solves == len(cells), m.resident_solves
    finally:
        m.close()


# -------------------------------------------------------------- whole steps

def _compare_step(tag, m, o):
    st = m.get_state()
    for f in ADV_FIELDS:
        assert_bitwise(f"{tag}: {f}", st[f], o.field(f))
    s = o.scalars()
    assert st["simulation_step"] == s.step, tag
    assert st["jacobi_sweeps_total"] == s.jacobi_sweeps_total, (tag, st["jacobi_sweeps_total"],
                                                                s.jacobi_sweeps_total)
    for k, want in (("dt", s.dt), ("simulation_time", s.time), ("last_p_residual", s.p),
                    ("last_u_residual", s.u), ("last_v_residual", s.v)):
        assert same_f32(st[k], want), (tag, k, st[k], want)


@pytest.mark.parametrize("loose", [False, True], ids=["default", "loose"])
@pytest.mark.parametrize("passes", [0, 20])
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("name", sorted(RES_STEP_CASES))
def test_step_with_the_tolerance_on(name, scheme, passes, loose):
    """update() from the `signs` state with the tolerance on, two steps, every
    field and scalar after each.  Under the default 1e-4 every pass runs every
    sweep; under the loose tolerance a step of the 20-pass cases leaves the
    corrector loop early (test_resident_seams_cpu.py): the solves of passes
    >= 1 decide the break on the device (check_break) and the launches behind
    the break return at pass_off, workgroup 0 finalizing."""
    g, kw = resident_step_case(name)
    p_tol = RES_STEP_LOOSE[name] if loose else 1e-4
    m, o = _pair(g, scheme=scheme, corrector_passes=passes, p_tol=p_tol, **kw)
    try:
        _assert_plan(m, g["nx"], g["ny"], RES_STEP_CASES[name][2])
        load_state(adversarial_state(g["nx"], g["ny"], 1, "signs"), model=m, oracle=o)
        per_step, before = [], 0
        for step in range(2):
            o.update()
            m.update()
            _compare_step(f"{name} scheme {scheme} passes {passes} p_tol {p_tol} step {step + 1}", m, o)
            total = int(o.scalars().jacobi_sweeps_total)
            per_step.append(total - before)
            before = total
        if loose and passes == 20:
            assert min(per_step) < 1 + 19 * RES_LIMIT + 1, per_step
        m.get_residuals()
        # one launch per solve of the step's sequence, the passes behind a break included
        assert m.resident_solves == 2 * (1 + passes), m.resident_solves
    finally:
        m.close()


@pytest.mark.parametrize("name", ["24x9", "96x17"])
def test_batched_steps_equal_single_steps(name):
    """update_n(3) and three update() calls from the same loaded state give the
    same bits (and the oracle's)."""
    g, kw = resident_step_case(name)
    kw = dict(kw, corrector_passes=2, p_tol=RES_STEP_LOOSE[name])
    st0 = adversarial_state(g["nx"], g["ny"], 1, "signs")
    a, o = _pair(g, **kw)
    b, _ = _pair(g, **kw)
    try:
        _assert_plan(a, g["nx"], g["ny"], "pow2")
        load_state(st0, model=a, oracle=o)
        load_state(st0, model=b)
        a.update_n(3)
        for _ in range(3):
            b.update()
            o.update()
        sa, sb = a.get_state(), b.get_state()
        for f in ADV_FIELDS:
            assert_bitwise(f"{name} batched vs single: {f}", sa[f], sb[f])
        for k in ("dt", "simulation_time", "last_p_residual", "last_u_residual", "last_v_residual"):
            assert same_f32(sa[k], sb[k]), (k, sa[k], sb[k])
        assert sa["jacobi_sweeps_total"] == sb["jacobi_sweeps_total"]
        assert sa["simulation_step"] == sb["simulation_step"]
        _compare_step(f"{name} three steps", b, o)
        assert a.resident_solves == b.resident_solves == 3 * 3, (a.resident_solves, b.resident_solves)
    finally:
        a.close()
        b.close()
