"""GPU: the row-slab decomposition fed adversarial state, at small shapes.

Every other small comparison of the slabs with the oracle starts from rest:
smooth, small, mostly single-signed fields, with (near-)zero rows at the lower
slab boundaries, where a stale or misplaced ghost row equals the right one.
Here the slabs start from the states of test_gpu_adversarial.py (random signs,
43 binades with zeros and subnormals, planted NaN / Inf: _util.adversarial_state)
cut out of a single-domain state (cfd_set_state per slab), on layouts chosen
for the branches only slabs take: 4-row slabs, odd and uneven splits, ranks of
one run that differ in the asynchronous u/v exchange, clamped and default halo
depths, both velocity schemes, the fused finish and corrector passes, the
three forms of the tolerance mode, SOR and multigrid, and the renderer.
Everything is bitwise against oracle/cfd_oracle.c on the global grid; all
slabs live in this process over cfdamd.LocalHub.  The oracle-only premises
(non-finite shares, sweep counts, exit sweeps, non-zero boundary rows) are
pinned without a GPU in test_slabs_adversarial_cpu.py.
"""
import numpy as np
import pytest

from _slabs import (FIXED_FORMS, FIXED_SWEEPS, MAX_NONFINITE_SHARE, SOLVER_LAYOUTS, STEP_ROWS,
                    TOL_FORMS, TOL_GRID, TOL_KW, TOL_STEP_SWEEPS, _slab_slices, adv_global_state,
                    assemble, boundary_rows, clean_ranks, fixed_spikes, grid_of, has_clean_rank,
                    layout_id, run_slabs, snapshot, solver_kw, sor_refused, step_cases, step_count,
                    step_kw, tol_spikes)
from _util import (ADV_FIELDS, adversarial_state, assert_bitwise, load_state, nonfinite_share,
                   same_f32, SPIKE_P_TOLS, spike_state)

pytestmark = pytest.mark.gpu
JOIN = 120.0   # seconds a case's ranks get; each takes a few at the most


def _cfd():
    import cfdamd
    return cfdamd


def _setup(g, **kw):
    """(cfdamd.Grid, cfdamd.SimulationParams, OracleModel) of one grid dict and
    parameter set (the oracle's keyword names)."""
    c = _cfd()
    from oracle import OracleModel
    cyl = g.get("cylinder")
    params = c.SimulationParams(
        viscosity=kw.get("viscosity", 1e-6), velocity_scheme=c.VelocityScheme(kw.get("scheme", 0)),
        inlet_profile=c.InletProfile(kw.get("inlet_profile", 0)),
        pressure_solver=c.PressureSolver(kw.get("pressure_solver", 0)),
        jacobi_iters=kw.get("jacobi_iters", 50), corrector_passes=kw.get("corrector_passes", 20),
        tol_enabled=bool(kw.get("tol_enabled", 1)), p_tol=kw.get("p_tol", 1e-4),
        bc_kind=c.BoundaryKind(kw.get("bc_kind", 0)))
    grid = c.Grid(g["nx"], g["ny"], g["lx"], g["ly"], c.Cylinder(*cyl) if cyl else None)
    return grid, params, OracleModel(g["nx"], g["ny"], g["lx"], g["ly"], cylinder=cyl, **kw)


def _residuals_code(m):
    """None when get_residuals() succeeds, else the CfdError's code."""
    try:
        m.get_residuals()
        return None
    except _cfd().CfdError as e:
        return e.code


def _step_and_snapshot(steps):
    """A rank's part of `steps` update() calls: the slab's state after each
    one, then what get_residuals() answers."""
    def fn(m, r):
        snaps = []
        for _ in range(steps):
            m.update()
            snaps.append(snapshot(m))
        return snaps, _residuals_code(m)
    return fn


def _compare_slabs(tag, states, o, nx, nan_equal, fields=ADV_FIELDS):
    """The assembled owned rows (and the v / v* face rows neighbours share)
    and every rank's scalars against the oracle, as test_gpu_adversarial's
    _compare_step."""
    got = assemble(states, nx, nan_equal=nan_equal)
    for f in fields:
        assert_bitwise(f"{tag}: {f}", got[f], o.field(f), nan_equal=nan_equal)
    s = o.scalars()
    for r, (_, _, st, _) in enumerate(states):
        assert st["simulation_step"] == s.step, (tag, r)
        assert st["jacobi_sweeps_total"] == s.jacobi_sweeps_total, \
            (tag, r, st["jacobi_sweeps_total"], s.jacobi_sweeps_total)
        for k, want in (("dt", s.dt), ("simulation_time", s.time), ("last_p_residual", s.p),
                        ("last_u_residual", s.u), ("last_v_residual", s.v)):
            assert same_f32(st[k], want), (tag, r, k, st[k], want)


# ------------------------------------------------------------ 2a: whole steps

@pytest.mark.parametrize("passes", [0, 2])
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("layout,flavour", step_cases(),
                         ids=[f"{layout_id(lay)}-{fl}" for lay, fl in step_cases()])
def test_slab_steps_from_adversarial_state(layout, flavour, scheme, passes):
    """update() on slabs from an adversarial single-domain state: every field
    and scalar bitwise after each step.  corrector_passes 0 takes the fused
    step (k_predict_march in three launches where a slab has 8 rows, the
    fused finish with the solve's residual on the step all-reduce), 2 the
    plain k_corrector4 / k_copy_star_div / k_boundary / k_step_reduce path;
    the second-order scheme reads two ghost rows of u and v across every
    boundary."""
    name, n, depth, want_depth, _ = layout
    g, _ = grid_of(name)
    nx, ny = g["nx"], g["ny"]
    nonfinite = flavour == "nonfinite"
    steps = step_count(flavour)
    grid, params, o = _setup(g, **step_kw(layout, flavour, scheme, passes))
    load_state(adversarial_state(nx, ny, 1, flavour), oracle=o)
    out = run_slabs(n, grid, params, adv_global_state(nx, ny, flavour), depth,
                    _step_and_snapshot(steps), join=JOIN)
    tag = f"{layout_id(layout)} scheme {scheme} passes {passes} {flavour}"
    assert [s[0][0][1] - s[0][0][0] for s in out] == STEP_ROWS[(name, n)], tag
    assert want_depth == min(8 if depth is None else depth, ny // n - 2)
    assert [s[0][0][3] for s in out] == [want_depth] * n, tag
    for step in range(steps):
        o.update()
        _compare_slabs(f"{tag} step {step + 1}", [s[0][step] for s in out], o, nx, nonfinite)
    share = nonfinite_share([o.field(f) for f in ADV_FIELDS])
    codes = [s[1] for s in out]
    if nonfinite:
        # nan_equal must not hide the comparison: most words stay finite
        assert 0.0 < share <= MAX_NONFINITE_SHARE, (tag, share)
        # the flag crosses the ranks: a slab with finite rows only reports it too
        assert codes == [_cfd().CFD_ENONFINITE] * n, (tag, codes)
        # ... and such slabs exist (from the oracle alone; on 248 x 301 every one
        # of the four slabs holds a planted word, see has_clean_rank)
        clean = clean_ranks(o, nx, ny, n)
        assert bool(clean) == has_clean_rank(layout, scheme, passes), (tag, clean)
        for r in clean:
            assert nonfinite_share([out[r][0][-1][2][f] for f in ADV_FIELDS]) == 0.0, (tag, r)
    else:
        assert share == 0.0, (tag, share)
        assert codes == [None] * n, (tag, codes)


# ------------------------------------------------- 2b: the tolerance mode

def _run_tol_form(form, flavour, monkeypatch):
    _, n, depth, spec_env = form
    g, _ = grid_of(TOL_GRID)
    nx, ny = g["nx"], g["ny"]
    if spec_env is None:
        monkeypatch.delenv("CFD_SPEC_SLABS", raising=False)
    else:
        monkeypatch.setenv("CFD_SPEC_SLABS", spec_env)
    grid, params, o = _setup(g, **TOL_KW)
    load_state(adversarial_state(nx, ny, 1, flavour), oracle=o)

    def fn(m, r):
        c0 = m.comm_calls
        m.update()
        return snapshot(m), m.comm_calls - c0, _residuals_code(m)

    out = run_slabs(n, grid, params, adv_global_state(nx, ny, flavour), depth, fn, join=JOIN)
    o.update()
    return out, o, nx


@pytest.mark.parametrize("flavour", ["signs", "range"])
@pytest.mark.parametrize("form", TOL_FORMS, ids=[f[0] for f in TOL_FORMS])
def test_slab_tolerance_step_from_adversarial_state(monkeypatch, form, flavour):
    """One step with the tolerance on (50 sweeps, 2 corrector passes) on
    120 x 37: speculative slab blocks (2 ranks, depth 8), the host-driven
    per-sweep loop by CFD_SPEC_SLABS=0, and host-driven by geometry (3 ranks
    of fewer than 16 rows).  No solve exits early on the oracle, so the step
    runs 150 sweeps; the blocks must make fewer collective calls than the
    host-driven loop does on the same input."""
    out, o, nx = _run_tol_form(form, flavour, monkeypatch)
    tag = f"tolerance {form[0]} {flavour}"
    assert o.scalars().jacobi_sweeps_total == TOL_STEP_SWEEPS, tag
    assert nonfinite_share([o.field(f) for f in ADV_FIELDS]) == 0.0, tag
    assert [s[0][3] for s in out] == [form[2]] * form[1], tag
    _compare_slabs(tag, [s[0] for s in out], o, nx, False)
    assert all(s[0][2]["jacobi_sweeps_total"] == TOL_STEP_SWEEPS for s in out), tag
    assert [s[2] for s in out] == [None] * form[1], tag
    if form[0] == "spec":
        host = next(f for f in TOL_FORMS if f[0] == "host-env")
        ref, _, _ = _run_tol_form(host, flavour, monkeypatch)
        calls, host_calls = [s[1] for s in out], [s[1] for s in ref]
        assert len(set(calls)) == 1 and len(set(host_calls)) == 1, (calls, host_calls)
        assert calls[0] < host_calls[0], (tag, calls, host_calls)


# ------------------------------------- 2c: the Jacobi residual across ranks

def _spike_solves(n, depth, g, kw, spikes, nan_in):
    """pressure_solve() on every rank from each planted spike, against
    o.jacobi(): {spike: (oracle residual, oracle sweeps)}."""
    nx, ny = g["nx"], g["ny"]
    grid, params, o = _setup(g, **kw)
    inputs = [spike_state(nx, ny, 2, col, row, nan_in) for col, row in spikes]

    def fn(m, r):
        res = []
        for pp, rhs in inputs:
            m.set_state(**_slab_slices(dict(p_prime=pp, rhs=rhs, jacobi_sweeps_total=0),
                                       nx, m.j0, m.j1))
            got = np.float32(m.pressure_solve())
            st = m.get_state()
            res.append((got, st["jacobi_sweeps_total"], st["p_prime"]))
        return m.j0, m.j1, m.halo_depth, res

    out = run_slabs(n, grid, params, None, depth, fn, join=JOIN)
    assert [s[2] for s in out] == [depth] * n, [s[2] for s in out]
    want = {}
    for k, (col, row) in enumerate(spikes):
        tag = f"{kw} n {n} depth {depth} spike ({col},{row}) nan {nan_in}"
        pp, rhs = inputs[k]
        o.field("p_prime")[:] = pp
        o.field("rhs")[:] = rhs
        s = o.scalars()
        s.jacobi_sweeps_total = 0
        o.set_scalars(s)
        res = np.float32(o.jacobi())
        sweeps = int(o.scalars().jacobi_sweeps_total)
        assert np.isfinite(res), tag
        for r in range(n):
            got, got_sweeps, _ = out[r][3][k]
            assert same_f32(got, res), (tag, r, got, res)
            assert got_sweeps == sweeps, (tag, r, got_sweeps, sweeps)
        assert_bitwise(tag, np.concatenate([out[r][3][k][2] for r in range(n)]),
                       o.field("p_prime"), nan_equal=nan_in is not None)
        want[(col, row)] = (res, sweeps)
    return want


@pytest.mark.parametrize("nan_in", [None, "p_prime", "rhs"])
@pytest.mark.parametrize("iters", FIXED_SWEEPS)
@pytest.mark.parametrize("form", FIXED_FORMS, ids=[f[0] for f in FIXED_FORMS])
def test_slab_jacobi_residual_fixed_count(form, iters, nan_in):
    """A collective pressure_solve() of 1, 8, 9 and 17 sweeps on 120 x 37 from
    noise with p' = 1 planted at every spike column, on the single-domain
    rows and on both rows of every slab boundary: the residual (k_fold_slots
    and the max all-reduce across ranks, its nx-8 / nx-7 column mask, its
    NaN-ignoring maximum) has the oracle's bits on every rank, with the sweep
    count and p'."""
    _, n, depth = form
    g, _ = grid_of(TOL_GRID)
    nx, ny = g["nx"], g["ny"]
    kw = dict(bc_kind=1, jacobi_iters=iters, tol_enabled=0)
    res = _spike_solves(n, depth, g, kw, fixed_spikes(nx, ny, n), nan_in)
    if nan_in is None:
        for row in boundary_rows(ny, n):
            assert res[(nx - 8, row)] != res[(nx - 7, row)], (form, iters, row, res)


@pytest.mark.parametrize("nan_in", [None, "p_prime", "rhs"])
@pytest.mark.parametrize("form", TOL_FORMS, ids=[f[0] for f in TOL_FORMS])
def test_slab_jacobi_residual_tolerance(monkeypatch, form, nan_in):
    """The same with the tolerance on, over the tolerance list that puts the
    early exit on sweeps 1 .. 10 and at the limit, in the three forms of the
    slabs' tolerance mode, with the spike at the residual's last included and
    first excluded column and both sides of the 112-column seam, on the two
    rows of the first slab boundary and the last swept row."""
    _, n, depth, spec_env = form
    if spec_env is None:
        monkeypatch.delenv("CFD_SPEC_SLABS", raising=False)
    else:
        monkeypatch.setenv("CFD_SPEC_SLABS", spec_env)
    g, _ = grid_of(TOL_GRID)
    nx, ny = g["nx"], g["ny"]
    spikes = tol_spikes(nx, ny, n)
    exits = set()
    for p_tol in SPIKE_P_TOLS:
        kw = dict(bc_kind=1, jacobi_iters=50, tol_enabled=1, p_tol=p_tol)
        res = _spike_solves(n, depth, g, kw, spikes, nan_in)
        exits.update(sweeps for _, sweeps in res.values())
        if nan_in is None:
            for row in sorted({r for _, r in spikes}):
                assert res[(nx - 8, row)] != res[(nx - 7, row)], (form, p_tol, row, res)
    if nan_in is None:
        residues = {e % 8 for e in exits}
        assert len(residues) >= 3 and residues - {0}, sorted(exits)
        assert 50 in exits, sorted(exits)


# ------------------------------------------ 2d: SOR and multigrid on slabs

@pytest.mark.parametrize("passes", [0, 2])
@pytest.mark.parametrize("flavour", ["signs", "range"])
@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("layout", SOLVER_LAYOUTS, ids=[f"{s[0]}-n{s[1]}" for s in SOLVER_LAYOUTS])
def test_slab_sor_and_multigrid_from_adversarial_state(monkeypatch, layout, solver, flavour, passes):
    """Red-black SOR and multigrid steps on slabs from an adversarial state,
    every field (rhs included) after each of two steps: 120 x 37 on 19 / 18
    rows (the multigrid levels gathered) and 128 x 64 on four 16-row slabs
    whose boundaries divide by 2, 4 and 8, with the fine levels partitioned.
    SOR on slabs needs 16 interior rows a slab (validate_sharded); the first
    and last of four 16-row slabs have 15, so there the library's answer is
    CFD_EINVAL at creation, and that is what is checked."""
    name, n, depth, part = layout
    if part is None:
        monkeypatch.delenv("CFD_MG_PARTITION", raising=False)
    else:
        monkeypatch.setenv("CFD_MG_PARTITION", part)
    g, _ = grid_of(name)
    nx, ny = g["nx"], g["ny"]
    grid, params, o = _setup(g, **solver_kw(solver, passes))
    if solver == 1 and sor_refused(ny, n):
        c = _cfd()
        monkeypatch.setenv("CFD_HALO_DEPTH", str(depth))
        hub = c.LocalHub(n)
        try:
            with pytest.raises(c.CfdError, match="16 interior rows per slab") as ei:
                c.Model(grid, params, device=0, n_ranks=n, rank=0, local_hub=hub)
            assert ei.value.code == -1, ei.value   # CFD_EINVAL
        finally:
            hub.close()
        return
    load_state(adversarial_state(nx, ny, 1, flavour), oracle=o)
    out = run_slabs(n, grid, params, adv_global_state(nx, ny, flavour), depth,
                    _step_and_snapshot(2), join=JOIN)
    tag = f"{name} n {n} solver {solver} passes {passes} {flavour}"
    assert [s[0][0][3] for s in out] == [depth] * n, tag
    for step in range(2):
        o.update()
        _compare_slabs(f"{tag} step {step + 1}", [s[0][step] for s in out], o, nx, False)
    assert nonfinite_share([o.field(f) for f in ADV_FIELDS]) == 0.0, tag
    assert [s[1] for s in out] == [None] * n, tag


# ------------------------------------------------------ 2e: render on slabs

def test_slab_render_from_adversarial_state():
    """cfd_render / cfd_derive_field on three slabs of the 128 x 60 cylinder
    channel: from the loaded `nonfinite` state with no step taken (the u / v
    ghost rows the vorticity reads across a boundary come from set_state's
    exchange alone), then after one step from `signs`.  The stacked images and
    fields of all three modes equal oracle/render.py on the assembled
    snapshot, and every rank reports the global minimum and maximum."""
    from render import derive, render
    g, _ = grid_of("128x60")
    nx, ny, n = g["nx"], g["ny"], 3
    grid, params, _ = _setup(g, corrector_passes=0, tol_enabled=0, jacobi_iters=9)
    finite = adv_global_state(nx, ny, "signs")

    def views(m):
        snap = m.get_snapshot()
        return (snap, [m.render(mode) for mode in (0, 1, 2)],
                [m.derive_field(mode) for mode in (0, 1, 2)])

    def fn(m, r):
        first = views(m)
        m.set_state(**_slab_slices(finite, nx, m.j0, m.j1))
        m.update()
        return m.j0, m.j1, first, views(m)

    out = run_slabs(n, grid, params, adv_global_state(nx, ny, "nonfinite"), 4, fn, join=JOIN)
    for k, stage in ((2, "nonfinite, no step"), (3, "signs, one step")):
        u = np.concatenate([s[k][0].u for s in out])
        p = np.concatenate([s[k][0].p for s in out])
        v = np.concatenate([s[k][0].v.reshape(-1, nx)[:(None if r == n - 1 else -1)].ravel()
                            for r, s in enumerate(out)])
        assert u.size == (nx + 1) * ny and v.size == nx * (ny + 1) and p.size == nx * ny
        for mode in (0, 1, 2):
            tag = f"render {stage} mode {mode}"
            want_img, wmm = render(mode, u, v, p, nx, ny, grid.dx, grid.dy, g["cylinder"])
            img = np.concatenate([s[k][1][mode][0] for s in out])
            bad = np.argwhere((img != want_img).any(-1))
            assert bad.size == 0, f"{tag}: {len(bad)} pixels differ, first {bad[0]}"
            fld = np.concatenate([s[k][2][mode][0] for s in out])
            assert_bitwise(tag, fld, derive(mode, u, v, p, nx, ny, grid.dx, grid.dy),
                           nan_equal=True)
            for r, s in enumerate(out):
                for mm in (s[k][1][mode][1], s[k][2][mode][1]):
                    assert np.float32(mm[0]) == wmm[0] and np.float32(mm[1]) == wmm[1], \
                        (tag, r, mm, wmm)
