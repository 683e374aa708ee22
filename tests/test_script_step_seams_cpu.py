"""CPU: the premises of the script substep's and update's seam tests
(test_gpu_script_step_seams.py, test_gpu_script_update_seams.py), checked with
the restatements alone (tests/_script_step_ref.py, pinned to node by
test_script_step_cpu.py; tests/_script_update_ref.py, by
test_script_update_cpu.py): the wave-column and segment geometry the table
claims, which widths a model can be built for, that the cases of each scheme
take every branch the restatement counts, the clipped discs' faces, that the
extreme flavours are extreme where they say and hide little, and that each
planted word of the update cases alone holds the maximum."""
import numpy as np
import pytest

import _script_step_cases as t
import _script_step_ref as ref
from _util import assert_bitwise


# ------------------------------------------------------------ predictor shapes
def test_geometry_is_what_the_table_claims():
    """nch, nwc, the lane of the face-nx chunk and the segment starts, from the
    formulas of cfd_script_step.hip's header."""
    G = t.geometry
    # nx: (nch, wave columns, wave column and lane of the face-nx chunk)
    want = {8: (2, 1, 0, 3), 12: (3, 1, 0, 4), 16: (4, 1, 0, 5), 24: (6, 1, 0, 7),
            240: (60, 1, 0, 61), 244: (61, 1, 0, 62), 248: (62, 2, 1, 1), 252: (63, 2, 1, 2),
            256: (64, 2, 1, 3), 488: (122, 2, 1, 61), 492: (123, 2, 1, 62), 496: (124, 3, 2, 1)}
    assert set(want) == set(t.WIDTHS) | set(t.DEVICE_WIDTHS)
    for nx, w in want.items():
        g = G(nx, 9)
        assert (g.nch, g.nwc, g.face_wc, g.face_lane) == w, nx
        # the lanes of wave column wc hold chunks 62 wc - 1 + lane; lanes 1 .. 62 store
        assert 62 * g.face_wc - 1 + g.face_lane == g.nch and 1 <= g.face_lane <= 62
        # a wave column exactly full: the face-nx chunk on its last storing lane
        assert (g.face_lane == 62) == (nx in (244, 492))
        # the face-nx chunk alone in the last wave column: lane 63 of the one
        # before holds it too and supplies `east`
        assert (g.face_lane == 1 and g.face_wc > 0) == (nx in (248, 496))
    # ny: (R, segment starts, blocks per wave column)
    rows = {4: (4, (0,), 1), 5: (4, (0, 1), 1), 7: (4, (0, 3), 1), 8: (8, (0,), 1),
            9: (8, (0, 1), 1), 16: (8, (0, 8), 1), 17: (8, (0, 8, 9), 1),
            33: (8, (0, 8, 16, 24, 25), 2)}
    assert set(rows) == set(t.HEIGHTS)
    for ny, (R, starts, blocks) in rows.items():
        g = G(16, ny)
        assert (g.R, g.starts, g.nblocks) == (R, starts, blocks), ny
        assert g.starts[-1] + g.R == ny and all(s + g.R <= ny for s in g.starts)


def test_table_covers_the_shapes():
    shapes = {(c.nx, c.ny) for c in t.CASES}
    for nx in t.WIDTHS + t.DEVICE_WIDTHS:
        assert {(nx, 9), (nx, 33)} <= shapes
    for ny in t.HEIGHTS:
        assert {(8, ny), (16, ny), (248, ny)} <= shapes
    assert {(8, 4), (496, 33)} <= shapes
    for nx, ny in shapes:      # both division paths on every shape, every scheme on each
        fast = {t.is_fast(t.grid_of(c)) for c in t.CASES if (c.nx, c.ny) == (nx, ny)}
        assert fast == {True, False}, (nx, ny)
    for c in t.CASES:
        assert t.is_fast(t.grid_of(c)) == (c.path == "pow2"), c.name
    # what a model can run: every height, and every seam a model's widths reach
    dev = {(c.nx, c.ny) for c in t.DEVICE_CASES}
    assert {ny for nx, ny in dev if nx == 16} == set(t.HEIGHTS) == {ny for nx, ny in dev if nx == 248}
    lanes = {(t.geometry(nx, ny).face_wc, t.geometry(nx, ny).face_lane) for nx, ny in dev}
    assert {(0, 5), (0, 61), (1, 1), (1, 3), (1, 61), (2, 1)} <= lanes
    assert t.BY_NAME[t.SUBSTEP_CASE].device and t.BY_NAME[t.SUBSTEP_CASE].cyl
    assert max(c.nx * c.ny for c in t.CASES) <= 496 * 33


def test_widths_off_the_8_grid_are_refused_by_the_constructor():
    """Why 8, 12, 244, 252 and 492 stay with the restatement although
    script_step_ok would take them: CFD_EINVAL before any device call."""
    import cfdamd as c
    refused = sorted({(k.nx, k.ny) for k in t.CASES if not k.device} |
                     {s for s in t.EXTREME_SHAPES if not t.on_device(*s)} |
                     {(d.nx, d.ny) for d in t.DISCS if not d.device} | {(8, 120)})
    assert {nx for nx, _ in refused} == {8, 12, 244, 252, 492}
    for nx, ny in refused:
        with pytest.raises(c.CfdError) as e:
            c.Model(c.Grid(nx, ny, 30.0, 10.0),
                    c.SimulationParams(pressure_solver=c.PressureSolver.JacobiScript))
        assert e.value.code == -1 and "multiple of 8" in str(e.value), (nx, ny)


def test_random_state_is_the_substep_tests_recipe():
    from test_gpu_script_step import _random_state
    g = t.grid_of(t.BY_NAME["248x9_div"])
    for a, b in zip(t.random_state(g, 11, t.DT_SUB), _random_state(g, 11, t.DT_SUB)):
        assert_bitwise("random_state", a, b)
    u, v, _ = t.random_state(g, 11, t.DT_SUB)
    for z in (0.0, -0.0):
        assert np.any((u == 0) & (np.signbit(u) == np.signbit(np.float32(z))))


@pytest.mark.parametrize("scheme", t.SCHEMES)
def test_cases_of_a_scheme_take_every_branch(scheme):
    """Over the cases of a scheme every counter of the restatement is positive
    (single small cases miss some: the union is the condition) -- over all
    cases, and over those a model can run."""
    names = ref.counter_names(scheme)
    for cases in (t.CASES, t.DEVICE_CASES):
        tot = dict.fromkeys(names, 0)
        for c in cases:
            cnt = t.predicted(c, scheme)[-1]
            for k in names:
                tot[k] += cnt.get(k, 0)
            if c.cyl:
                assert cnt["u_obstacle"] > 0 and cnt["v_obstacle"] > 0, c.name
            else:
                assert cnt.get("u_obstacle", 0) == 0 and cnt.get("v_obstacle", 0) == 0, c.name
        assert [k for k in names if tot[k] == 0] == []


def test_cylinders_are_interior_and_where_the_grid_holds_one():
    for c in t.CASES:
        assert (c.cyl is not None) == (c.nx >= 16 and c.ny >= 9), c.name
        if c.cyl:
            g = t.grid_of(c)
            fc = t.face_counts(g)
            assert fc[:6] == (0,) * 6 and fc[6] > 0 and fc[7] > 0, (c.name, fc)
            ou, ov = ref.obstacle_faces(g)
            assert np.array_equal(ref.intervals_to_mask(ref.obstacle_intervals(ou), g.nx + 1), ou)
            if c.nx >= 488:     # across the seam between the first two wave columns
                assert ou[:, 247].any() and ou[:, 248].any() and ov[:, 247].any() and ov[:, 248].any()


# ---------------------------------------------------------------- clipped discs
@pytest.mark.parametrize("name", [d.name for d in t.DISCS])
def test_disc_faces_are_one_interval_per_row_and_counted(name):
    d = t.DISC_BY_NAME[name]
    g = t.disc_grid(d)
    ou, ov = ref.obstacle_faces(g)
    assert np.array_equal(ref.intervals_to_mask(ref.obstacle_intervals(ou), g.nx + 1), ou)
    assert np.array_equal(ref.intervals_to_mask(ref.obstacle_intervals(ov), g.nx), ov)
    assert t.face_counts(g) == d.counts, name


def test_discs_reach_the_clauses_they_are_for():
    c = {d.name[len("248x16_"):]: d.counts for d in t.DISCS if d.nx == 248}
    assert c["inlet"][0] == 10 and c["outlet"][1] == 10          # u columns 0 and nx
    assert c["bottom_wall"][2] > 0 and c["bottom_wall"][4] > 0   # u row 0, v row 0
    assert c["top_wall"][3] > 0 and c["top_wall"][5] > 0         # u row ny-1, v row ny
    assert all(c["taller_than_channel"][2:6])
    assert c["corner_inlet_bottom"][0] and c["corner_inlet_bottom"][2] and c["corner_inlet_bottom"][4]
    assert c["corner_outlet_top"][1] and c["corner_outlet_top"][3] and c["corner_outlet_top"][5]
    assert c["one_u_face_no_v_face"][6:] == (1, 0)
    assert c["smaller_than_any_face"][6:] == (0, 0) == c["outside_the_domain"][6:]
    g = t.disc_grid(t.DISC_BY_NAME["248x16_inlet"])
    assert t.is_fast(g) and not t.is_fast(t.disc_grid(t.DISC_BY_NAME["16x5_inlet"]))
    # the outlet clause decides something: the corrected u(nx-1) it would copy is not 0
    decided = 0
    for d in t.DEVICE_DISCS:
        if d.counts[1] > (d.counts[3] > 0):      # an outlet face off the wall rows
            g = t.disc_grid(d)
            ou, _ = ref.obstacle_faces(g)
            us, vs, pp, p, u, v, pn = t.disc_corrected(d, ref.UNIFORM)
            rows = np.flatnonzero(ou[:, g.nx])
            free = ref.correct(ref.Grid(d.nx, d.ny, d.lx, d.ly, t.NU, None), us, vs, pp, p, t.DT_SUB,
                               t.INLET, ref.UNIFORM)[0]
            inner = [j for j in rows if 0 < j < g.ny - 1]
            assert inner and np.all(free[inner, g.nx] != 0) and not u[rows, g.nx].any(), d.name
            decided += 1
    assert decided >= 3
    # some row's interval is [nx, nx + 1): `nx >= oul` at equality
    iv = ref.obstacle_intervals(ref.obstacle_faces(t.disc_grid(t.DISC_BY_NAME["248x16_outlet_one_face_rows"]))[0])
    assert np.any((iv[:, 0] == 248) & (iv[:, 1] == 249))


# --------------------------------------------------------------- extreme values
EXTREME = [(nx, ny, fl, s) for nx, ny in t.EXTREME_SHAPES for fl in t.FLAVOURS for s in t.SCHEMES]


def _planted(nx, ny, rows, cols):
    return t.nonfinite_positions(nx, ny, rows, cols, np.random.default_rng(0))


@pytest.mark.parametrize("nx,ny,flavour,scheme", EXTREME)
def test_extreme_predictor_cases_are_what_they_say(nx, ny, flavour, scheme):
    g, dt_sub, u, v, p, us, vs, rhs = t.extreme_predicted(nx, ny, flavour, scheme)
    assert t.is_fast(g) == (t.extreme_path(nx, ny, flavour, scheme) == "pow2")
    if flavour == "huge":
        assert np.isfinite(u).all() and np.isfinite(v).all()
        for a in (us, vs, rhs):
            assert np.isposinf(a).any() and np.isneginf(a).any()
        # u*, v* come from finite doubles: no NaN; rhs subtracts stored infinities
        assert not np.isnan(us).any() and not np.isnan(vs).any()
    elif flavour == "tiny":
        assert t.subnormal_share(u) > 0.3 and t.subnormal_share(v) > 0.3
        for a in (us, vs, rhs):
            assert np.isfinite(a).all() and t.subnormal_share(a) >= t.SUBNORMAL_SHARE
    else:
        # all three words in each field; a grid under 400 cells holds them between u and v
        for a in (u, v) if nx * ny >= 400 else (np.concatenate((u.ravel(), v.ravel())),):
            assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
        for a in (us, vs, rhs):
            assert 0 < t.nonfinite_share(a) <= t.NONFINITE_CAP, t.nonfinite_share(a)
        if (nx, ny) == (248, 17):
            pu, pv = _planted(nx, ny, ny, nx + 1), _planted(nx, ny, ny + 1, nx)
            geo = t.geometry(nx, ny)
            assert geo.starts == (0, 8, 9)
            for pos, cols in ((pu, nx + 1), (pv, nx)):
                assert {i for _, i in pos} >= {0, cols - 1} | {i for i in (246, 247, 248, 249) if i < cols}
                assert {j for j, _ in pos} >= {7, 8, 9}
            assert len(pu) >= ny * (nx + 1) // 400 and len(pv) >= (ny + 1) * nx // 400


def test_extreme_flavours_use_both_division_paths():
    for nx, ny in t.EXTREME_SHAPES:
        for fl in t.FLAVOURS:
            assert {t.extreme_path(nx, ny, fl, s) for s in t.SCHEMES} == set(t.PATHS)
        for s in t.SCHEMES:
            assert {t.extreme_path(nx, ny, fl, s) for fl in t.FLAVOURS} == set(t.PATHS)
    assert t.EXTREME_DEVICE_SHAPES == [(248, 17), (16, 7)]


@pytest.mark.parametrize("path", t.PATHS)
@pytest.mark.parametrize("flavour", t.FLAVOURS)
def test_extreme_corrector_cases_are_what_they_say(flavour, path):
    g, dt_sub, us, vs, pp, p, u, v, pn = t.extreme_corrected(flavour, path)
    assert t.is_fast(g) == (path == "pow2")
    if flavour == "huge":
        for a in (us, vs, pp, p):
            assert np.isfinite(a).all() and np.abs(a).max() > 1e37
        for a in (u, v, pn):
            assert np.isinf(a).any() and not np.isnan(a).any()
        assert np.isposinf(u).any() and np.isneginf(u).any()
    elif flavour == "tiny":
        for a in (u, v, pn):
            assert np.isfinite(a).all() and t.subnormal_share(a) >= t.SUBNORMAL_SHARE
    else:
        for a in (us, vs, pp):
            assert np.isnan(a).any() and np.isposinf(a).any() and np.isneginf(a).any()
        for a in (u, v, pn):
            assert 0 < t.nonfinite_share(a) <= t.NONFINITE_CAP


@pytest.mark.parametrize("scheme", t.SCHEMES)
def test_the_four_corner_words_reach_only_themselves_and_corner_cells_of_rhs(scheme):
    """No stencil of the script reads u[0, 0], u[ny-1, nx], v[0, 0] or
    v[ny, nx-1]; the divergence does, through the u*, v* they are copied to.  A
    NaN there is therefore not inert, which is why the update's planted words
    are finite, and the script's Jacobi reads no boundary cell of rhs, which is
    why a finite plant there moves nothing but its own residual."""
    c = t.BY_NAME["16x9_div"]
    g = t.grid_of(c)
    u, v, p, us, vs, rhs, _ = t.predicted(c, scheme)
    u2, v2 = u.copy(), v.copy()
    u2[0, 0] += 3
    u2[g.ny - 1, g.nx] -= 3
    v2[0, 0] += 5
    v2[g.ny, g.nx - 1] = np.nan
    us2, vs2, rhs2 = ref.predict(g, u2, v2, c.dt_sub, scheme)
    du = us2.view(np.uint32) != us.view(np.uint32)
    dv = vs2.view(np.uint32) != vs.view(np.uint32)
    dr = rhs2.view(np.uint32) != rhs.view(np.uint32)
    assert sorted(zip(*np.nonzero(du))) == [(0, 0), (g.ny - 1, g.nx)]
    assert sorted(zip(*np.nonzero(dv))) == [(0, 0), (g.ny, g.nx - 1)]
    assert sorted(zip(*np.nonzero(dr))) == [(0, 0), (g.ny - 1, g.nx - 1)]
    assert np.isnan(rhs2[g.ny - 1, g.nx - 1])


# ------------------------------------------------------ the update's two passes
def test_update_grids_hit_the_block_structure():
    sizes = {k: t.words(*g) for k, g in t.UPDATE_GRIDS.items()}
    nu, nv = sizes["one_stride"]
    assert nu + nv < t.THREAD_STRIDE
    nu, nv = sizes["block_multiple"]
    assert (nu + nv) % t.BLOCK_WORDS == 0 and nu % t.BLOCK_WORDS and nu % 64    # mid-block, mid-wave
    nu, nv = sizes["one_past_a_block"]
    assert (nu + nv) % t.BLOCK_WORDS == 1
    nu, nv = sizes["boundary_on_a_stride"]
    assert nu % t.THREAD_STRIDE == 0
    for k, (nx, ny) in t.UPDATE_GRIDS.items():
        assert t.on_device(nx, ny) and nx <= 64, k
        assert sum(t.words(nx, ny)) == 2 * nx * ny + nx + ny
    # the searches return the smallest: no admissible grid with fewer words has the property
    for k, pred in (("block_multiple", lambda n: n % 1024 == 0), ("one_past_a_block", lambda n: n % 1024 == 1)):
        best = sum(sizes[k])
        for nx in range(16, 65, 8):
            for ny in range(4, best // (2 * nx) + 1):
                n = sum(t.words(nx, ny))
                assert not (pred(n) and n < best), (k, nx, ny)
    assert sum(t.words(8, 4)) == 76 and sum(t.words(8, 120)) == 2048    # the grids a model refuses


@pytest.mark.parametrize("gname,kind", t.UPDATE_CASES)
def test_update_case_holds_its_maximum_where_planted(gname, kind):
    g, st, target, new, rep = t.updated(gname, kind)
    assert "extrapolated" in rep["branches"] and rep["substeps_run"] == t.UPDATE_SUBSTEPS
    for f in ("u", "v", "p"):
        assert np.isfinite(new[f]).all()
    with np.errstate(invalid="ignore"):
        uo = (2 * st["u"].astype(np.float64) - st["u_prev"]).astype(np.float32).astype(np.float64)
        vo = (2 * st["v"].astype(np.float64) - st["v_prev"]).astype(np.float32).astype(np.float64)
        du = np.abs(new["u"].astype(np.float64) - uo).ravel()
        dv = np.abs(new["v"].astype(np.float64) - vo).ravel()
    pw = t.plant_words(g.nx, g.ny)
    nu, nv = t.words(g.nx, g.ny)
    assert [pw[k][2] for k in t.PLANTS] == [0, nu - 1, nu, nu + nv - 1]
    if kind in t.PLANTS or kind == "zero_but_last_word":
        f, k, _ = pw["last_v" if kind == "zero_but_last_word" else kind]
        d, res = (du, rep["residual_u"]) if f == "u_prev" else (dv, rep["residual_v"])
        assert list(np.flatnonzero(d == res)) == [k] and res > 2.9
        assert np.sort(d)[-2] < 0.5 * res      # and nothing comes near it
    if kind in t.PLANTS or kind == "nan_first_word":
        assert rep["max_vel"] > 0
        assert ("dt_is_cfl" in rep["branches"]) == (gname != "one_stride")
    if kind == "nan_first_word":
        assert np.isnan(du[0]) and np.count_nonzero(np.isnan(du)) == 1 and not np.isnan(dv).any()
        assert np.isfinite([rep["residual_u"], rep["residual_v"], rep["residual_p"], rep["dt_next"]]).all()
        assert rep["residual_u"] > 0
    if kind in ("all_zero", "zero_but_last_word"):
        assert rep["max_vel"] == 0 and "maxvel_zero" in rep["branches"]
        assert rep["dt_next"] == t.UPDATE_DT_USER and not new["u"].any() and not new["v"].any()
        assert rep["residual_u"] == 0 and rep["residual_p"] == 0
        assert (rep["residual_v"] == 0) == (kind == "all_zero")
    assert rep["script_decisions"] == (rep["substep_count_next"], rep["dt_next"])
