"""GPU: red-black SOR and the three-V-cycle multigrid (cfd_params.pressure_solver
1 and 2) where their kernels' geometry has seams: the 54- / 52-column wave
windows and 14-row tiles of k_mg_smooth5w, the 113- / 111-row strips of
k_mg_smooth5m, the odd coarse sizes of the (n + 1) / 2 hierarchy, hierarchies
of one and two levels inside k_mg_tail, the 124-column wave columns and the
overlapping 16- / 32-row segments of k_sor_march -- fed rhs of both signs and of
43 binades with zeros and subnormals, stale NaN in the ping-pong buffers, NaN
on the boundary rhs cells nothing may read, and one interior NaN the final
residual must ignore.

Everything is bitwise against oracle.mg_solve / oracle.sor_solve / OracleModel
(oracle/cfd_oracle_solvers.c), which tests/test_oracle_solvers.py pins against
the reference script run by node and against numpy at these shapes, together
with the premises of the NaN cases.  test_shape_table_hits_seams (no device)
derives from the kernels' constants that the shape lists reach every seam.

What no comparison here can see: the fused residual's store of row ny - 1.
That row is boundary, its residual is 0, and the level's r buffer is zeroed
when the hierarchy is built and written by nothing else, so a single-domain
launch that skipped the row would leave the same bits.  The rows the
residual can lose visibly -- the last row of a 14-row tile or of a 111-row
strip inside the grid -- are covered by the shapes of 14k + 1, 111 and 111 + 1
rows.
"""
import functools

import numpy as np
import pytest

from _util import (adversarial_state, assert_bitwise, load_state, nonfinite_share, same_f32,
                   SHALLOW_LX, SHALLOW_LY, SHALLOW_NAN_GRIDS, shallow_nan_rhs, solver_rhs, spacing,
                   SPACINGS, with_boundary_nan, ADV_FIELDS)

gpu = pytest.mark.gpu

# ---- geometry, csrc/cfd_solvers.hip
MG_SWEEPS = 5                                 # :374  kSmT
MG_WIN_COLS = 64 - 2 * MG_SWEEPS              # :464  kOW of k_mg_smooth5w / :552 of k_mg_smooth5m: 54
MG_WIN_COLS_RES = 64 - 2 * (MG_SWEEPS + 1)    # :462  kHL = kSmT + 1 with the fused residual: 52
MG_TILE_ROWS = 14                             # :382  kSmTHSmall (levels below 2^23 cells, :869)
MG_MARCH_ROWS = 128 - 15                      # :544  mg_march_rows<false>() with kMgSlots 128 (:538): 113
MG_MARCH_ROWS_RES = 128 - 17                  # :544  mg_march_rows<true>(): 111
SOR_PAIRS = 62                                # :244  c = wc * 62 - 1 + lane (launcher :796): 124 columns
SOR_SEG_ROWS, SOR_SEG_ROWS_BIG = 16, 32       # :767  kSorRows, kSorRowsBig (chosen at :797)
MG_TAIL_CELLS = 4096                          # :15-16 "default 64 x 64 cells" (mg_build, cfd_model_solvers.hip)

MAX_NONFINITE_SHARE = 0.20                    # as tests/test_gpu_adversarial.py

MG_SHAPES = [
    (16, 4),       # one level: the lc == 0 copy branch of k_mg_tail
    (16, 5),       # two levels: 16x5 -> 8x3
    (2048, 4),     # one level of more cells than the tail threshold: the tail still runs it alone
    (56, 15),      # 54 + 2 columns, 14 + 1 rows
    (104, 29),     # 2 x 52 exactly (residual), three 54-wide windows otherwise; 2 x 14 + 1 rows
    (112, 28),     # exactly 2 x 14 rows
    (216, 57),     # 4 x 54; levels 108 = 2 x 54, 54 = 52 + 2, 27; rows 57 -> 29 -> 15 -> 8 -> 4
    (208, 113),    # 4 x 52; one plain march strip of 113 rows, two residual strips
    (160, 227),    # 2 x 113 + 1 rows; four residual windows, the last of 4 columns
    (160, 222),    # 2 x 111 rows
    # added for the table: a width is a multiple of 8, so a level of 54k + 1 or
    # 52k + 1 columns is odd and first appears three halvings down
    (440, 33),     # 440 -> 220 -> 110 -> 55 = 54 + 1 columns (x 5 rows)
    (424, 33),     # 424 -> 212 -> 106 -> 53 = 52 + 1 columns
    (56, 223),     # 2 x 111 + 1 rows, then 112 = 111 + 1
]
MG_TB0_SHAPES = [(56, 15), (216, 57)]         # the single-sweep kernels (CFD_MG_TB=0)
MG_SMOOTH_MODES = (None, "1", "2", "3")       # CFD_MG_SMOOTH: unset, LDS blocks, march, windows
MG_TAILS = ("default", "0")                   # CFD_MG_TAIL: 0 = every level but the coarsest grid-wide

SOR_SHAPES = [(248, 17), (248, 18), (248, 33), (248, 34), (248, 35), (256, 35), (120, 33), (16, 18),
              # added for the table: 62 + 2 pairs (the smallest last wave column
              # a width of 8k has) and 16 + 1 rows
              (128, 19)]
SOR_ITERS = 7
SOR_TOL_NY = (17, 18, 19, 33, 34, 35)         # the row categories, tolerance on, at nx = 248


# ------------------------------------------------------------- the shape table

def mg_levels(nx, ny):
    """mgVcycle's recursion (index.html:1444-1451; mg_build, cfd_model_solvers.hip)."""
    dims = [(nx, ny)]
    while not (dims[-1][0] <= 4 or dims[-1][1] <= 4):
        dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
    return dims


def mg_grid_wide(nx, ny, tail):
    """Levels above k_mg_tail: those before the first one of at most
    CFD_MG_TAIL cells, the coarsest always inside (mg_build, cfd_model_solvers.hip)."""
    dims = mg_levels(nx, ny)
    thr = MG_TAIL_CELLS if tail == "default" else int(tail)
    first = next((l for l, (a, b) in enumerate(dims) if a * b <= thr), len(dims) - 1)
    return dims[:first]


def test_shape_table_hits_seams():
    """From the constants above: some level that runs grid-wide (under the
    default tail or CFD_MG_TAIL=0, both in the matrix) is an exact multiple of,
    and one over, each window width, tile height and strip height; some width
    leaves a last window of at most 2 columns; the SOR shapes do the same for
    wave columns and segments."""
    levels = {d for nx, ny in MG_SHAPES for tail in MG_TAILS for d in mg_grid_wide(nx, ny, tail)}
    assert all(a * b < (1 << 22) for a, b in levels)   # below the march / 30-row-tile thresholds
    table = {}
    for name, unit, axis in (("win54", MG_WIN_COLS, 0), ("win52", MG_WIN_COLS_RES, 0),
                             ("tile14", MG_TILE_ROWS, 1), ("march113", MG_MARCH_ROWS, 1),
                             ("march111", MG_MARCH_ROWS_RES, 1)):
        sizes = sorted({d[axis] for d in levels})
        table[name] = dict(exact=[n for n in sizes if n % unit == 0],
                           one_over=[n for n in sizes if n > unit and n % unit == 1])
        if axis == 0:
            table[name]["last_le_2"] = [n for n in sizes if n > unit and 1 <= n % unit <= 2]
            # more than one window per row, so the window index splits into column and row
            assert any(n > unit for n in table[name]["exact"]), (name, sizes)
    # hierarchies of one and two levels, and a one-level grid above the tail threshold
    depth = {len(mg_levels(nx, ny)) for nx, ny in MG_SHAPES}
    assert {1, 2} <= depth and max(depth) >= 5, depth
    assert any(len(mg_levels(nx, ny)) == 1 and nx * ny > MG_TAIL_CELLS for nx, ny in MG_SHAPES)
    # odd sizes on the finest level and on coarse levels in both directions
    assert any(ny % 2 for _, ny in MG_SHAPES)
    coarse = {d for nx, ny in MG_SHAPES for d in mg_levels(nx, ny)[1:]}
    assert any(a % 2 for a, _ in coarse) and any(b % 2 for _, b in coarse)
    # the single-sweep kernels run grid-wide too
    assert all(mg_grid_wide(nx, ny, "0") for nx, ny in MG_TB0_SHAPES)

    # SOR: the fused form needs ny - 2 >= 16 (sor_fused_ok, :791), 32-row segments from 32 rows
    pairs = sorted({nx // 2 for nx, _ in SOR_SHAPES})
    # a width is a multiple of 8 (cfd_create): the smallest non-zero excess over whole wave columns
    least = min(p % SOR_PAIRS for p in range(8, 8 * SOR_PAIRS + 1, 4) if p % SOR_PAIRS)
    table["sor_cols"] = dict(exact=[2 * p for p in pairs if p % SOR_PAIRS == 0],
                             least_over=[2 * p for p in pairs if p > SOR_PAIRS and p % SOR_PAIRS == least],
                             one_wave=[2 * p for p in pairs if p < SOR_PAIRS])
    assert least == 2, least
    rows = sorted({ny - 2 for _, ny in SOR_SHAPES})

    def seg(n):
        return SOR_SEG_ROWS_BIG if n >= SOR_SEG_ROWS_BIG else SOR_SEG_ROWS
    fused = [n for n in rows if n >= SOR_SEG_ROWS]
    table["sor_rows"] = dict(fallback=[n for n in rows if n < SOR_SEG_ROWS],
                             exact16=[n for n in fused if seg(n) == 16 and n % 16 == 0],
                             one_over16=[n for n in fused if seg(n) == 16 and n % 16 == 1],
                             overlap16=[n for n in fused if seg(n) == 16 and n % 16 == 15],
                             exact32=[n for n in fused if seg(n) == 32 and n % 32 == 0],
                             one_over32=[n for n in fused if seg(n) == 32 and n % 32 == 1])
    assert {ny - 2 for ny in SOR_TOL_NY} == set(rows)   # the tolerance-on cases take every row category
    for name, cats in table.items():
        print(name, cats)
        for cat, hits in cats.items():
            assert hits, f"no shape reaches {name} / {cat}"


# ------------------------------------------------------------------- helpers

def _cfd():
    import cfdamd
    return cfdamd


def _dxdy(nx, ny, lx, ly):
    return np.float32(lx) / np.float32(nx), np.float32(ly) / np.float32(ny)


@functools.lru_cache(maxsize=None)
def _mg_case(nx, ny, kind, flavour):
    """(rhs, oracle p', oracle residual) of one multigrid solve, computed once.
    flavour: signs / range, or the same with NaN on the boundary cells of rhs
    (bnan-*), or the shallow grids' one interior NaN."""
    import oracle
    if flavour == "shallow-nan":
        lx, ly = SHALLOW_LX, SHALLOW_LY
        rhs = shallow_nan_rhs(nx, ny)
    else:
        lx, ly = spacing(nx, ny, kind)
        rhs = solver_rhs(nx, ny, flavour.replace("bnan-", ""))
        if flavour.startswith("bnan-"):
            rhs = with_boundary_nan(rhs, nx, ny)
    want = np.empty(nx * ny, np.float32)
    r = np.float32(oracle.mg_solve(want, rhs, nx, ny, *_dxdy(nx, ny, lx, ly)))
    for a in (rhs, want):
        a.setflags(write=False)
    return rhs, want, r


@functools.lru_cache(maxsize=None)
def _sor_case(nx, ny, kind, flavour, iters, tol, scale=None):
    """(rhs, oracle p', oracle residual, iterations run) of one SOR solve."""
    import oracle
    lx, ly = spacing(nx, ny, kind)
    rhs = solver_rhs(nx, ny, flavour.replace("bnan-", ""), scale)
    if flavour.startswith("bnan-"):
        rhs = with_boundary_nan(rhs, nx, ny)
    want = np.empty(nx * ny, np.float32)
    r, n = oracle.sor_solve(want, rhs, nx, ny, *_dxdy(nx, ny, lx, ly), iters, tol, 1e-4)
    for a in (rhs, want):
        a.setflags(write=False)
    return rhs, want, np.float32(r), n


def _solver_model(nx, ny, lx, ly, solver, **kw):
    c = _cfd()
    return c.Model(c.Grid(nx, ny, lx, ly), c.SimulationParams(pressure_solver=c.PressureSolver(solver), **kw))


def _set_mode(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("CFD_MG_SMOOTH", raising=False)
    else:
        monkeypatch.setenv("CFD_MG_SMOOTH", mode)


def _mg_env(monkeypatch, tail, tb="1"):
    """CFD_MG_TAIL is read when the hierarchy is built (the model's first
    multigrid solve), CFD_MG_TB and CFD_MG_SMOOTH per solve / launch."""
    if tail == "default":
        monkeypatch.delenv("CFD_MG_TAIL", raising=False)
    else:
        monkeypatch.setenv("CFD_MG_TAIL", tail)
    monkeypatch.setenv("CFD_MG_TB", tb)
    monkeypatch.delenv("CFD_MG_SMOOTH", raising=False)


def _check_mg(tag, m, case, nan_equal=False):
    rhs, want, r = case
    # a p' the solve must zero first (index.html:777)
    m.set_state(rhs=rhs, p_prime=np.full(want.size, 7.0, np.float32), jacobi_sweeps_total=0)
    got = np.float32(m.pressure_solve())
    st = m.get_state()
    print(f"{tag}: residual {got!r} (oracle {r!r})")
    assert_bitwise(f"{tag}: p'", st["p_prime"], want, nan_equal=nan_equal)
    assert same_f32(got, r), (tag, got, r)
    assert st["jacobi_sweeps_total"] == 1, tag
    return st


# ------------------------------------------------------ multigrid shape matrix

def _mg_matrix_cases():
    out = [(nx, ny, kind, tail, "1") for nx, ny in MG_SHAPES for kind in SPACINGS for tail in MG_TAILS]
    out += [(nx, ny, kind, tail, "0") for nx, ny in MG_TB0_SHAPES for kind in SPACINGS for tail in MG_TAILS]
    return out


@gpu
@pytest.mark.parametrize("nx,ny,kind,tail,tb", _mg_matrix_cases())
def test_multigrid_shape_matrix(monkeypatch, nx, ny, kind, tail, tb):
    """pressure_solve() against oracle.mg_solve: p' and the residual bitwise,
    one sweep counted; one model per tail setting serves both rhs flavours and
    every smoothing form (tb 0: the single-sweep kernels, which have one form)."""
    _mg_env(monkeypatch, tail, tb)
    m = _solver_model(nx, ny, *spacing(nx, ny, kind), 2)
    try:
        for mode in (MG_SMOOTH_MODES if tb == "1" else (None,)):
            _set_mode(monkeypatch, mode)
            for flavour in ("signs", "range"):
                case = _mg_case(nx, ny, kind, flavour)
                assert nonfinite_share([case[1]]) == 0.0 and np.isfinite(case[2])
                _check_mg(f"mg {nx}x{ny} {kind} tail {tail} tb {tb} smooth {mode} {flavour}", m, case)
    finally:
        m.close()


# ------------------------------------------------------------ SOR shape matrix

@gpu
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("kind", SPACINGS)
@pytest.mark.parametrize("nx,ny", SOR_SHAPES)
def test_sor_shape_matrix(monkeypatch, nx, ny, kind, fused):
    """Seven iterations, tolerance off, of k_sor_march (CFD_SOR_FUSED=1; ny = 17
    falls back to the colour passes) and of k_sor_color (=0)."""
    monkeypatch.setenv("CFD_SOR_FUSED", fused)
    m = _solver_model(nx, ny, *spacing(nx, ny, kind), 1, jacobi_iters=SOR_ITERS, tol_enabled=False)
    try:
        for flavour in ("signs", "range"):
            tag = f"sor {nx}x{ny} {kind} fused {fused} {flavour}"
            rhs, want, r, n = _sor_case(nx, ny, kind, flavour, SOR_ITERS, False)
            assert n == SOR_ITERS and nonfinite_share([want]) == 0.0
            m.set_state(rhs=rhs, p_prime=np.full(nx * ny, 7.0, np.float32), jacobi_sweeps_total=0)
            got = np.float32(m.pressure_solve())
            st = m.get_state()
            assert_bitwise(f"{tag}: p'", st["p_prime"], want)
            assert same_f32(got, r), (tag, got, r)
            assert st["jacobi_sweeps_total"] == n, tag
    finally:
        m.close()


SOR_TOL_PROBE = 4000   # iteration limit of the oracle's probing solve


@gpu
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("kind", SPACINGS)
@pytest.mark.parametrize("ny", SOR_TOL_NY)
def test_sor_early_exit_per_row_category(monkeypatch, ny, kind, fused):
    """Tolerance on, rhs scaled by 1e-2: the solve stops where the oracle's
    does.  The limit is the smallest for which the oracle exits early, plus
    10, so the launches after the exit all have to stand down."""
    nx = 248
    monkeypatch.setenv("CFD_SOR_FUSED", fused)
    n_exit = _sor_case(nx, ny, kind, "signs", SOR_TOL_PROBE, True, 1e-2)[3]
    assert n_exit < SOR_TOL_PROBE, n_exit
    iters = n_exit + 1 + 10
    rhs, want, r, n = _sor_case(nx, ny, kind, "signs", iters, True, 1e-2)
    assert n == n_exit
    tag = f"sor tol {nx}x{ny} {kind} fused {fused} exit {n} of {iters}"
    print(tag)
    m = _solver_model(nx, ny, *spacing(nx, ny, kind), 1, jacobi_iters=iters, tol_enabled=True)
    try:
        m.set_state(rhs=rhs, p_prime=np.full(nx * ny, 7.0, np.float32), jacobi_sweeps_total=0)
        got = np.float32(m.pressure_solve())
        st = m.get_state()
        assert_bitwise(f"{tag}: p'", st["p_prime"], want)
        assert same_f32(got, r), (tag, got, r)
        assert st["jacobi_sweeps_total"] == n, (tag, st["jacobi_sweeps_total"])
        assert n < iters
    finally:
        m.close()


# ---------------------------------------------------------------- stale buffers

def _variants():
    return [(2, "default"), (2, "0"), (1, "1"), (1, "0")]   # (solver, CFD_MG_TAIL or CFD_SOR_FUSED)


@gpu
@pytest.mark.parametrize("solver,variant", _variants())
@pytest.mark.parametrize("kind", SPACINGS)
@pytest.mark.parametrize("nx,ny", [(56, 15), (248, 35)])
def test_solve_ignores_stale_nan_in_both_buffers(monkeypatch, nx, ny, kind, solver, variant):
    """Both scripts zero p' first (index.html:743, :777).  A three-sweep Jacobi
    launch on the `nonfinite` state leaves NaN-spoilt words in both p'
    ping-pong buffers; the model then switches solver, takes a finite rhs and
    must give the oracle's result with no non-finite word: nothing of either
    buffer may be read before it is written."""
    c = _cfd()
    if solver == 2:
        _mg_env(monkeypatch, variant)
    else:
        monkeypatch.setenv("CFD_SOR_FUSED", variant)
    lx, ly = spacing(nx, ny, kind)
    m = _solver_model(nx, ny, lx, ly, 0, jacobi_iters=3, tol_enabled=False)
    try:
        st = adversarial_state(nx, ny, 1, "nonfinite")
        if np.isfinite(st["p_prime"]).all():      # a grid too small for the flavour to reach p'
            st["p_prime"][nx // 2 + (ny // 2) * nx] = np.nan
        planted = np.count_nonzero(~np.isfinite(st["p_prime"]))
        load_state(st, model=m)
        m.jacobi_pressure()
        spoilt = np.count_nonzero(~np.isfinite(m.get_state()["p_prime"]))
        assert spoilt > planted >= 1, (spoilt, planted)   # the written buffer; the read one kept `planted`
        m.set_parameters(c.SimulationParams(pressure_solver=c.PressureSolver(solver),
                                            jacobi_iters=SOR_ITERS, tol_enabled=False))
        tag = f"stale {nx}x{ny} {kind} solver {solver} variant {variant}"
        if solver == 2:
            case = _mg_case(nx, ny, kind, "signs")
            m.set_state(rhs=case[0], jacobi_sweeps_total=0)   # p' keeps its spoilt words
            got = np.float32(m.pressure_solve())
            want, r, n = case[1], case[2], 1
        else:
            rhs, want, r, n = _sor_case(nx, ny, kind, "signs", SOR_ITERS, False)
            m.set_state(rhs=rhs, jacobi_sweeps_total=0)
            got = np.float32(m.pressure_solve())
        out = m.get_state()
        assert nonfinite_share([out["p_prime"]]) == 0.0, tag
        assert_bitwise(f"{tag}: p'", out["p_prime"], want)
        assert same_f32(got, r), (tag, got, r)
        assert out["jacobi_sweeps_total"] == n, tag
    finally:
        m.close()


# ------------------------------------------------- NaN on every boundary rhs cell

@gpu
@pytest.mark.parametrize("solver,variant", _variants())
@pytest.mark.parametrize("kind", SPACINGS)
@pytest.mark.parametrize("nx,ny", [(56, 15), (216, 29), (248, 35)])
def test_boundary_rhs_nan_is_never_used(monkeypatch, nx, ny, kind, solver, variant):
    """The kernels load the boundary cells of rhs into their windows; nothing
    may use them.  The result is the oracle's, which test_oracle_solvers.py
    shows to be the NaN-free solve's: no non-finite word, a finite residual."""
    if solver == 2:
        _mg_env(monkeypatch, variant)
    else:
        monkeypatch.setenv("CFD_SOR_FUSED", variant)
    m = _solver_model(nx, ny, *spacing(nx, ny, kind), solver, jacobi_iters=SOR_ITERS, tol_enabled=False)
    try:
        tag = f"boundary NaN {nx}x{ny} {kind} solver {solver} variant {variant}"
        if solver == 2:
            case = _mg_case(nx, ny, kind, "bnan-signs")
            assert_bitwise("oracle", case[1], _mg_case(nx, ny, kind, "signs")[1])
            assert np.isfinite(case[2])
            for mode in (None, "2", "3"):
                _set_mode(monkeypatch, mode)
                st = _check_mg(f"{tag} smooth {mode}", m, case)
                assert nonfinite_share([st["p_prime"]]) == 0.0
        else:
            rhs, want, r, n = _sor_case(nx, ny, kind, "bnan-signs", SOR_ITERS, False)
            assert_bitwise("oracle", want, _sor_case(nx, ny, kind, "signs", SOR_ITERS, False)[1])
            assert np.isfinite(r)
            m.set_state(rhs=rhs, p_prime=np.full(nx * ny, 7.0, np.float32), jacobi_sweeps_total=0)
            got = np.float32(m.pressure_solve())
            st = m.get_state()
            assert nonfinite_share([st["p_prime"]]) == 0.0
            assert_bitwise(f"{tag}: p'", st["p_prime"], want)
            assert same_f32(got, r), (tag, got, r)
            assert st["jacobi_sweeps_total"] == n
    finally:
        m.close()


# ------------------------------------------- the NaN-ignoring final residual

@gpu
@pytest.mark.parametrize("nx,ny,tail", [(nx, ny, "default") for nx, ny in SHALLOW_NAN_GRIDS] + [(2048, 5, "0")])
def test_multigrid_final_residual_ignores_nan(monkeypatch, nx, ny, tail):
    """One NaN in rhs at (nx / 2, 1) on hierarchies of one and two levels: it
    spoils a small share of p' (asserted, so nan_equal hides little), and the
    residual of k_mg_final_residual is the maximum over the cells it has not
    reached: finite, positive, the oracle's bits.  2048 x 5 runs its finest
    level grid-wide, so the NaN passes through the fused residual, the
    restriction and the prolong-add (under every smoothing form)."""
    _mg_env(monkeypatch, tail)
    case = _mg_case(nx, ny, "shallow", "shallow-nan")
    share = nonfinite_share([case[1]])
    assert 0.0 < share <= MAX_NONFINITE_SHARE, share
    assert np.isfinite(case[2]) and case[2] > 0.0, case[2]
    m = _solver_model(nx, ny, SHALLOW_LX, SHALLOW_LY, 2)
    try:
        for mode in MG_SMOOTH_MODES:
            _set_mode(monkeypatch, mode)
            _check_mg(f"shallow NaN {nx}x{ny} tail {tail} smooth {mode} share {share:.4f}", m, case,
                      nan_equal=True)
    finally:
        m.close()


# ------------------------------------------- whole steps from adversarial state

STEP_GRIDS = {
    "cavity-56x15": dict(nx=56, ny=15, lx=56 / 128.0, ly=15 / 128.0),
    # the cylinder as CHANNELS of test_gpu_adversarial.py sizes it
    "channel-248x35": dict(nx=248, ny=35, lx=30.0, ly=10.0, cylinder=(7.5, 5.0, 1.5)),
}


@gpu
@pytest.mark.parametrize("passes", [0, 2])
@pytest.mark.parametrize("flavour", ["signs", "range"])
@pytest.mark.parametrize("solver", [1, 2])
@pytest.mark.parametrize("grid", sorted(STEP_GRIDS))
def test_steps_from_adversarial_state(grid, solver, flavour, passes):
    """update() twice with SOR (6 iterations, tolerance off) or multigrid from
    an adversarial state: every field and scalar bitwise after each step."""
    from test_gpu_adversarial import _compare_step, _model
    g = STEP_GRIDS[grid]
    kw = dict(pressure_solver=solver, corrector_passes=passes, tol_enabled=0, jacobi_iters=6)
    if "cylinder" not in g:
        kw.update(bc_kind=1, viscosity=0.01)
    m, o = _model(g, **kw)
    try:
        load_state(adversarial_state(g["nx"], g["ny"], 1, flavour), model=m, oracle=o)
        for step in (1, 2):
            o.update()
            m.update()
            _compare_step(f"{grid} solver {solver} {flavour} passes {passes} step {step}", m, o,
                          nan_equal=False)
        assert nonfinite_share([o.field(f) for f in ADV_FIELDS]) == 0.0
        m.get_residuals()
    finally:
        m.close()
