"""The case table of the script-order SOR's seam tests (pressure_solver 4,
cfd_sor_lex.hip): test_sor_lex_seams_cpu.py checks its premises with the
restatement alone (tests/_sor_lex_ref.py), test_gpu_sor_lex_seams.py runs the
kernel on every case a model can be built for.

The kernel gives a wave a band of 64 interior rows (B = ceil((ny - 2) / 64)
bands) and walks a band in chunks of 16 steps, NC = ceil((nx + 62) / 16) of
them.  With the tolerance on, the band that finishes an iteration last -- the
last band: it waits for the one below it -- tests the maximum all bands folded.

A case is a grid, an iteration limit, the tolerance switch and an rhs recipe
(seed, scale, optional rows): uniform(-1, 1) * scale in f32 from
default_rng(seed), then every row outside `rows` (inclusive) set to 0, so
nothing large is committed.  `exit` says where the restatement must stop:

    none   all `iters` iterations run (the tolerance off, or never met);
    mid    1 < n < iters;
    last   n == iters with the last maxError below p_tol (the replay launch
           returns at once);
    first  n == 1.

`n` is the iteration count measured with the restatement where a case was built
for one (asserted on the CPU); `band` names the band the rhs is confined to.

cfd_create takes nx % 8 == 0 only (include/cfd.h), so the chunk count never
fits nx + 62 exactly on the device: (nx + 62) % 16 is 14 or 6.  The widths one
short of, at and one past an exact fit (17, 18, 19, 34, 35) stay in the table
for the restatement -- `device` is False for them, and the CPU file asserts
that the constructor refuses each -- and the widths next to them that a model
accepts (16, 24, 32, 40) run on the device, both remainders included.
"""
from collections import namedtuple

import numpy as np

import _sor_lex_ref as ref

P_TOL = 1e-4
BAND = 64

Case = namedtuple("Case", "name nx ny lx ly iters tol seed scale rows exit n band device")


def _case(name, nx, ny, iters, tol, seed, scale, exit, rows=None, n=None, band=None, pow2=False):
    lx, ly = (nx / 128.0, ny / 128.0) if pow2 else (30.0, 10.0)
    return Case(name, nx, ny, lx, ly, iters, tol, seed, scale, rows, exit, n, band, nx % 8 == 0)


# ---- exits on more than one band (24 x 132: three bands, x x 195: four, the last of one row)
EXIT_CASES = [
    # the maximum in the first band; the last band, which tests, is far below p_tol
    _case("first_band", 24, 132, 100, True, 11, 0.03, "mid", rows=(1, 20), n=25, band=0),
    _case("first_band_exit_at_last", 24, 132, 25, True, 11, 0.03, "last", rows=(1, 20), n=25, band=0),
    _case("first_band_replay_of_one", 24, 132, 26, True, 11, 0.03, "mid", rows=(1, 20), n=25, band=0),
    # the maximum in the last band: nonzero rhs in the last two interior rows only
    _case("last_band_s0.03", 24, 132, 100, True, 12, 0.03, "mid", rows=(129, 130), n=9, band=2),
    _case("last_band_s0.1", 24, 132, 100, True, 12, 0.1, "mid", rows=(129, 130), n=38, band=2),
    _case("middle_band", 24, 132, 100, True, 13, 0.03, "mid", rows=(70, 99), n=35, band=1),
    # the first iteration already meets the tolerance
    _case("four_bands_first_iteration_34", 34, 195, 100, True, 3, 0.01, "first", n=1),
    _case("four_bands_first_iteration", 32, 195, 100, True, 3, 0.01, "first", n=1),
    _case("zero_rhs_three_bands", 24, 132, 100, True, 3, 0.0, "first", n=1),
    # both parities of the exit on more than one band
    _case("four_bands_odd_34", 34, 195, 100, True, 3, 0.03, "mid", n=15),
    _case("four_bands_odd", 32, 195, 100, True, 3, 0.03, "mid", n=15),
    _case("four_bands_even", 40, 195, 100, True, 3, 0.03, "mid", n=12),
    _case("three_bands_even", 24, 132, 100, True, 3, 0.01, "mid", n=12),
    _case("three_bands_odd", 24, 132, 100, True, 4, 0.01, "mid", n=7),
    # a one-row last band that takes the exit test with the maximum elsewhere
    _case("one_row_band_tests_first_band", 16, 67, 100, True, 14, 0.01, "mid", rows=(1, 20), n=38,
          band=0),
]

# ---- band and chunk edges: (nx, ny, pow2 spacing, seed, scale of the exiting solve)
# ny - 2 in {2 (the smallest: ny >= 4), 63, 64, 65, 128, 129, 193}; nx in
# {16 (the smallest), 24, 32, 40} on the device and {17, 18, 19, 34, 35} beside them
_GRIDS = [
    (16, 4, False, 31, 3e-4), (24, 4, True, 32, 10.0), (17, 4, False, 41, 3e-4),
    (40, 65, False, 33, 0.01),
    (32, 66, False, 34, 0.01), (24, 66, True, 35, 10.0), (35, 66, False, 44, 0.01),
    (16, 67, False, 36, 0.003), (40, 67, False, 37, 0.01), (18, 67, False, 42, 0.01),
    (24, 130, False, 38, 0.01), (34, 130, False, 45, 0.01),
    (16, 131, False, 39, 0.01), (32, 131, True, 40, 10.0), (19, 131, False, 43, 0.01),
    (32, 195, False, 3, 0.03), (40, 195, False, 3, 0.03), (34, 195, False, 3, 0.03),
]
FIXED_ITERS = 7      # more than two iterations of a band in flight
EXIT_ITERS = 60

GEOMETRY_CASES = []
for _nx, _ny, _p2, _seed, _scale in _GRIDS:
    _tag = f"{_nx}x{_ny}" + ("_p2" if _p2 else "")
    GEOMETRY_CASES.append(_case(_tag + "_fixed7", _nx, _ny, FIXED_ITERS, False, _seed,
                                1000.0 if _p2 else 1.0, "none", pow2=_p2))
    GEOMETRY_CASES.append(_case(_tag + "_exit", _nx, _ny, EXIT_ITERS, True, _seed, _scale, "mid",
                                pow2=_p2))

CASES = EXIT_CASES + GEOMETRY_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the substep cases: a 24 x 132 channel with a cylinder, velocities of
# _random_state (test_gpu_script_step.py) at a CFL number this small, so that
# the rhs the predictor forms meets the tolerance mid-run
STEP_GRID = dict(nx=24, ny=132, lx=30.0, ly=10.0, nu=0.01, cyl=(7.5, 5.0, 0.75))
STEP_CFL = 3e-7
STEP_ITERS = 100
DEVICE_CASES = [c for c in CASES if c.device]
# tolerance-on cases whose last band is a single row (it takes the exit test)
ONE_ROW_LAST_BAND = [c for c in CASES if c.tol and (c.ny - 2) % BAND == 1 and c.ny - 2 > BAND]


# ---- one non-finite rhs word above the seam between the last two bands of 24 x 132
# (rows 128 | 129): it spoils row 130 in iteration 1, 129 in 2 and 128 in 3, so
# it crosses the seam through the memory reads of the band's top lane and of
# lane 0, not through the lanes' exchange.  The last case exits with NaN present.
NONFINITE_CELL = (20, 130)
NONFINITE_SHARE = 0.05      # cap on the non-finite share of the expected p'
NONFINITE_CASES = [
    (_case("nan_fixed6", 24, 132, 6, False, 21, 1.0, "none"), np.float32(np.nan)),
    (_case("inf_fixed6", 24, 132, 6, False, 21, 1.0, "none"), np.float32(np.inf)),
    (_case("nan_exit", 24, 132, 60, True, 21, 0.01, "mid", n=8), np.float32(np.nan)),
]


# ---- one three-band model, five solves and no fresh model in between: whatever
# the p' buffers, the exit word and the polled block hold from the solve before,
# each result is the restatement of that solve alone
STALE_SEQUENCE = [
    _case("stale_a_odd_fixed", 24, 132, 7, False, 51, 1.0, "none"),        # the current buffer flips
    _case("stale_a_one_iteration", 24, 132, 1, False, 52, 1.0, "none"),    # writes one buffer only
    BY_NAME["first_band_replay_of_one"],                                   # more iterations: the block grows
    _case("stale_c_never_below", 24, 132, 9, True, 53, 100.0, "none"),     # the old exit word must not leak
    BY_NAME["middle_band"],                                                # grows again (100 iterations)
    _case("stale_e_fewer_iterations", 24, 132, 30, True, 4, 0.01, "mid", n=7),
]


def nonfinite_restated(c, word):
    """restated() of a NONFINITE_CASES entry, the word planted in its rhs."""
    key = c.name + "+word"
    if key not in _REF:
        rhs = rhs_of(c)
        rhs[NONFINITE_CELL[0] + NONFINITE_CELL[1] * c.nx] = word
        _REF[key] = (rhs,) + solve(c, rhs)
        for a in _REF[key][:2]:
            a.setflags(write=False)
    return _REF[key]


def bands(ny):
    return -(-(ny - 2) // BAND)


def spacings(c):
    return np.float32(c.lx) / np.float32(c.nx), np.float32(c.ly) / np.float32(c.ny)


def make_rhs(nx, ny, seed, scale, rows=None):
    rhs = (np.random.default_rng(seed).uniform(-1, 1, nx * ny) * scale).astype(np.float32)
    if rows is not None:
        r = rhs.reshape(ny, nx)
        r[:rows[0]] = 0.0
        r[rows[1] + 1:] = 0.0
    return rhs


def rhs_of(c):
    return make_rhs(c.nx, c.ny, c.seed, c.scale, c.rows)


def solve(c, rhs, iters=None, tol=None):
    """The restatement (anti-diagonal form) of one solve with the case's grid."""
    dx, dy = spacings(c)
    return ref.sor_lex_diag(rhs, c.nx, c.ny, dx, dy, c.iters if iters is None else iters,
                            c.tol if tol is None else tol, P_TOL)


_REF = {}


def restated(c):
    """(rhs, p' [ny, nx], iterations run, maxError list), computed once per
    case; callers leave the arrays unchanged."""
    if c.name not in _REF:
        rhs = rhs_of(c)
        _REF[c.name] = (rhs,) + solve(c, rhs)
        for a in _REF[c.name][:2]:
            a.setflags(write=False)
    return _REF[c.name]


def band_maxima(c, m):
    """max |P(m) - P(m-1)| over each band's interior cells, P(k) the
    fixed-count result of k iterations: what each band folds in iteration m
    (1-based)."""
    rhs = rhs_of(c)
    a = solve(c, rhs, m, False)[0].astype(np.float64)
    b = solve(c, rhs, m - 1, False)[0].astype(np.float64)
    d = np.abs(a - b)[1:c.ny - 1, 1:c.nx - 1]
    return [float(d[s:s + BAND].max()) for s in range(0, c.ny - 2, BAND)]
