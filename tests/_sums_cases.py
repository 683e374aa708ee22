"""States at the edge of the fma-form guard (test infrastructure only), shared
by tests/test_sums_guard_cpu.py, which steps the oracle alone over them and
pins every premise, and tests/test_gpu_sums_fma_shapes.py, which runs them on
the device.  Grids have dx = dy = 2^-7: R = 1 / dx^2 = 2^14."""
import numpy as np

from _util import adversarial_state, bits

P2 = 1.0 / 128.0
R = 2.0 ** 14
LIM = 2.0 ** 123                       # the guard: m0 R + SUMS_C rm < LIM
SUMS_C = 0.1875 * 4096                 # 768
P_THR = 2.0 ** 122 / R                 # the finish publishes at least this (2^108)
R_THR = 2.0 ** 112                     # the predictor march publishes at least this
P_THR_BITS = int(np.float32(P_THR).view(np.uint32))
INF_BITS = 0x7F800000
MI355X_CUS = 256                       # the CPU side's stand-in for the band shape


def grid(nx, ny):
    return dict(nx=nx, ny=ny, lx=nx * P2, ly=ny * P2)


def band_shape(n_cu):
    """16 columns, 32 rows per CU + 9: k_correct_finish4m takes its 16-row
    bands (cf_rows) and the last band is ragged."""
    nx, ny = 16, 32 * n_cu + 9
    assert -(-(ny + 1) // 16) >= 2 * n_cu and (ny + 1) % 16 != 0
    return nx, ny


def abs_bits_max(a):
    return int((bits(a) & np.uint32(0x7FFFFFFF)).max())


def argmax_cells(pp, nx):
    """(column, row) of every cell whose |p'| bits equal the field's largest."""
    b = bits(pp) & np.uint32(0x7FFFFFFF)
    return [(int(k) % nx, int(k) // nx) for k in np.nonzero(b == b.max())[0]]


def guard_bound(pp_before, rhs):
    """The guard's sum in f32 from the p' a solve starts from and its rhs, as
    the publishers bound them (each at least its threshold)."""
    m0 = max(np.float32(P_THR), np.float32(np.max(np.abs(pp_before))))
    rm = max(np.float32(R_THR), np.float32(np.max(np.abs(rhs))))
    with np.errstate(over="ignore"):   # an overflowed sum is Inf and fails the guard's test
        return np.float32(np.float32(m0 * np.float32(R)) +
                          np.float32(np.float32(SUMS_C) * rm))


# --------------------------------------------- section 3: one p' cell decides

SPIKE_S = np.float32(1.37 * 2.0 ** 112)   # one sweep leaves 0.25 S at the cell, 0.1875 S beside it
SPIKE_DT = np.float32(2.0 ** -100)        # rhs <= 2^10 / dt: its share of p' is below 2^95, and the
                                          # correction dt S / dx about 2^19 keeps every field finite


def finish_cells(shape, nx, ny):
    """[(class, column, row)] of the planted p' cell.  After one sweep the
    boundary copies repeat row 1 in row 0, row ny-2 in row ny-1 and column 1 in
    column 0, so those classes share their maximum with the copy; `last_row`
    plants in row ny-1 itself, which the sweep reads for row ny-2 and the copy
    then overwrites: the maximum stands in rows ny-2 and ny-1 alike."""
    mid_c, mid_r = (nx // 2) | 1, ny // 2
    if shape == "band":
        last = 16 * ((ny + 1) // 16)          # first row of the ragged last band
        assert last < ny - 2
        return [("row15", 5, 15), ("row16", 10, 16), ("before_last_band", 7, last - 1),
                ("last_band", 4, last), ("row_ny-2", 13, ny - 2), ("last_row", 6, ny - 1)]
    cells = [("col1", 1, mid_r), ("col_nx-2", nx - 2, mid_r)]
    if nx > 1024:
        cells += [("chunk_left", 1023, ny - 3), ("chunk_right", 1024, 2)]
    elif nx == 1024:
        cells += [("chunk_end", 1021, 1)]
    else:
        cells += [("row1", mid_c, 1), ("row_ny-2", mid_c + 2, ny - 2), ("last_row", mid_c + 3, ny - 1)]
    return cells


FINISH_SHAPES = ("120x37", "1024x5", "1032x6", "band")
FINISH_KINDS = ("spike", "nan", "inf")


def shape_of(shape, n_cu=MI355X_CUS):
    return band_shape(n_cu) if shape == "band" else tuple(int(x) for x in shape.split("x"))


def finish_state(nx, ny, col, row, kind):
    """`signs` velocities, p' and rhs noise <= 1e-3 and one planted p' word."""
    st = adversarial_state(nx, ny, 3, "signs")
    rng = np.random.default_rng([nx, ny, 31])
    st["p_prime"] = rng.uniform(-1e-3, 1e-3, nx * ny).astype(np.float32)
    st["rhs"] = rng.uniform(-1e-3, 1e-3, nx * ny).astype(np.float32)
    st["p_prime"][col + row * nx] = {"spike": SPIKE_S, "nan": np.float32(np.nan),
                                     "inf": np.float32(np.inf)}[kind]
    return st


def class_holds_max(pp, nx, ny, col, row):
    """The planted cell's class holds the field's largest |p'| (read from the
    state): the cell itself, or for row ny-1 the copy the boundary left there."""
    cells = argmax_cells(pp, nx)
    return (col, row) in cells


# ------------------------------------------ section 4: one rhs cell decides

MARCH_V = np.float32(3.0)             # the planted face velocity
MARCH_BG = 2.0 ** -14                 # `signs` velocities times this
MARCH_DT_HI = np.float32(2.0 ** -110)   # |rhs| of the planted face about 3 * 2^7 / dt = 1.5 * 2^118
MARCH_DT_LO = np.float32(2.0 ** -90)    # the twin, 20 binades lower
RHS_DECIDES = 2.0 * LIM / SUMS_C      # 768 |rhs| >= 2 LIM


def march_faces(shape, nx, ny):
    """[(class, face, row)] of the planted u face.  Face nx is left out: the
    boundary conditions rewrite it at the end of every step, so no state
    reaches a second step with a value of its own there; cell nx-1, the last
    one the last chunk's lane stores, is reached through face nx-1."""
    mid_r = ny // 2
    faces = [("face1", 1, mid_r), ("face_nx-1", nx - 1, mid_r)]
    # k_predict_march: lanes 1..62 of a wave column store 62 four-cell chunks;
    # 240 columns are 60 chunks of one wave column, 248 fill it (62) and leave
    # face nx to the second.  Face nx-4 lies between the last two chunks.
    faces += [("last_chunks", nx - 4, mid_r), ("first_row", nx // 3, 1), ("last_row", nx // 3 + 1, ny - 2)]
    if ny >= 12:
        # 8-row segments, the last one moved up to end at ny: rows ny-8 .. 7
        # are stored by both, row 8 only by the last
        faces += [("row7_two_segments", 101, 7), ("row8_last_segment", 102, 8)]
    return faces


# 1032 x 6: under 8 rows, the march's 4-row segments
MARCH_SHAPES = ("120x37", "240x12", "248x13", "1032x6")


def march_state(nx, ny, face, row):
    st = adversarial_state(nx, ny, 4, "signs")
    for f in ("u", "v", "u_star", "v_star"):
        st[f] = (st[f] * np.float32(MARCH_BG)).astype(np.float32)
    st["p_prime"][:] = 0.0
    st["rhs"][:] = 0.0
    st["p"] = (st["p"] * np.float32(2.0 ** -10)).astype(np.float32)
    st["u"][face + row * (nx + 1)] = MARCH_V
    return st


# --------------------------------------------- section 5: the window's top

TOP_DT = np.float32(2.0 ** -116)
TOP_SHAPES = ((120, 37), (16, 4))
TOP_SWEEPS = (9, 24)
TOP_FACTORS = {"inside": 1.1, "above": 1.5}    # R C = factor * 2^122
TOP_MARGIN = 2.0 ** -10


def top_state(nx, ny, factor):
    """p' = C (1 + delta), delta a few ulps of mixed pattern, C R = factor *
    2^122, consistent with the boundary rows and columns a sweep leaves
    (column nx-1 zero, column 0 and rows 0 / ny-1 copies); u = dt grad p'
    exactly as the corrector forms it, so the first step's rhs is the
    Laplacian of p', its solve keeps p' to a few ulps, and the corrected
    velocities -- the second step's rhs times dt -- are rounding residue."""
    c = np.float32(factor * 2.0 ** 122 / R)
    rng = np.random.default_rng([nx, ny, 51])
    ulps = rng.integers(-6, 7, (ny, nx)).astype(np.int64)
    ulps[::3, ::2] = 6
    ulps[1::4, 1::3] = -6
    pp = (np.full((ny, nx), c, np.float32).view(np.uint32).astype(np.int64) + ulps).astype(np.uint32)
    pp = pp.view(np.float32).copy()
    pp[0, :] = pp[1, :]
    pp[ny - 1, :] = pp[ny - 2, :]
    pp[:, 0] = pp[:, 1]
    pp[:, nx - 1] = 0.0
    dt, dx = TOP_DT, np.float32(P2)
    u = np.zeros((ny, nx + 1), np.float32)
    u[:, 1:nx] = dt * ((pp[:, 1:] - pp[:, :-1]) / dx)
    # rows 0 and ny-1 of u* are never predicted: what a state holds there
    # stays in every later rhs of those rows, so they start at zero
    u[0, :] = u[ny - 1, :] = 0.0
    v = np.zeros((ny + 1, nx), np.float32)
    v[1:ny, :] = dt * ((pp[1:, :] - pp[:-1, :]) / dx)
    z = np.zeros(nx * ny, np.float32)
    return {"u": u.ravel(), "v": v.ravel(), "u_star": u.ravel().copy(), "v_star": v.ravel().copy(),
            "p": z.copy(), "p_prime": pp.ravel(), "rhs": z.copy()}


def counter_must(bound):
    """What the guard must answer to a bound formed on the host: True the form
    runs, False it is refused, None inside the margin that keeps clear of the
    one-ulp difference between a contracted and an uncontracted evaluation."""
    if not np.isfinite(bound):
        return False
    if bound <= LIM * (1.0 - TOP_MARGIN):
        return True
    if bound >= LIM * (1.0 + TOP_MARGIN):
        return False
    return None
