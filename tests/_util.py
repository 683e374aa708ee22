"""Shared helpers for the test-suite (test infrastructure only)."""
import numpy as np

STATE_FIELDS = ("u", "v", "p", "u_star", "v_star", "p_prime")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).ravel()


def assert_bitwise(name, got, want, nan_equal=False):
    """Every f32 word identical.  nan_equal: any NaN matches any NaN (the
    sign/payload of a NaN produced by arithmetic is the hardware's default
    NaN, not part of the reference's semantics)."""
    assert np.shape(got) == np.shape(want), f"{name}: shape {np.shape(got)} != {np.shape(want)}"
    g, w = bits(got), bits(want)
    ne = g != w
    if nan_equal:
        ne &= ~(np.isnan(g.view(np.float32)) & np.isnan(w.view(np.float32)))
    bad = np.nonzero(ne)[0]
    if bad.size:
        k = bad[0]
        raise AssertionError(
            f"{name}: {bad.size}/{g.size} words differ; first at {k}: got "
            f"{np.float32(got.ravel()[k])!r} want {np.float32(want.ravel()[k])!r}")


def same_f32(a, b):
    """Two f32 scalars with identical bits."""
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)


# ---------------------------------------------------------------------------
# Adversarial states: random, wide-range and non-finite fields for the parity
# tests (test_gpu_adversarial.py on the device, test_adversarial_cpu.py for the
# two restatements of the reference).

ADV_FIELDS = ("u", "v", "u_star", "v_star", "p", "p_prime", "rhs")
ADV_FLAVOURS = ("signs", "range", "nonfinite")
ADV_STEP = 50           # simulation_step of a loaded state: the inlet ramp (100 steps) mid-way
ADV_VEL_CAP = 8.0       # |u|, |v| <= 8: the CFL dt of the next step stays a normal number
# the non-finite words planted by the `nonfinite` flavour, in this order; a
# grid takes one per 1500 cells (at least one, at most all five: 3 NaN of
# both signs, +Inf and -Inf), which keeps the spoilt share of a step's result
# under 14 % on every shape of test_gpu_adversarial.py (worst: 112 x 9)
_NONFINITE = (("u", 0x7FC00000), ("p_prime", 0x7F800000), ("v", 0xFFC00000), ("u", 0xFF800000),
              ("p_prime", 0x7FC00001))


def _field_sizes(nx, ny):
    su, sv, sp = (nx + 1) * ny, nx * (ny + 1), nx * ny
    return {"u": su, "v": sv, "u_star": su, "v_star": sv, "p": sp, "p_prime": sp, "rhs": sp}


def nonfinite_cells(nx, ny):
    """[(field, flat index, f32 bits)] of the `nonfinite` flavour: interior
    cells spread evenly along the longer side of the grid, on alternating
    sides of its middle line, so that what each one spoils in a step stays
    apart from the others'."""
    n = max(1, min(len(_NONFINITE), (nx * ny) // 1500))
    out = []
    for k in range(n):
        f, word = _NONFINITE[k]
        frac = (2 * k + 1) / (2.0 * n)
        if nx >= ny:
            i = min(max(int(frac * nx), 2), nx - 3)
            j = min(max(ny // 2 + (1 if k % 2 else -1) * (ny // 4), 1), ny - 2)
        else:
            j = min(max(int(frac * ny), 2), ny - 3)
            i = min(max(nx // 2 + (1 if k % 2 else -1) * (nx // 4), 2), nx - 3)
        pitch = nx + 1 if f == "u" else nx
        out.append((f, i + j * pitch, word))
    return out


def adversarial_state(nx, ny, seed, flavour):
    """f32 arrays for u, v, u*, v*, p, p', rhs in the reference's flat layout
    (u rows of nx+1 faces, v of ny+1 rows), independent per field:

    signs      uniform in (-1, 1);
    range      random sign, magnitude log-uniform over 2^-40 .. 2^3, about 1 %
               of the words exact +0 / -0 and about 1 % subnormal; velocities
               capped at ADV_VEL_CAP;
    nonfinite  `signs` with the words of nonfinite_cells() planted."""
    assert flavour in ADV_FLAVOURS, flavour
    rng = np.random.default_rng([nx, ny, seed, ADV_FLAVOURS.index(flavour)])
    out = {}
    for f, n in _field_sizes(nx, ny).items():
        if flavour == "range":
            mag = np.exp2(rng.uniform(-40.0, 3.0, n)).astype(np.float32)
            kind = rng.uniform(0.0, 1.0, n)
            sub = kind < 0.01     # subnormal: any non-zero 23-bit fraction, exponent field 0
            mag[sub] = rng.integers(1, 1 << 23, int(sub.sum()), dtype=np.uint32).view(np.float32)
            mag[(kind >= 0.01) & (kind < 0.02)] = 0.0
            a = np.where(rng.uniform(0.0, 1.0, n) < 0.5, -mag, mag).astype(np.float32)
            if f in ("u", "v", "u_star", "v_star"):
                a = np.clip(a, -ADV_VEL_CAP, ADV_VEL_CAP).astype(np.float32)
        else:
            a = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        out[f] = a
    if flavour == "nonfinite":
        for f, idx, word in nonfinite_cells(nx, ny):
            out[f].view(np.uint32)[idx] = word
    return out


def load_state(st, model=None, oracle=None, np_model=None, step=ADV_STEP, dt=None):
    """Write the arrays of `st` (adversarial_state) and the step scalars into a
    cfdamd.Model (set_state), an OracleModel (field()[:] / set_scalars) and an
    NpModel, whichever are given: the same simulation_step (inlet ramp mid-way),
    time, zero sweep count and, when given, dt in each."""
    time = np.float32(step) * np.float32(0.005)
    if model is not None:
        kw = dict(st, simulation_step=step, simulation_time=time, jacobi_sweeps_total=0)
        if dt is not None:
            kw["dt"] = np.float32(dt)
        model.set_state(**kw)
    if oracle is not None:
        for f in ADV_FIELDS:
            oracle.field(f)[:] = st[f]
        s = oracle.scalars()
        s.step, s.time, s.jacobi_sweeps_total = step, time, 0
        if dt is not None:
            s.dt = np.float32(dt)
        oracle.set_scalars(s)
    if np_model is not None:
        for f in ADV_FIELDS:
            getattr(np_model, "pp" if f == "p_prime" else f)[:] = st[f]
        np_model.step, np_model.time, np_model.sweeps = step, time, 0
        if dt is not None:
            np_model.dt = np.float32(dt)


def nonfinite_share(arrays):
    """Largest share of non-finite words in any of the arrays."""
    return max(float(np.count_nonzero(~np.isfinite(a))) / a.size for a in arrays)


# inputs of the SOR / multigrid seam tests (test_gpu_solver_seams.py on the
# device, test_oracle_solvers.py for their premises with the oracle alone)

SPACINGS = ("pow2", "div")
# (nx, ny) of the NaN-ignoring final residual: lx = 8, ly = 1, one and two levels
SHALLOW_NAN_GRIDS = [(1024, 4), (2048, 4), (2048, 5)]
SHALLOW_LX, SHALLOW_LY = 8.0, 1.0


def spacing(nx, ny, kind):
    """(lx, ly): pow2 gives dx = dy = 2^-7 (every division of the solvers by a
    grid constant becomes a multiply by its exact reciprocal), div a 30 x 10
    domain (IEEE double division)."""
    assert kind in SPACINGS, kind
    return (nx / 128.0, ny / 128.0) if kind == "pow2" else (30.0, 10.0)


def solver_rhs(nx, ny, flavour, scale=None):
    """rhs of a pressure solve from adversarial_state's per-field generator:
    `signs` times 50 (as the large multigrid grids), `range` as it is."""
    rhs = adversarial_state(nx, ny, 1, flavour)["rhs"]
    if scale is None:
        scale = 50.0 if flavour == "signs" else 1.0
    return (rhs * np.float32(scale)).astype(np.float32)


def with_boundary_nan(rhs, nx, ny):
    """A copy with NaN on every boundary cell (neither solver may read them)."""
    r = rhs.reshape(ny, nx).copy()
    r[0, :] = r[ny - 1, :] = np.nan
    r[:, 0] = r[:, nx - 1] = np.nan
    return r.ravel()


def shallow_nan_rhs(nx, ny):
    """uniform(-1, 1) with one NaN at (nx / 2, 1)."""
    rhs = np.random.default_rng([nx, ny, 77]).uniform(-1, 1, nx * ny).astype(np.float32)
    rhs[nx // 2 + nx] = np.nan
    return rhs


# planted-spike states of the Jacobi residual tests

SPIKE_NOISE = 1e-3
# tolerances of the tolerance-mode spike solves on 120 x 37 (<= 50 sweeps): the
# reference's early exit (model.rs:816) falls on sweeps 1 .. 10 and beyond, and
# 1e-4 runs to the limit (asserted in test_adversarial_cpu.py)
SPIKE_P_TOLS = (0.3, 0.1, 0.04, 0.02, 0.012, 0.008, 0.004, 1e-4)


def spike_columns(nx):
    """Columns of the planted p' spike: first and last column of the residual
    (1, nx-8), the first excluded one (nx-7), the last swept one (nx-2) and the
    two sides of the seam between 112-column wave columns, where the grid has it."""
    cols = [1, nx - 8, nx - 7, nx - 2] + [c for c in (112, 113) if c < nx - 1]
    return sorted(set(cols))


def spike_rows(ny):
    return sorted({1, ny // 2, ny - 2})


def spike_state(nx, ny, seed, col, row, nan_in=None):
    """(p', rhs): random of magnitude <= SPIKE_NOISE with p' = 1 at (col, row),
    so the first sweep's largest |dp'| sits there; nan_in ("p_prime" / "rhs")
    also plants one NaN at an interior cell a quarter of the grid away."""
    rng = np.random.default_rng([nx, ny, seed])
    pp = rng.uniform(-SPIKE_NOISE, SPIKE_NOISE, nx * ny).astype(np.float32)
    rhs = rng.uniform(-SPIKE_NOISE, SPIKE_NOISE, nx * ny).astype(np.float32)
    pp[col + row * nx] = 1.0
    if nan_in is not None:
        i = 1 + (col + nx // 4) % (nx - 2)
        j = 1 + (row + ny // 4) % (ny - 2)
        assert (i, j) != (col, row)
        {"p_prime": pp, "rhs": rhs}[nan_in][i + j * nx] = np.nan
    return pp, rhs


# ---------------------------------------------------------------------------
# the resident solve's seam tests (test_gpu_resident_seams.py on the device,
# test_resident_seams_cpu.py for their premises with the oracle alone)

RES_T = 10               # sweeps per block of k_jacobi_resident between grid barriers
RES_LIMIT = 50           # jacobi_iters of the spike solves (the reference's default)
RES_BR, RES_BC = 8, 48   # the tile every small shape takes (asserted on the device)
# the small shapes: what each pins is listed in test_gpu_resident_seams.py
RES_SHAPES = [(16, 4), (48, 8), (16, 9), (24, 9), (56, 9), (104, 16), (96, 17), (120, 37),
              (16, 65), (16, 72), (16, 257)]
# the 800-wide grid whose 8 x 48 tiling no longer fits 256 CUs: 19-row tiles,
# 248 = 13 * 19 + 1 (asserted on the device through the geometry getter)
RES_WIDE = (800, 248)
RES_WIDE_BR, RES_WIDE_BC = 19, 46
RES_ITERS = (1, 2, 3, 9, 10, 11, 19, 50)   # Tb 1, 2, 3, both sides of a block, a ragged last block
RES_NAN_ITERS = 4
# exit sweeps the loose tolerances of the signs / range solves are built for
# (tol_exiting_at): the middle of the first block and of the second
RES_MID_EXITS = (4, 14)

# tolerances of the spike solves per (nx, ny, spacing): over the shape's spike
# states the reference's early exit falls on every sweep 1..10, on at least
# three sweeps of 11..49 and never (50 sweeps) -- exit_stages_missing(),
# asserted in test_resident_seams_cpu.py.  1e-4 is the reference's default.
RES_P_TOLS = {
    (16, 4, "pow2"): (0.025, 0.008, 0.006, 0.0012, 1e-4),
    (16, 4, "div"): (0.08, 0.02, 0.012, 0.006, 0.0015, 1e-4),
    (48, 8, "pow2"): (0.09, 0.01, 0.006, 0.005, 1e-4),
    (48, 8, "div"): (0.15, 0.09, 0.025, 0.01, 0.006, 1e-4),
    (16, 9, "pow2"): (0.09, 0.01, 0.006, 0.005, 1e-4),
    (16, 9, "div"): (0.12, 0.015, 0.012, 0.009, 0.006, 1e-4),
    (24, 9, "pow2"): (0.09, 0.01, 0.006, 0.005, 1e-4),
    (24, 9, "div"): (0.07, 0.008, 0.005, 1e-4),
    (56, 9, "pow2"): (0.09, 0.01, 0.006, 0.005, 1e-4),
    (56, 9, "div"): (0.15, 0.09, 0.025, 0.01, 0.006, 1e-4),
    (104, 16, "pow2"): (0.08, 0.01, 0.006, 0.005, 1e-4),
    (104, 16, "div"): (0.03, 0.01, 0.0012, 1e-4),
    (96, 17, "pow2"): (0.08, 0.01, 0.006, 0.005, 1e-4),
    (96, 17, "div"): (0.09, 0.025, 0.009, 0.0012, 1e-4),
    (120, 37, "pow2"): (0.08, 0.01, 0.006, 0.005, 1e-4),
    (120, 37, "div"): (0.1, 0.007, 1e-4, 6e-5),
    (16, 65, "pow2"): (0.09, 0.01, 0.006, 0.005, 1e-4),
    (16, 65, "div"): (0.015, 0.01, 0.0012, 1e-4),
    (16, 72, "pow2"): (0.09, 0.01, 0.006, 0.005, 1e-4),
    (16, 72, "div"): (0.015, 0.01, 0.001, 1e-4),
    (16, 257, "pow2"): (0.09, 0.01, 0.006, 0.005, 1e-4),
    (16, 257, "div"): (0.1, 0.015, 0.012, 0.0012, 1e-4, 3e-5),
}
# The wide grid is no exit-stage shape: a solve of its 198 K cells costs the
# oracle what a hundred of the small shapes' do, so it takes four spike cells
# (a corner of the first tile seams, the last swept row) and three tolerances
# (an exit in the first block, in a later one, and the default)
RES_WIDE_P_TOLS = (0.01, 0.002, 1e-4)
RES_WIDE_SPIKES = ((45, 18), (46, 19), (1, 246), (798, 246))


def resident_spike_columns(nx, bc=RES_BC):
    """spike_columns() plus both sides of the first two seams between tile
    columns (47, 48, 95, 96 for 48-column tiles), where the grid has them."""
    seams = list(range(bc, nx, bc))[:2]
    return sorted(set(spike_columns(nx)) | {c for s in seams for c in (s - 1, s) if c <= nx - 2})


def resident_spike_rows(ny, br=RES_BR):
    """First swept row, both sides of the first tile-row seam, and the last
    two swept rows, where the grid has them."""
    return sorted({r for r in (1, br - 1, br, ny - 3, ny - 2) if 1 <= r <= ny - 2})


def jacobi_history(nx, ny, kind, pp, rhs, iters=RES_LIMIT):
    """(fields, residuals) of the oracle's Jacobi sweep by sweep: fields[k] is
    p' after k sweeps (fields[0] the input), residuals[k] the residual of
    sweep k (residuals[0] is None).  One-sweep solves chained: a sweep reads
    nothing but p' and rhs."""
    from oracle import OracleModel
    lx, ly = spacing(nx, ny, kind)
    o = OracleModel(nx, ny, lx, ly, jacobi_iters=1, tol_enabled=0)
    o.field("p_prime")[:] = pp
    o.field("rhs")[:] = rhs
    fields, res = [np.array(pp, np.float32)], [None]
    for _ in range(iters):
        res.append(np.float32(o.jacobi()))
        fields.append(o.field("p_prime").copy())
    return fields, res


def exit_sweep(res, p_tol, iters=RES_LIMIT):
    """Sweeps a tolerance-mode solve of at most `iters` runs (model.rs:816),
    from jacobi_history's residuals."""
    for k in range(1, iters + 1):
        if res[k] < np.float32(p_tol):
            return k
    return iters


def tol_exiting_at(res, k):
    """A tolerance under which the solve exits at sweep k exactly: half-way
    between residual k and the smallest residual before it (None where
    residual k is not below all of them)."""
    before = min(res[1:k])
    if not res[k] < before:
        return None
    tol = np.float32(0.5 * (float(res[k]) + float(before)))
    return float(tol) if res[k] < tol <= before else None


def exit_stages_missing(exits, T=RES_T, limit=RES_LIMIT):
    """What a set of exit sweeps lacks of: every sweep of the first block
    (every j, j = T-1 with no re-run included), three stages of a later block,
    and the limit.  Empty when complete."""
    missing = [k for k in range(1, T + 1) if k not in exits]
    if len([e for e in exits if T < e < limit]) < 3:
        missing.append("three of %d..%d" % (T + 1, limit - 1))
    if limit not in exits:
        missing.append(limit)
    return missing


def stale_row_indistinct(fields, n, nx, ny):
    """The earlier sweeps (of n-1, n-2) whose row ny-2 equals sweep n's in
    every column 1..nx-2, bit for bit: a row ny-1 copied from such a sweep
    could not be told from the right one.  Empty where a stale copy shows."""
    def row(k):
        return bits(fields[k].reshape(ny, nx)[ny - 2, 1:nx - 1])
    return [k for k in (n - 1, n - 2) if k >= 0 and np.array_equal(row(k), row(n))]


# whole steps with the tolerance on: (nx, ny, spacing, cylinder)
RES_STEP_CASES = {
    "24x9": (24, 9, "pow2", None),
    "96x17": (96, 17, "pow2", None),
    "16x65": (16, 65, "pow2", None),
    "96x17-cylinder": (96, 17, "div", (7.5, 5.0, 0.75)),
}


# p_tol of the whole steps: the default, under which every solve of these
# states runs its 50 sweeps and every pass runs, and a loose one under which
# the corrector loop ends early within two steps (test_resident_seams_cpu.py)
RES_STEP_LOOSE = {"24x9": 0.01, "96x17": 0.01, "16x65": 0.01, "96x17-cylinder": 0.03}


def resident_step_case(name):
    """(grid, params) of a whole-step case: the lid-driven cavity on the
    power-of-two spacing, the channel with a cylinder on the 30 x 10 domain."""
    nx, ny, kind, cyl = RES_STEP_CASES[name]
    lx, ly = spacing(nx, ny, kind)
    g = dict(nx=nx, ny=ny, lx=lx, ly=ly)
    if cyl:
        return dict(g, cylinder=cyl), dict()
    return g, dict(bc_kind=1, viscosity=0.01)


def seam_nan_cells(nx, ny, br=RES_BR, bc=RES_BC):
    """(col, row) beside the first tile seams: rows br-1 and br at a middle
    column, columns bc-1 and bc at a middle row, where the grid has the seam
    and the cell is swept."""
    out = []
    if ny > br:
        out +=[(min(nx // 2, nx - 2), r) for r in (br - 1, br) if r <= ny - 2]
    if nx - 1 > bc:
        out += [(c, min(max(ny // 2, 1), ny - 2)) for c in (bc - 1, bc)]
    return out


# planted-NaN shapes: every small shape with a tile seam whose spoilt share
# stays under the suite's cap of 0.20 (test_resident_seams_cpu.py).  16 x 9 has
# the seam but not the room: a NaN at (8, 7) reaches 34 of its 144 cells in 4
# sweeps, so it has no NaN flavour.
RES_NAN_SHAPES = [s for s in RES_SHAPES if seam_nan_cells(*s) and s != (16, 9)]


def seam_nan_state(nx, ny, cell, nan_in):
    """(p', rhs) of adversarial_state's `signs` with one NaN at cell (col, row)."""
    st = adversarial_state(nx, ny, 1, "signs")
    pp, rhs = st["p_prime"].copy(), st["rhs"].copy()
    {"p_prime": pp, "rhs": rhs}[nan_in][cell[0] + cell[1] * nx] = np.nan
    return pp, rhs


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (n if n > 0 else 1.0))
