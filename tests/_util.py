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


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (n if n > 0 else 1.0))
