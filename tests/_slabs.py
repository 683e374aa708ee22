"""Row slabs of one grid in one process over cfdamd.LocalHub (test
infrastructure only): the slab plan's boundaries, a single-domain state cut
into slabs and put back together, and the thread-per-rank runner the slab
tests share."""
import os
import threading
import time

import numpy as np

from _util import assert_bitwise

FIELD_KEYS = ("u", "v", "p", "u_star", "v_star", "p_prime", "rhs")
SCALAR_KEYS = ("dt", "simulation_time", "simulation_step", "last_p_residual", "last_u_residual",
               "last_v_residual", "jacobi_sweeps_total")
# seconds the other ranks get to return after one rank has raised (they wait
# for it at a hub barrier and never will)
GRACE_AFTER_ERROR = 2.0


def slab_bounds(ny, n):
    """j0 of ranks 1..n-1 (cfd_plan_slab, host only): the n-1 slab boundaries."""
    import ctypes as C
    import cfdamd
    L = cfdamd.load()
    j0, j1 = C.c_uint64(), C.c_uint64()
    out = []
    for r in range(1, n):
        rc = L.cfd_plan_slab(ny, n, r, C.byref(j0), C.byref(j1))
        assert rc == 0, (ny, n, r, rc)
        out.append(int(j0.value))
    return out


def boundary_rows(ny, n):
    """The rows either side of every slab boundary: j0-1 and j0."""
    return sorted({b + d for b in slab_bounds(ny, n) for d in (-1, 0)})


def _slab_slices(st, nx, j0, j1):
    """Rows [j0, j1) of a single-domain state (v and v* with the face row j1),
    and its scalars, as Model.set_state takes them; keys `st` lacks are left out."""
    out = {}
    for k in ("u", "u_star"):
        if k in st:
            out[k] = st[k].reshape(-1, nx + 1)[j0:j1].ravel().copy()
    for k in ("v", "v_star"):
        if k in st:
            out[k] = st[k].reshape(-1, nx)[j0:j1 + 1].ravel().copy()
    for k in ("p", "p_prime", "rhs"):
        if k in st:
            out[k] = st[k].reshape(-1, nx)[j0:j1].ravel().copy()
    for k in SCALAR_KEYS:
        if k in st:
            out[k] = st[k]
    return out


def assemble(states, nx, nan_equal=False):
    """Owned rows of every slab -> global flat arrays (v gets the top face
    from the last slab).  nan_equal: as assert_bitwise's, for the face row
    two neighbours share."""
    out = {}
    for f in ("u", "p", "p_prime", "u_star", "rhs"):
        out[f] = np.concatenate([s[f] for (_, _, s, _) in states])
    for f in ("v", "v_star"):
        parts = []
        for k, (j0, j1, s, _) in enumerate(states):
            rows = s[f].reshape(j1 - j0 + 1, nx)
            parts.append(rows if k == len(states) - 1 else rows[:-1])
            if k < len(states) - 1:
                # the shared face row is held (and computed) by both ranks
                nxt = states[k + 1][2][f].reshape(-1, nx)[0]
                assert_bitwise(f"{f} shared face row {j1}", rows[-1], nxt, nan_equal=nan_equal)
        out[f] = np.concatenate(parts).ravel()
    return out


def snapshot(m):
    """(j0, j1, state, halo depth) of one slab, as assemble() takes them."""
    return (m.j0, m.j1, m.get_state(), m.halo_depth)


def run_slabs(n, grid, params, state, halo_depth, fn, join=900.0):
    """n LocalHub slabs of `grid`, one thread per rank.  Every rank creates its
    model (CFD_HALO_DEPTH = halo_depth, or the library's default depth when
    None), injects its rows of the single-domain `state` when one is given
    (cfd_set_state, collective: it exchanges the ghosts), runs fn(model, rank)
    and synchronizes; returns [fn's value per rank].  Collective calls
    (update, pressure_solve, set_state, render) must be made by every rank's
    fn in the same order.  The first exception of any rank is raised here; a
    rank that has not returned `join` seconds in (or soon after another one
    raised, which leaves it at a hub barrier for good) fails the call too."""
    import cfdamd
    prev = os.environ.get("CFD_HALO_DEPTH")
    if halo_depth is None:
        os.environ.pop("CFD_HALO_DEPTH", None)
    else:
        os.environ["CFD_HALO_DEPTH"] = str(halo_depth)
    hub = cfdamd.LocalHub(n)
    out, models, errors = [None] * n, [None] * n, []

    def worker(r):
        try:
            m = cfdamd.Model(grid, params, device=0, n_ranks=n, rank=r, local_hub=hub)
            models[r] = m
            if state is not None:
                m.set_state(**_slab_slices(state, grid.nx, m.j0, m.j1))
            out[r] = fn(m, r)
            m.synchronize()
        except BaseException as e:   # surfaced below
            errors.append((r, e))

    ts = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(n)]
    try:
        for t in ts:
            t.start()
        t0 = time.monotonic()
        t_err = None
        while any(t.is_alive() for t in ts):
            for t in ts:
                t.join(0.02)
            now = time.monotonic()
            if errors and t_err is None:
                t_err = now
            if now - t0 > join or (t_err is not None and now - t_err > GRACE_AFTER_ERROR):
                break
    finally:
        if prev is None:
            os.environ.pop("CFD_HALO_DEPTH", None)
        else:
            os.environ["CFD_HALO_DEPTH"] = prev
    stuck = [r for r, t in enumerate(ts) if t.is_alive()]
    if not stuck:   # a rank still inside the library keeps its model and the hub
        for m in models:
            if m is not None:
                m.close()
        hub.close()
    if errors:
        raise errors[0][1]
    assert not stuck, f"ranks {stuck} of {n} did not return within {join} s"
    return out


def run_sharded_from_state(n, grid, params, state, steps):
    """LocalHub slabs started from a single-domain state, `steps` steps on:
    [(j0, j1, state, halo depth)] per rank."""
    def fn(m, r):
        m.update_n(steps)
        m.synchronize()
        return snapshot(m)
    return run_slabs(n, grid, params, state, None, fn)


# ---------------------------------------------------------------------------
# Cases of test_gpu_slabs_adversarial.py, shared with the oracle-only premises
# in test_slabs_adversarial_cpu.py.

P2 = 1.0 / 128.0        # dx = dy = 2^-7, as test_gpu_adversarial.py
CAVITY_KW = dict(bc_kind=1, viscosity=0.01)
CYL128 = dict(nx=128, ny=60, lx=30.0, ly=10.0, cylinder=(7.5, 5.0, 1.9))
CYL248 = dict(nx=248, ny=301, lx=8.0, ly=10.0, cylinder=(4.0, 5.0, 1.0))
MAX_NONFINITE_SHARE = 0.20


def pow2_grid(nx, ny):
    return dict(nx=nx, ny=ny, lx=nx * P2, ly=ny * P2)


def grid_of(name):
    """(grid dict, parameters every case on it shares) of a layout's grid."""
    if name == "128x60":
        return CYL128, {}
    if name == "248x301":
        return CYL248, {}
    nx, ny = (int(x) for x in name.split("x"))
    return pow2_grid(nx, ny), dict(CAVITY_KW)


# (grid, ranks, CFD_HALO_DEPTH or None, the depth every rank must report, inlet profile)
STEP_LAYOUTS = [
    ("16x8", 2, None, 2, 0),      # 4-row slabs: the minimum; no async u/v exchange
    ("112x18", 2, 3, 3, 0),       # odd 9-row slabs: the march's edge launches overlap its interior
    ("112x18", 4, 8, 2, 0),       # 5/5/4/4 rows, the depth clamped
    ("120x37", 3, 1, 1, 0),       # 13/12/12 rows, an exchange every sweep
    ("120x37", 2, 8, 8, 0),       # 19/18 rows, 8 + 1 sweep blocks, overlapped bands
    ("248x31", 4, 5, 5, 0),       # 8/8/8/7 rows: the ranks differ in the async u/v exchange
    ("1032x16", 2, 6, 6, 0),      # 8-row slabs, two chunks of the vector correctors
    ("128x60", 2, 4, 4, 0), ("128x60", 2, 4, 4, 1),
    ("128x60", 3, 4, 4, 0), ("128x60", 3, 4, 4, 1),
    ("248x301", 4, None, 8, 0),   # the default depth, kind-4 Jacobi on slabs
]
# row counts of the slabs, as the comments above claim them
STEP_ROWS = {("16x8", 2): [4, 4], ("112x18", 2): [9, 9], ("112x18", 4): [5, 5, 4, 4],
             ("120x37", 3): [13, 12, 12], ("120x37", 2): [19, 18], ("248x31", 4): [8, 8, 8, 7],
             ("1032x16", 2): [8, 8], ("128x60", 2): [30, 30], ("128x60", 3): [20, 20, 20],
             ("248x301", 4): [76, 75, 75, 75]}


def layout_id(layout):
    name, n, depth, _, profile = layout
    return f"{name}-n{n}-d{'default' if depth is None else depth}-inlet{profile}"


def step_cases():
    """(layout, flavour): `signs` and `range` on every layout, `nonfinite` on
    grids of at least 1000 cells."""
    out = []
    for lay in STEP_LAYOUTS:
        g, _ = grid_of(lay[0])
        for flavour in ("signs", "range", "nonfinite"):
            if flavour != "nonfinite" or g["nx"] * g["ny"] >= 1000:
                out.append((lay, flavour))
    return out


def step_kw(layout, flavour, scheme, passes):
    """Parameters of a 2a step: tolerance off, 9 sweeps (3 from `nonfinite`)."""
    _, kw = grid_of(layout[0])
    kw.update(scheme=scheme, corrector_passes=passes, tol_enabled=0,
              jacobi_iters=3 if flavour == "nonfinite" else 9, inlet_profile=layout[4])
    return kw


def step_count(flavour):
    return 1 if flavour == "nonfinite" else 2


def clean_ranks(o, nx, ny, n):
    """Ranks whose slab (owned rows, v and v* with the shared face row) holds
    no non-finite word in any field of the OracleModel `o`."""
    edges = [0] + slab_bounds(ny, n) + [ny]
    out = []
    for r in range(n):
        bad = 0
        for f in ("u", "v", "u_star", "v_star", "p", "p_prime", "rhs"):
            pitch = nx + 1 if f in ("u", "u_star") else nx
            hi = edges[r + 1] + (1 if f in ("v", "v_star") else 0)
            bad += np.count_nonzero(~np.isfinite(o.field(f).reshape(-1, pitch)[edges[r]:hi]))
        if not bad:
            out.append(r)
    return out


def has_clean_rank(layout, scheme, passes):
    """Whether, on the oracle, a `nonfinite` step of this layout leaves some
    slab without a non-finite word (that rank must report CFD_ENONFINITE all
    the same).  112 x 18 has one planted word (u at row 5): with no corrector
    pass it stays below row 10, clear of ranks 2 and 3 of 4.  128 x 60 on 3
    ranks plants rows 15 and 45, which the first-order scheme without passes
    keeps out of rows 20 .. 39.  Everywhere else every slab holds a planted
    word or is reached from one: the five words of 248 x 301 lie on rows 30,
    90, 150, 210 and 270, one or two in each of its four slabs.
    (test_slabs_adversarial_cpu.py checks this table against the oracle.)"""
    name, n = layout[0], layout[1]
    return ((name, n) == ("112x18", 4) and passes == 0) or \
           ((name, n) == ("128x60", 3) and scheme == 0 and passes == 0)


# 2b / 2c: the three forms of the tolerance mode on 120 x 37
# (name, ranks, CFD_HALO_DEPTH, CFD_SPEC_SLABS or None)
TOL_GRID = "120x37"
TOL_FORMS = [("spec", 2, 8, None), ("host-env", 2, 8, "0"), ("host-geometry", 3, 2, None)]
TOL_KW = dict(CAVITY_KW, jacobi_iters=50, corrector_passes=2, tol_enabled=1)
TOL_STEP_SWEEPS = 150    # three 50-sweep solves: none exits early on the oracle

# 2c: (name, ranks, CFD_HALO_DEPTH) of the fixed-count residual solves
FIXED_FORMS = [("n2-d8", 2, 8), ("n3-d2", 3, 2)]
FIXED_SWEEPS = (1, 8, 9, 17)


def tol_spikes(nx, ny, n):
    """The trimmed (column, row) product of the tolerance-mode spike solves:
    the last included and the first excluded column of the residual and both
    sides of the 112-column seam, on the two rows of the first slab boundary
    and on the last swept row."""
    b = slab_bounds(ny, n)[0]
    return [(c, r) for c in (nx - 8, nx - 7, 112, 113) for r in (b - 1, b, ny - 2)]


def fixed_spikes(nx, ny, n):
    """Every spike column on the single-domain rows and the boundary rows."""
    from _util import spike_columns, spike_rows
    rows = sorted(set(spike_rows(ny)) | set(boundary_rows(ny, n)))
    return [(c, r) for c in spike_columns(nx) for r in rows]


# 2d: SOR and multigrid. (grid, ranks, CFD_HALO_DEPTH, CFD_MG_PARTITION or None)
SOLVER_LAYOUTS = [("120x37", 2, 4, None), ("128x64", 4, 4, "1")]


def solver_kw(solver, passes):
    return dict(CAVITY_KW, pressure_solver=solver, corrector_passes=passes, jacobi_iters=9,
                tol_enabled=0)


def sor_refused(ny, n):
    """Whether the library refuses SOR on n slabs of ny rows: every slab needs
    16 interior rows (rows 0 and ny-1 are boundary rows, not swept)."""
    edges = [0] + slab_bounds(ny, n) + [ny]
    return any(min(b, ny - 1) - max(a, 1) < 16 for a, b in zip(edges, edges[1:]))


def adv_global_state(nx, ny, flavour, dt=None):
    """adversarial_state plus the scalars load_state gives the oracle, as one
    single-domain state dict for _slab_slices."""
    from _util import ADV_STEP, adversarial_state
    st = dict(adversarial_state(nx, ny, 1, flavour))
    st.update(simulation_step=ADV_STEP, simulation_time=np.float32(ADV_STEP) * np.float32(0.005),
              jacobi_sweeps_total=0)
    if dt is not None:
        st["dt"] = np.float32(dt)
    return st
