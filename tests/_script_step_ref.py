"""numpy restatement of the script's substep (index.html:366-867 pisoStep and
:870-930 applyBoundaryConditions) around its pressure solve: the predictor
pass (u*, v*, rhs), the corrector pass (u, v, p += p', boundary conditions),
and the host data both need (obstacle faces, inlet column).

Arithmetic is the script's: float64 on float32 arrays widened, one rounding to
float32 per stored value (a Float32Array store), every guard and quirk as
written.  Indices are the script's flat ones, so v[idx+2] at i = nx-2 reads the
next row's first value as the script does.  Values a guard does not select are
computed and dropped (np.where), never read out of bounds (indices are clipped;
a clipped index is never selected).

`counters`, when a dict is passed, counts per branch how many faces took it:
  {u,v}_{e,w,n,s}_{pos,neg}        each upwind side of each face
  {u,v}_{e,w,n,s}_{pos,neg}_fb     the guarded fallback of that side (only the
                                   schemes and sides that have a reachable one)
  {u,v}_obstacle                   a visited face inside the cylinder
  {u,v}_sel_zero, {u,v}_sel_negzero  a selector that is exactly +0 / -0
tests/golden/make_js_script_step_golden.py asserts this file equal to node bit
for bit; tests/test_script_step_cpu.py pins it to the committed fixtures.
"""
import numpy as np

FIRST, SECOND, QUICK = 0, 1, 2
SCHEME_NAMES = {FIRST: "first", SECOND: "second", QUICK: "quick"}
UNIFORM, PARABOLIC = 0, 1
PROFILE_NAMES = {UNIFORM: "uniform", PARABOLIC: "parabolic"}


class Grid:
    """The script's globals as the library forms them: f32 values widened."""

    def __init__(self, nx, ny, lx, ly, nu, cyl=None):
        self.nx, self.ny = int(nx), int(ny)
        self.lx, self.ly = float(np.float32(lx)), float(np.float32(ly))
        # dx = lx / nx in f32 (src/app.rs:37-38), then widened
        self.dx = float(np.float32(lx) / np.float32(nx))
        self.dy = float(np.float32(ly) / np.float32(ny))
        self.nu = float(np.float32(nu))
        # (x, y, radius) as f32 widened, or None: no face is an obstacle
        self.cyl = None if cyl is None else tuple(float(np.float32(c)) for c in cyl)


def _f32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a, np.float64).astype(np.float32)


# ---- obstacle faces and inlet column (host data) ----
def in_obstacle(g, x, y):
    """isPointInObstacle (:212-215); x**2 is x*x (asserted against node)."""
    if g.cyl is None:
        return np.zeros(np.broadcast(x, y).shape, bool)
    cx, cy, r = g.cyl
    ex, ey = x - cx, y - cy
    return np.sqrt(ex * ex + ey * ey) <= r


def obstacle_faces(g):
    """Per-face evaluation: u faces (ny, nx+1) at (i dx, (j+1/2) dy), v faces
    (ny+1, nx) at ((i+1/2) dx, j dy)."""
    iu = np.arange(g.nx + 1, dtype=np.float64)[None, :]
    ju = np.arange(g.ny, dtype=np.float64)[:, None]
    ou = in_obstacle(g, iu * g.dx, (ju + 0.5) * g.dy)
    iv = np.arange(g.nx, dtype=np.float64)[None, :]
    jv = np.arange(g.ny + 1, dtype=np.float64)[:, None]
    ov = in_obstacle(g, (iv + 0.5) * g.dx, jv * g.dy)
    return ou, ov


def obstacle_intervals(mask):
    """The library's form: per row the half-open column interval [lo, hi) of
    the obstacle faces (lo == hi == 0: none).  Raises if a row is not one
    interval."""
    out = np.zeros((mask.shape[0], 2), np.int32)
    for j, row in enumerate(mask):
        k = np.flatnonzero(row)
        if k.size:
            if k[-1] - k[0] + 1 != k.size:
                raise ValueError(f"row {j}: obstacle faces are not one interval")
            out[j] = (k[0], k[-1] + 1)
    return out


def intervals_to_mask(iv, width):
    cols = np.arange(width)[None, :]
    return (cols >= iv[:, :1]) & (cols < iv[:, 1:])


def inlet_column(g, inlet_velocity, profile):
    """The ny values applyBoundaryConditions stores into u[0, j] (:873-885)."""
    iv = float(inlet_velocity)
    y = (np.arange(g.ny, dtype=np.float64) + 0.5) * g.dy
    if profile == PARABOLIC:
        center = g.ly / 2
        radius = g.ly / 2
        t = (y - center) / radius
        val = iv * (1 - t * t)
        val = np.where(val > 0, val, np.where(np.isnan(val), val, 0.0))   # Math.max(val, 0)
    else:
        val = np.full(g.ny, iv)
    return _f32(val)


# ---- predictor ----
def _hit(counters, name, mask):
    if counters is not None:
        counters[name] = counters.get(name, 0) + int(np.count_nonzero(mask))


def _sel(counters, f, face, s, pos_val, neg_val, live, pos_fb=None, neg_fb=None):
    """value = (s >= 0) ? pos_val : neg_val, counting the sides over `live`
    faces; *_fb: mask of faces whose side takes its guarded fallback."""
    pos = s >= 0
    _hit(counters, f"{f}_{face}_pos", pos & live)
    _hit(counters, f"{f}_{face}_neg", ~pos & live)
    if pos_fb is not None:
        _hit(counters, f"{f}_{face}_pos_fb", pos & pos_fb & live)
    if neg_fb is not None:
        _hit(counters, f"{f}_{face}_neg_fb", ~pos & neg_fb & live)
    zero = (s == 0) & live
    _hit(counters, f"{f}_sel_negzero", zero & np.signbit(s))
    _hit(counters, f"{f}_sel_zero", zero & ~np.signbit(s))
    return np.where(pos, pos_val, neg_val)


def predict(g, u, v, dt_sub, scheme, counters=None):
    """:368-739 -> u_star (ny, nx+1), v_star (ny+1, nx), rhs (ny, nx), f32."""
    nx, ny, dx, dy, nu = g.nx, g.ny, g.dx, g.dy, g.nu
    dt_sub = float(dt_sub)
    W = nx + 1
    uf = np.asarray(u, np.float32).reshape(-1).astype(np.float64)
    vf = np.asarray(v, np.float32).reshape(-1).astype(np.float64)
    assert uf.size == W * ny and vf.size == nx * (ny + 1)
    ou, ov = obstacle_faces(g)

    def U(idx):
        return uf[np.clip(idx, 0, uf.size - 1)]

    def V(idx):
        return vf[np.clip(idx, 0, vf.size - 1)]

    u_star = np.asarray(u, np.float32).reshape(ny, W).copy()
    v_star = np.asarray(v, np.float32).reshape(ny + 1, nx).copy()
    with np.errstate(all="ignore"):
        # ---- u: j in [1, ny-1), i in [1, nx) ----
        if ny > 2 and nx > 1:
            j, i = np.meshgrid(np.arange(1, ny - 1), np.arange(1, nx), indexing="ij")
            idx = i + j * W
            obst = ou[j, i]
            live = ~obst
            _hit(counters, "u_obstacle", obst)
            u0, ue, uw = U(idx), U(idx + 1), U(idx - 1)
            un, us = U(idx + W), U(idx - W)
            v_n = 0.5 * (V((i - 1) + (j + 1) * nx) + V(i + (j + 1) * nx))
            v_s = 0.5 * (V((i - 1) + j * nx) + V(i + j * nx))
            if scheme == FIRST:
                f_e = _sel(counters, "u", "e", 0.5 * (u0 + ue), u0, ue, live)
                f_w = _sel(counters, "u", "w", 0.5 * (uw + u0), uw, u0, live)
                f_n = _sel(counters, "u", "n", v_n, u0, un, live)
                f_s = _sel(counters, "u", "s", v_s, us, u0, live)
            elif scheme == SECOND:
                uee, uww = U(idx + 2), U(idx - 2)
                unn, uss = U(idx + 2 * W), U(idx - 2 * W)
                g_e = ((idx + 2) < uf.size) & (i < nx - 1)
                g_n = ((i + (j + 2) * W) < uf.size) & (j < ny - 1)
                f_e = _sel(counters, "u", "e", u0,
                           np.where(i > 1, 1.5 * u0 - 0.5 * uw, u0),
                           np.where(g_e, 1.5 * ue - 0.5 * uee, ue), live, i <= 1, ~g_e)
                f_w = _sel(counters, "u", "w", uw,
                           np.where(i > 2, 1.5 * uw - 0.5 * uww, uw),
                           np.where(i < nx, 1.5 * u0 - 0.5 * ue, u0), live, i <= 2)
                f_n = _sel(counters, "u", "n", v_n,
                           np.where(j > 1, 1.5 * u0 - 0.5 * us, u0),
                           np.where(g_n, 1.5 * un - 0.5 * unn, un), live, j <= 1, ~g_n)
                f_s = _sel(counters, "u", "s", v_s,
                           np.where(j > 1, 1.5 * us - 0.5 * uss, us),
                           np.where(j < ny, 1.5 * u0 - 0.5 * un, u0), live, j <= 1)
            else:
                uee, uww = U(idx + 2), U(idx - 2)
                unn, uss = U(idx + 2 * W), U(idx - 2 * W)
                f_e = _sel(counters, "u", "e", u0,
                           np.where(i >= 2, (-uw + 6 * u0 + 3 * ue) / 8, 1.5 * u0 - 0.5 * uw),
                           np.where(i <= nx - 2, (3 * u0 + 6 * ue - uee) / 8, ue),
                           live, i < 2, i > nx - 2)
                f_w = _sel(counters, "u", "w", uw,
                           np.where(i >= 3, (-uww + 6 * uw + 3 * u0) / 8, 1.5 * uw - 0.5 * u0),
                           (3 * uw + 6 * u0 - ue) / 8, live, i < 3)
                f_n = _sel(counters, "u", "n", v_n,
                           np.where(j >= 2, (-us + 6 * u0 + 3 * un) / 8, 1.5 * u0 - 0.5 * us),
                           np.where(j < ny - 2, (3 * u0 + 6 * un - unn) / 8, un),
                           live, j < 2, j >= ny - 2)
                f_s = _sel(counters, "u", "s", v_s,
                           np.where(j >= 2, (-uss + 6 * us + 3 * u0) / 8, 1.5 * us - 0.5 * u0),
                           np.where(j < ny - 1, (3 * us + 6 * u0 - un) / 8, u0), live, j < 2)
            F_e, F_w = f_e * f_e, f_w * f_w
            F_n, F_s = v_n * f_n, v_s * f_s
            conv = (F_e - F_w) / dx + (F_n - F_s) / dy
            lap = (ue - 2 * u0 + uw) / (dx * dx) + (un - 2 * u0 + us) / (dy * dy)
            val = u0 + dt_sub * (-conv + nu * lap)
            u_star[j, i] = _f32(np.where(obst, 0.0, val))
        # ---- v: j in [1, ny), i in [1, nx-1) ----
        if ny > 1 and nx > 2:
            j, i = np.meshgrid(np.arange(1, ny), np.arange(1, nx - 1), indexing="ij")
            idx = i + j * nx
            obst = ov[j, i]
            live = ~obst
            _hit(counters, "v_obstacle", obst)
            v0, ve, vw = V(idx), V(idx + 1), V(idx - 1)
            vn, vs = V(idx + nx), V(idx - nx)
            vee = V(idx + 2)   # flat: the next row's first value at i = nx-2
            u_e, u_w = U((i + 1) + j * W), U(i + j * W)
            vna, vsa = 0.5 * (v0 + vn), 0.5 * (vs + v0)
            if scheme == FIRST:
                f_e = _sel(counters, "v", "e", u_e, v0, ve, live)
                f_w = _sel(counters, "v", "w", u_w, vw, v0, live)
                f_n = _sel(counters, "v", "n", vna, v0, vn, live)
                f_s = _sel(counters, "v", "s", vsa, vs, v0, live)
                lap = (ve - 2 * v0 + vw) / (dx * dx) + (vn - 2 * v0 + vs) / (dy * dy)
            else:
                vww = V(idx - 2)
                vnn, vss = V(idx + 2 * nx), V(idx - 2 * nx)
                if scheme == SECOND:
                    g_e = ((idx + 2) < vf.size) & (i < nx - 2)
                    g_n = ((i + (j + 2) * nx) < vf.size) & (j < ny - 1)
                    f_e = _sel(counters, "v", "e", u_e,
                               np.where(i > 0, 1.5 * v0 - 0.5 * vw, v0),
                               np.where(g_e, 1.5 * ve - 0.5 * vee, ve), live, None, ~g_e)
                    f_w = _sel(counters, "v", "w", u_w,
                               np.where(i > 1, 1.5 * vw - 0.5 * vww, vw),
                               np.where(i < nx - 1, 1.5 * v0 - 0.5 * ve, v0), live, i <= 1)
                    f_n = _sel(counters, "v", "n", vna,
                               np.where(j > 1, 1.5 * v0 - 0.5 * vs, v0),
                               np.where(g_n, 1.5 * vn - 0.5 * vnn, vn), live, j <= 1, ~g_n)
                    f_s = _sel(counters, "v", "s", vsa,
                               np.where(j > 1, 1.5 * vs - 0.5 * vss, vs),
                               np.where(j < ny, 1.5 * v0 - 0.5 * vn, v0), live, j <= 1)
                else:
                    f_e = _sel(counters, "v", "e", u_e,
                               np.where(i >= 2, (-vw + 6 * v0 + 3 * ve) / 8, 1.5 * v0 - 0.5 * vw),
                               np.where(i < nx - 2, (3 * v0 + 6 * ve - vee) / 8, ve),
                               live, i < 2, i >= nx - 2)
                    f_w = _sel(counters, "v", "w", u_w,
                               np.where(i >= 3, (-vww + 6 * vw + 3 * v0) / 8, 1.5 * vw - 0.5 * v0),
                               (3 * vw + 6 * v0 - ve) / 8, live, i < 3)
                    f_n = _sel(counters, "v", "n", vna,
                               np.where(j >= 2, (-vs + 6 * v0 + 3 * vn) / 8, 1.5 * v0 - 0.5 * vs),
                               np.where(j < ny - 1, (3 * v0 + 6 * vn - vnn) / 8, vn),
                               live, j < 2, j >= ny - 1)
                    f_s = _sel(counters, "v", "s", vsa,
                               np.where(j >= 2, (-vss + 6 * vs + 3 * v0) / 8, 1.5 * vs - 0.5 * v0),
                               np.where(j < ny - 1, (3 * vs + 6 * v0 - vn) / 8, v0),
                               live, j < 2, j >= ny - 1)
                # the script's own y-Laplacian (:641, :721)
                lap = (ve - 2 * v0 + vw) / (dx * dx) + (vee - 2 * v0 + v0) / (dy * dy)
            F_e, F_w = u_e * f_e, u_w * f_w
            F_n, F_s = f_n * f_n, f_s * f_s
            conv = (F_e - F_w) / dx + (F_n - F_s) / dy
            val = v0 + dt_sub * (-conv + nu * lap)
            v_star[j, i] = _f32(np.where(obst, 0.0, val))
        us64, vs64 = u_star.astype(np.float64), v_star.astype(np.float64)
        div = (us64[:, 1:] - us64[:, :-1]) / dx + (vs64[1:, :] - vs64[:-1, :]) / dy
        rhs = _f32(div / dt_sub)
    return u_star, v_star, rhs


# ---- corrector + boundary conditions ----
def correct(g, u_star, v_star, p_prime, p, dt_sub, inlet_velocity, profile):
    """:842-866 and applyBoundaryConditions.  The u, v from before the substep
    are not an input: every face the corrector leaves alone (columns 0 and nx
    of u, rows 0 and ny of v) is rewritten by the boundary pass."""
    nx, ny, dx, dy = g.nx, g.ny, g.dx, g.dy
    dt_sub = float(dt_sub)
    us = np.asarray(u_star, np.float32).reshape(ny, nx + 1).astype(np.float64)
    vs = np.asarray(v_star, np.float32).reshape(ny + 1, nx).astype(np.float64)
    pp = np.asarray(p_prime, np.float32).reshape(ny, nx).astype(np.float64)
    p64 = np.asarray(p, np.float32).reshape(ny, nx).astype(np.float64)
    with np.errstate(all="ignore"):
        u = np.zeros((ny, nx + 1), np.float32)
        u[:, 1:nx] = _f32(us[:, 1:nx] - dt_sub * (pp[:, 1:] - pp[:, :-1]) / dx)
        v = np.zeros((ny + 1, nx), np.float32)
        v[1:ny, :] = _f32(vs[1:ny, :] - dt_sub * (pp[1:, :] - pp[:-1, :]) / dy)
        p_new = _f32(p64 + pp)
    u[:, 0] = inlet_column(g, inlet_velocity, profile)
    u[:, nx] = u[:, nx - 1]
    u[0, :] = 0
    u[ny - 1, :] = 0
    v[0, :] = 0
    v[ny, :] = 0
    ou, ov = obstacle_faces(g)
    u[ou] = 0
    v[ov] = 0
    return u, v, p_new


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def counter_names(scheme):
    """Every counter `predict` keeps for a scheme (by running it on a tiny grid)."""
    g = Grid(16, 5, 16.0, 5.0, 0.01)
    c = {}
    predict(g, np.zeros((5, 17), np.float32), np.zeros((6, 16), np.float32), 0.1, scheme, c)
    return sorted(c)
