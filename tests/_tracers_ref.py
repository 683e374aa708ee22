"""Restatement of the JavaScript variant's tracer particles
(index.html:1472-1543 and the cadence of simulationLoop, :1231-1238), for the
cfd_tracers_* entry points.

Arithmetic as the script: every expression in IEEE double; u and v are the
script's Float32Arrays widened on load; dx, dy, Lx, Ly and dt are the f32
values of the model widened to double.  Element-wise float64 numpy rounds every
operation separately, so the vectorised form equals the script's per-tracer
loop bit for bit (tests/golden/js_tracers_*.npz pin it to the script's own
output under node).

A tracer list is the tuple (x, y, initial_y) of float64 arrays in list order.
"""
import numpy as np


class Domain:
    """Grid constants as the library forms them: f32 lx / nx, widened."""

    def __init__(self, nx, ny, lx, ly):
        self.nx, self.ny = int(nx), int(ny)
        self.lx, self.ly = float(np.float32(lx)), float(np.float32(ly))
        self.dx = float(np.float32(lx) / np.float32(nx))
        self.dy = float(np.float32(ly) / np.float32(ny))


def empty():
    return tuple(np.empty(0, np.float64) for _ in range(3))


def inject(dom, tr):
    """injectTracers (:1537-1543): ny tracers appended."""
    y = (np.arange(dom.ny, dtype=np.float64) + 0.5) * dom.dy
    return (np.concatenate([tr[0], np.zeros(dom.ny)]), np.concatenate([tr[1], y]),
            np.concatenate([tr[2], y]))


def init(dom):
    """initTracers (:1475-1483)."""
    return inject(dom, empty())


def cell_index(dom, x, y, clamps=None):
    """i, j of getVelocityAt (:1502-1507) as doubles; clamps: a 4-list that
    counts the evaluations each clamp changed (i < 0, i > Nx-2, j < 0, j > Ny-2)."""
    with np.errstate(over="ignore", invalid="ignore"):
        i = np.floor(x / dom.dx)
        j = np.floor(y / dom.dy)
    hit = [i < 0, i > dom.nx - 2, j < 0, j > dom.ny - 2]
    if clamps is not None:
        for k in range(4):
            clamps[k] += int(np.count_nonzero(hit[k]))
    i = np.where(hit[0], 0.0, i)
    i = np.where(i > dom.nx - 2, float(dom.nx - 2), i)
    j = np.where(hit[2], 0.0, j)
    j = np.where(j > dom.ny - 2, float(dom.ny - 2), j)
    return i, j


def velocity_at(dom, u, v, x, y, clamps=None):
    """getVelocityAt (:1499-1525) for arrays of finite positions."""
    nx = dom.nx
    U = np.asarray(u, np.float32).reshape(-1).astype(np.float64)
    V = np.asarray(v, np.float32).reshape(-1).astype(np.float64)
    i, j = cell_index(dom, x, y, clamps)
    with np.errstate(over="ignore", invalid="ignore"):
        rx = (x - i * dom.dx) / dom.dx
        ry = (y - j * dom.dy) / dom.dy
        ii, jj = i.astype(np.int64), j.astype(np.int64)

        def centre(a, b):   # cellCenterVelocity (:1512-1516)
            cu = 0.5 * (U[a + b * (nx + 1)] + U[(a + 1) + b * (nx + 1)])
            cv = 0.5 * (V[a + b * nx] + V[a + (b + 1) * nx])
            return cu, cv

        u00, v00 = centre(ii, jj)
        u10, v10 = centre(ii + 1, jj)
        u01, v01 = centre(ii, jj + 1)
        u11, v11 = centre(ii + 1, jj + 1)
        ui = (1 - rx) * ((1 - ry) * u00 + ry * u01) + rx * ((1 - ry) * u10 + ry * u11)
        vi = (1 - rx) * ((1 - ry) * v00 + ry * v01) + rx * ((1 - ry) * v10 + ry * v11)
    return ui, vi


def keep_mask(dom, x, y):
    """updateTracers' test (:1492); NaN fails every comparison."""
    with np.errstate(invalid="ignore"):
        return (x >= 0) & (x <= dom.lx) & (y >= 0) & (y <= dom.ly)


def advance(dom, u, v, dt, tr, clamps=None, exits=None):
    """updateTracers(dt) (:1485-1497).  exits: a 4-list that counts the tracers
    that left through x < 0, x > Lx, y < 0, y > Ly."""
    x, y, iy = tr
    if x.size == 0:
        return empty()
    dt = float(dt)
    ui, vi = velocity_at(dom, u, v, x, y, clamps)
    with np.errstate(over="ignore", invalid="ignore"):
        x = x + dt * ui
        y = y + dt * vi
    if exits is not None:
        with np.errstate(invalid="ignore"):
            for k, c in enumerate((x < 0, x > dom.lx, y < 0, y > dom.ly)):
                exits[k] += int(np.count_nonzero(c))
    keep = keep_mask(dom, x, y)
    return x[keep], y[keep], iy[keep]


def step(dom, u, v, dt, step_count, interval, tr, **kw):
    """The tracer part of simulationLoop (:1233-1238) after a step that left
    velocities u, v, the next step's dt and simulationStepCount == step_count."""
    tr = advance(dom, u, v, dt, tr, **kw)
    if step_count % interval == 0:
        tr = inject(dom, tr)
    return tr


def density(dom, tr):
    """cfd_tracers_density: tracers per pressure cell, (ny, nx) uint32, the cell
    floor(x/dx), floor(y/dy) clipped to the grid."""
    x, y, _ = tr
    i = np.clip(np.floor(x / dom.dx), 0, dom.nx - 1)
    j = np.clip(np.floor(y / dom.dy), 0, dom.ny - 1)
    h, _, _ = np.histogram2d(j, i, bins=(dom.ny, dom.nx), range=((-0.5, dom.ny - 0.5), (-0.5, dom.nx - 0.5)))
    return h.astype(np.uint32)


def bits_equal(a, b):
    """Two tracer lists equal in length, order and every bit."""
    return all(p.shape == q.shape and np.array_equal(p.view(np.uint64), q.view(np.uint64))
               for p, q in zip(a, b))
