"""Restatement of the JavaScript variant's Jacobi branch (index.html:796-838),
its default pressure solver, for CFD_SOLVER_JACOBI_SCRIPT (pressure_solver 5).

Arithmetic as the script: every expression in IEEE double in the script's
order, every store rounded to f32 (the arrays are Float32Array); p' starts at
0; per iteration the interior takes
    0.7 * ((E + W)/(dx*dx) + (N + S)/(dy*dy) - rhs) / denom + (1 - 0.7) * old
from the previous iterate, maxError = max |new - old| over the interior on the
stored values (a NaN never enters, as the script's `>`), then rows 0 / ny-1 take
rows 1 / ny-2 and column 0 takes column 1, column nx-1 is 0, corners included
(:828-835).  Element-wise f64 numpy is IEEE-exact, so this equals the script's
loops bit for bit (tests/golden/make_js_jacobi_golden.py asserts it against
node).

The early exit follows the library (include/cfd.h): (float)maxError is compared
with the float p_tol.  The script compares the doubles; `slivers` lists the
iterations where the two comparisons differ (none on any committed fixture).

Returns (p' as f32 [ny, nx], iterations run, maxError list as f64)."""
import numpy as np

OMEGA = 0.7
P_TOL = 1e-6   # the script's pressureTolerance for this branch (:800)


def consts(dx, dy):
    dx, dy = float(np.float32(dx)), float(np.float32(dy))
    dx2, dy2 = dx * dx, dy * dy
    return dx2, dy2, 2 / dx2 + 2 / dy2


def _below(max_error, p_tol):
    return np.float32(max_error) < np.float32(p_tol)


def slivers(max_errors, p_tol=P_TOL):
    """Iterations whose double and float exit tests disagree."""
    return [k for k, e in enumerate(max_errors) if (e < float(p_tol)) != bool(_below(e, p_tol))]


def jacobi_script(rhs, nx, ny, dx, dy, iters, tol_enabled=True, p_tol=P_TOL):
    dx2, dy2, denom = consts(dx, dy)
    R = np.asarray(rhs, np.float32).reshape(ny, nx).astype(np.float64)[1:-1, 1:-1]
    P = np.zeros((ny, nx), np.float32)
    errs = []
    with np.errstate(all="ignore"):
        for _ in range(iters):
            D = P.astype(np.float64)
            old = D[1:-1, 1:-1]
            p_update = ((D[1:-1, 2:] + D[1:-1, :-2]) / dx2 + (D[2:, 1:-1] + D[:-2, 1:-1]) / dy2 - R) / denom
            new = (OMEGA * p_update + (1 - OMEGA) * old).astype(np.float32)
            err = np.abs(new.astype(np.float64) - old)
            err = err[err > 0.0]                      # NaN never enters, as `>` in the script
            max_error = float(err.max()) if err.size else 0.0
            P[1:-1, 1:-1] = new
            P[0, :] = P[1, :]
            P[-1, :] = P[-2, :]
            P[:, 0] = P[:, 1]
            P[:, -1] = 0.0
            errs.append(max_error)
            if tol_enabled and _below(max_error, p_tol):
                break
    return P, len(errs), errs
