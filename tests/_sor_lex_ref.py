"""Restatement of the JavaScript variant's SOR branch (index.html:743-774) in
the script's own order, for CFD_SOLVER_SOR_LEX (pressure_solver 4).

Arithmetic as the script: every expression in IEEE double, every store rounded
to f32 (the script's arrays are Float32Array); p' starts at 0; after each
iteration rows 0 / ny-1 take rows 1 / ny-2, then column 0 takes column 1 and
column nx-1 is 0, corners included (:761-770).

Two forms with identical results:
  sor_lex_loop  the plain loops, cell by cell (pinned to the script's own
                output by tests/golden/js_sor_*.npz);
  sor_lex_diag  the same updates an anti-diagonal at a time: cell (i, j) reads
                the new (i-1, j), (i, j-1) and the old (i+1, j), (i, j+1), so
                the cells with equal i + j are independent.  Element-wise f64
                numpy is IEEE-exact, so it equals the loop form bit for bit.

The early exit follows the library (include/cfd.h): (float)maxError is compared
with the float p_tol.  The script compares the doubles; `slivers` lists the
iterations where the two comparisons differ (none on any committed fixture).

Both return (p' as f32 [ny, nx], iterations run, maxError list as f64)."""
import numpy as np

OMEGA = 1.7


def consts(dx, dy):
    """dx2, dy2, denom as the script forms them from the f32 spacings
    (index.html:181-183)."""
    dx, dy = float(np.float32(dx)), float(np.float32(dy))
    dx2, dy2 = dx * dx, dy * dy
    return dx2, dy2, 2 / dx2 + 2 / dy2


def _bcs(P):
    P[0, :] = P[1, :]
    P[-1, :] = P[-2, :]
    P[:, 0] = P[:, 1]
    P[:, -1] = 0.0


def _below(max_error, p_tol):
    return np.float32(max_error) < np.float32(p_tol)


def slivers(max_errors, p_tol=1e-4):
    """Iterations whose double and float exit tests disagree."""
    return [k for k, e in enumerate(max_errors) if (e < float(p_tol)) != bool(_below(e, p_tol))]


def sor_lex_loop(rhs, nx, ny, dx, dy, iters, tol_enabled=True, p_tol=1e-4):
    dx2, dy2, denom = consts(dx, dy)
    R = np.asarray(rhs, np.float32).reshape(ny, nx)
    P = np.zeros((ny, nx), np.float32)
    errs = []
    for _ in range(iters):
        max_error = 0.0
        for j in range(1, ny - 1):
            for i in range(1, nx - 1):
                p_old = float(P[j, i])
                p_update = ((float(P[j, i + 1]) + float(P[j, i - 1])) / dx2 +
                            (float(P[j + 1, i]) + float(P[j - 1, i])) / dy2 - float(R[j, i])) / denom
                P[j, i] = (1 - OMEGA) * p_old + OMEGA * p_update
                error = abs(float(P[j, i]) - p_old)
                if error > max_error:
                    max_error = error
        _bcs(P)
        errs.append(max_error)
        if tol_enabled and _below(max_error, p_tol):
            break
    return P, len(errs), errs


def sor_lex_diag(rhs, nx, ny, dx, dy, iters, tol_enabled=True, p_tol=1e-4):
    dx2, dy2, denom = consts(dx, dy)
    R = np.asarray(rhs, np.float32).reshape(-1).astype(np.float64)
    P = np.zeros(nx * ny, np.float32)
    diags = []
    for d in range(2, nx + ny - 3):
        j = np.arange(max(1, d - (nx - 2)), min(ny - 2, d - 1) + 1)
        diags.append(j * nx + (d - j))
    rd = [R[idx] for idx in diags]
    errs = []
    with np.errstate(all="ignore"):
        for _ in range(iters):
            max_error = 0.0
            for idx, r in zip(diags, rd):
                p_old = P[idx].astype(np.float64)
                h = (P[idx + 1].astype(np.float64) + P[idx - 1].astype(np.float64)) / dx2
                v = (P[idx + nx].astype(np.float64) + P[idx - nx].astype(np.float64)) / dy2
                p_update = (h + v - r) / denom
                new = ((1 - OMEGA) * p_old + OMEGA * p_update).astype(np.float32)
                P[idx] = new
                err = np.abs(new.astype(np.float64) - p_old)
                err = err[err > max_error]          # NaN never enters, as `>` in the script
                if err.size:
                    max_error = float(err.max())
            _bcs(P.reshape(ny, nx))
            errs.append(max_error)
            if tol_enabled and _below(max_error, p_tol):
                break
    return P.reshape(ny, nx), len(errs), errs
