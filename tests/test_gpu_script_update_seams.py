"""GPU: the two passes around the substeps of cfd_script_update
(cfd_script_update.hip: k_script_begin, k_script_end) at the seams of their
flat mapping -- nu + nv words, 1024 to a block, a thread striding by 256 --
against the restatement (tests/_script_update_ref.py) on the grids and planted
words of tests/_script_step_cases.py, whose premises
test_script_step_seams_cpu.py checks without a device:

* grids of fewer words than one thread stride, of an exact multiple of the
  block with the u|v boundary mid-block and mid-wave, of one word past a block,
  and with the u|v boundary on a thread stride;
* on each, the maximum of |u - uOld| or |v - vOld| planted in the first and the
  last word of u and of v (flat words 0, nu - 1, nu, nu + nv - 1), and nowhere
  else near it;
* every velocity zero (max_vel == 0: the dt rule returns dt_user), zero but for
  the last word, and a NaN in the first word, which no maximum takes.

One step from a seeded state at step 7 (k_script_begin extrapolates), two
substeps, the script's Jacobi.  Fields and u_prev / v_prev bitwise, the
report's doubles by value and bits.
"""
import numpy as np
import pytest

import _script_step_cases as t
import _script_update_ref as upd
from _util import assert_bitwise

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.float64(x).view(np.uint64)


@pytest.mark.parametrize("gname,kind", t.UPDATE_CASES)
def test_update_matches_restatement(gname, kind):
    import cfdamd as c
    g, st0, target, want, rep = t.updated(gname, kind)
    s = t.UPDATE_SOLVER
    m = c.Model(c.Grid(g.nx, g.ny, g.lx, g.ly),
                c.SimulationParams(viscosity=g.nu, pressure_solver=c.PressureSolver(s),
                                   jacobi_iters=upd.ITERS, tol_enabled=True, p_tol=upd.P_TOL[s]))
    try:
        m.set_state(u=st0["u"].ravel(), v=st0["v"].ravel(), p=st0["p"].ravel())
        m.script_begin(st0)
        r = m.script_update(c.ScriptScheme(t.UPDATE_SCHEME), target, t.UPDATE_DT_USER,
                            c.InletProfile(t.UPDATE_PROFILE))
        tag = f"{gname} {kind}"
        st = m.get_state()
        for f in ("u", "v", "p"):
            assert_bitwise(f"{tag}: {f}", st[f], want[f].ravel())
        ss = m.script_state()
        assert_bitwise(f"{tag}: u_prev", ss["u_prev"], want["u_prev"].ravel())
        assert_bitwise(f"{tag}: v_prev", ss["v_prev"], want["v_prev"].ravel())
        for k in ("residual_u", "residual_v", "residual_p", "dt_next", "inlet_velocity"):
            assert _bits(getattr(r, k)) == _bits(rep[k]), (tag, k, getattr(r, k), rep[k])
        assert (r.substeps_run, r.substep_count_next, r.step_count) == \
            (t.UPDATE_SUBSTEPS, rep["substep_count_next"], t.UPDATE_STEP + 1), tag
        assert (ss["dt"], ss["substep_count"], ss["step_count"]) == \
            (rep["dt_next"], rep["substep_count_next"], t.UPDATE_STEP + 1), tag
    finally:
        m.close()
