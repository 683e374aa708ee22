"""CPU: the reference side of tests/test_gpu_adversarial.py, double-checked.

The GPU tests compare the default-path kernels with oracle/cfd_oracle.c on
random, wide-range and non-finite states (_util.adversarial_state) and on
planted-spike Jacobi solves (_util.spike_state).  Here the C restatement and
the independent numpy restatement (oracle/np_model.py) must agree bit for bit
on the same inputs, so a mistake in how either restates the reference's
NaN-ignoring maxima (model.rs:795-798, f32::max / reduce_max), the residual's
column range (:752-772) or the upwind selects shows without a GPU.  The
oracle-only preconditions the GPU tests rely on -- the non-finite share of a
`nonfinite` step, the planted spike's included / excluded discrimination,
the exit sweeps of the tolerance list -- are asserted here too.
"""
import numpy as np
import pytest

from _util import (ADV_FIELDS, ADV_FLAVOURS, adversarial_state, assert_bitwise, load_state,
                   nonfinite_share, same_f32, SPIKE_P_TOLS, spike_columns, spike_rows, spike_state)
from np_model import NpModel
from oracle import OracleModel

NPF = {f: ("pp" if f == "p_prime" else f) for f in ADV_FIELDS}
P2 = 1.0 / 128.0   # dx = dy = 2^-7

# (grid, params) -- the small shapes of the GPU module and its tall channel
CASES = {
    "16x4": (dict(nx=16, ny=4, lx=16 * P2, ly=4 * P2), dict(bc_kind=1, viscosity=0.01)),
    "120x37": (dict(nx=120, ny=37, lx=120 * P2, ly=37 * P2), dict(bc_kind=1, viscosity=0.01)),
    "248x13": (dict(nx=248, ny=13, lx=248 * P2, ly=13 * P2), dict(bc_kind=1, viscosity=0.01)),
    "248x301": (dict(nx=248, ny=301, lx=8.0, ly=10.0, cylinder=(4.0, 5.0, 1.0)), dict()),
}


def _pair(g, **p):
    return OracleModel(**g, **p), NpModel(**g, **p)


def _same_scalars(o, n):
    s = o.scalars()
    assert (s.step, s.jacobi_sweeps_total) == (n.step, n.sweeps)
    for a, b in ((s.dt, n.dt), (s.time, n.time), (s.p, n.res_p), (s.u, n.res_u), (s.v, n.res_v)):
        assert same_f32(a, b), (a, b)


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("flavour", ADV_FLAVOURS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_restatements_agree_on_adversarial_step(case, flavour, scheme):
    g, kw = CASES[case]
    nonfinite = flavour == "nonfinite"
    kw = dict(kw, scheme=scheme, corrector_passes=2, tol_enabled=0,
              jacobi_iters=3 if nonfinite else 9, inlet_profile=scheme)
    o, n = _pair(g, **kw)
    st = adversarial_state(g["nx"], g["ny"], 1, flavour)
    load_state(st, oracle=o, np_model=n)
    for step in range(1 if nonfinite else 2):
        o.update()
        n.update()
        for f in ADV_FIELDS:
            assert_bitwise(f"{case} {flavour} step {step}: {f}", o.field(f), getattr(n, NPF[f]),
                           nan_equal=nonfinite)
        _same_scalars(o, n)
    if nonfinite:
        # the planted words reached the result and left most of it comparable
        share = nonfinite_share([o.field(f) for f in ADV_FIELDS])
        assert 0.0 < share <= 0.20 or g["nx"] * g["ny"] < 1000, share
    else:
        assert nonfinite_share([o.field(f) for f in ADV_FIELDS]) == 0.0


def _jacobi_pair(g, pp, rhs, **kw):
    o, n = _pair(g, **kw)
    o.field("p_prime")[:] = pp
    o.field("rhs")[:] = rhs
    n.pp[:] = pp
    n.rhs[:] = rhs
    ro, rn = o.jacobi(), n.jacobi()
    return o, n, ro, rn


SOLVES = [(1, 0, 1e-4), (9, 0, 1e-4), (17, 0, 1e-4), (50, 1, 0.04), (50, 1, 0.008)]


@pytest.mark.parametrize("nan_in", [None, "p_prime", "rhs"])
@pytest.mark.parametrize("case,iters,tol,p_tol", [
    (c,) + s for c in sorted(CASES) for s in SOLVES
    if c != "248x301" or s[0] <= 9])   # the tall grid (numpy: 75 k cells a sweep): short solves
def test_restatements_agree_on_planted_spike(case, iters, tol, p_tol, nan_in):
    g, _ = CASES[case]
    nx, ny = g["nx"], g["ny"]
    for col in spike_columns(nx):
        for row in spike_rows(ny):
            pp, rhs = spike_state(nx, ny, 2, col, row, nan_in)
            o, n, ro, rn = _jacobi_pair(g, pp, rhs, jacobi_iters=iters, tol_enabled=tol, p_tol=p_tol)
            tag = f"{case} iters={iters} tol={tol} spike ({col},{row}) nan={nan_in}"
            assert same_f32(ro, rn), (tag, ro, rn)
            assert np.isfinite(ro), tag          # the maximum ignores the NaN
            assert o.scalars().jacobi_sweeps_total == n.sweeps, tag
            assert_bitwise(tag, o.field("p_prime"), n.pp, nan_equal=nan_in is not None)


@pytest.mark.parametrize("g", [CASES["120x37"][0], dict(nx=232, ny=20, lx=232 * P2, ly=20 * P2),
                               dict(nx=96, ny=72, lx=2.0, ly=1.5)],
                         ids=["120x37", "232x20", "96x72"])
@pytest.mark.parametrize("iters", [1, 8, 9, 17])
def test_spike_discriminates_included_from_excluded_column(g, iters):
    """The residual with the spike in column nx-8 (the last one it covers)
    differs from that with the spike in nx-7 (the first it leaves out), at
    every row and sweep count the GPU test uses: a kernel that took the
    maximum over all columns could not match both."""
    nx, ny = g["nx"], g["ny"]
    for row in spike_rows(ny):
        res = []
        for col in (nx - 8, nx - 7):
            o = OracleModel(**g, jacobi_iters=iters, tol_enabled=0)
            pp, rhs = spike_state(nx, ny, 2, col, row)
            o.field("p_prime")[:] = pp
            o.field("rhs")[:] = rhs
            res.append(np.float32(o.jacobi()))
        assert res[0] != res[1], (row, iters, res)
        if iters == 1:
            # one sweep: the spike itself (0.75 down) against its neighbour (0.19 up)
            assert res[0] > 0.7 and res[1] < 0.25, res


def test_tolerance_list_exit_sweeps():
    """The exit sweeps of the GPU test's tolerance list on 120 x 37 cover at
    least three residues mod 8, a non-zero one among them, and one solve
    runs to the sweep limit."""
    g = CASES["120x37"][0]
    nx, ny = g["nx"], g["ny"]
    exits = set()
    for p_tol in SPIKE_P_TOLS:
        for col in spike_columns(nx):
            for row in spike_rows(ny):
                o = OracleModel(**g, jacobi_iters=50, tol_enabled=1, p_tol=p_tol)
                pp, rhs = spike_state(nx, ny, 2, col, row)
                o.field("p_prime")[:] = pp
                o.field("rhs")[:] = rhs
                o.jacobi()
                exits.add(int(o.scalars().jacobi_sweeps_total))
    residues = {e % 8 for e in exits}
    assert len(residues) >= 3 and residues - {0}, sorted(exits)
    assert 50 in exits and min(exits) < 8, sorted(exits)
