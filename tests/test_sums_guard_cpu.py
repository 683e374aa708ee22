"""CPU: the premises of tests/test_gpu_sums_fma_shapes.py, pinned with the
oracle alone, and the analytic bound the fma form's guard rests on.

The GPU tests plant one p' word, one face velocity or a p' field at the top of
the guard's window (_sums_cases) and read which march body ran from
Model.sums_launches.  Whether each construction does what it is meant to --
where the largest |p'| stands after the step, how many cells carry the
deciding |rhs|, on which side of 2^123 the guard's sum falls, that every field
stays finite or the non-finite share small -- does not depend on the device:
it is asserted here, before a GPU is used.
"""
import numpy as np
import pytest

import _sums_cases as sc
from _util import ADV_FIELDS, adversarial_state, load_state, nonfinite_share
from oracle import OracleModel

MAX_NONFINITE_SHARE = 0.20


def _oracle(nx, ny, **kw):
    kw = dict(dict(bc_kind=1, viscosity=0.01, tol_enabled=0, corrector_passes=0), **kw)
    return OracleModel(**sc.grid(nx, ny), **kw)


def _finite(o):
    return all(np.all(np.isfinite(o.field(f))) for f in ADV_FIELDS)


# ------------------------------------------------ section 3: the finish's maximum

@pytest.mark.parametrize("kind", sc.FINISH_KINDS)
@pytest.mark.parametrize("shape", sc.FINISH_SHAPES)
def test_planted_p_prime_word_holds_the_maximum(shape, kind):
    nx, ny = sc.shape_of(shape)
    residues = set()
    for cls, col, row in sc.finish_cells(shape, nx, ny):
        tag = f"{shape} {cls} ({col},{row}) {kind}"
        o = _oracle(nx, ny, jacobi_iters=1)
        load_state(sc.finish_state(nx, ny, col, row, kind), oracle=o, dt=sc.SPIKE_DT)
        o.update()
        pp = o.field("p_prime")
        top = sc.abs_bits_max(pp)
        cells = sc.argmax_cells(pp, nx)
        residues.add(col % 4)
        if kind == "spike":
            assert _finite(o), tag
            assert top > sc.P_THR_BITS and top < sc.INF_BITS, (tag, hex(top))
            # the planted cell (for row ny-1: the copy the boundary left there)
            # holds the maximum, and only the boundary's copies share it
            assert (col, row) in cells, (tag, cells)
            assert all(abs(c - col) <= 1 and abs(r - row) <= 1 for c, r in cells), (tag, cells)
            # nothing else comes near: the finish's word is this cell's or wrong
            b = np.abs(pp.astype(np.float64))
            b[[c + r * nx for c, r in cells]] = 0.0
            assert b.max() < 0.8 * float(np.abs(pp).max()), tag
        else:
            assert top >= sc.INF_BITS, (tag, hex(top))
            assert (col, row) in cells or (col, row - 1) in cells, (tag, cells)
            share = nonfinite_share([o.field(f) for f in ADV_FIELDS])
            assert 0.0 < share <= MAX_NONFINITE_SHARE, (tag, share)
    if shape != "1024x5":
        assert residues == {0, 1, 2, 3}, (shape, residues)   # every word of a lane's float4


def test_band_shape_has_a_ragged_last_band():
    nx, ny = sc.band_shape(sc.MI355X_CUS)
    rows = {r for _, _, r in sc.finish_cells("band", nx, ny)}
    assert {15, 16, ny - 2, ny - 1} <= rows and (ny + 1) % 16 not in (0, 1)


# ------------------------------------------------- section 4: the march's maximum

def _deciding_cells(rhs, nx):
    k = np.nonzero(np.abs(rhs.astype(np.float64)) >= sc.RHS_DECIDES)[0]
    return [(int(i) % nx, int(i) // nx) for i in k]


@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("shape", sc.MARCH_SHAPES)
def test_planted_face_decides_through_a_handful_of_cells(shape, scheme):
    nx, ny = sc.shape_of(shape)
    for cls, face, row in sc.march_faces(shape, nx, ny):
        for dt, decides in ((sc.MARCH_DT_HI, True), (sc.MARCH_DT_LO, False)):
            tag = f"{shape} scheme {scheme} {cls} face {face} row {row} dt {dt}"
            o = _oracle(nx, ny, jacobi_iters=1, scheme=scheme)
            load_state(sc.march_state(nx, ny, face, row), oracle=o, dt=dt)
            o.update()
            for step in (2, 3):
                pp_before = float(np.max(np.abs(o.field("p_prime"))))
                o.update()
                assert _finite(o), tag
                assert pp_before * sc.R < sc.LIM / 2 / 16, (tag, step, pp_before)
                cells = _deciding_cells(o.field("rhs"), nx)
                if decides:
                    assert 1 <= len(cells) <= 24, (tag, step, len(cells))
                    assert all(abs(c - face) <= 4 and abs(r - row) <= 3 for c, r in cells), (tag, cells)
                else:
                    # the twin: both terms pass with room to spare
                    assert sc.counter_must(sc.guard_bound(np.float32(pp_before), o.field("rhs"))) is True, tag
                    assert float(np.max(np.abs(o.field("rhs")))) > 2.0 ** 90, tag


# ------------------------------------------------- section 5: the window's top

@pytest.mark.parametrize("sweeps", sc.TOP_SWEEPS)
@pytest.mark.parametrize("nx,ny", sc.TOP_SHAPES)
def test_window_top_states_fall_on_their_side(nx, ny, sweeps):
    for name, factor in sc.TOP_FACTORS.items():
        o = _oracle(nx, ny, jacobi_iters=sweeps)
        load_state(sc.top_state(nx, ny, factor), oracle=o, dt=sc.TOP_DT, step=0)
        o.update()
        assert _finite(o), name
        pp1 = o.field("p_prime").copy()
        o.update()
        assert _finite(o), name
        rhs2 = o.field("rhs")
        m0r = float(np.max(np.abs(pp1))) * sc.R
        rm = float(np.max(np.abs(rhs2)))
        assert rm < sc.R_THR, (name, rm)                     # the march publishes its threshold
        assert m0r > 2.0 ** 122 and m0r < sc.LIM, (name, m0r)  # above the finish's threshold: m0 is p' itself
        assert sc.SUMS_C * sc.R_THR < sc.LIM and m0r < sc.LIM   # neither term alone decides
        bound = sc.guard_bound(pp1, rhs2)
        if name == "inside":
            assert bound <= sc.LIM * (1.0 - sc.TOP_MARGIN), (name, bound)
            # the form's own sums stay finite: R (h + v) is at most 4 R max |p'|
            assert 4.0 * m0r * (1 + 2.0 ** -10) < 2.0 ** 128
        else:
            assert bound >= sc.LIM * (1.0 + sc.TOP_MARGIN), (name, bound)


# ------------------------------------------- the bound the guard rests on

@pytest.mark.parametrize("flavour", ["signs", "range"])
@pytest.mark.parametrize("nx,ny", [(16, 4), (120, 37), (232, 20)])
def test_sweep_raises_max_p_prime_by_at_most_the_bound(nx, ny, flavour):
    """max |p'| after sweep k <= (M0 + 0.1875 k Rm / R) (1 + 2^-20)^k, in
    float64: a sweep is 0.75 (h + v - rhs / R) / 4 + 0.25 p', at most 0.75
    M + 0.1875 Rm / R + 0.25 M, and the boundary copies repeat values or write
    zero.  The factor covers the update's at most six f32 roundings."""
    st = adversarial_state(nx, ny, 1, flavour)
    m0 = float(np.max(np.abs(st["p_prime"])))
    rm = float(np.max(np.abs(st["rhs"])))
    o = _oracle(nx, ny, jacobi_iters=1)
    o.field("p_prime")[:] = st["p_prime"]
    o.field("rhs")[:] = st["rhs"]
    for k in range(1, 18):
        o.jacobi()
        got = float(np.max(np.abs(o.field("p_prime"))))
        want = (m0 + 0.1875 * k * rm / sc.R) * (1.0 + 2.0 ** -20) ** k
        assert got <= want, (nx, ny, flavour, k, got, want)
    assert int(o.scalars().jacobi_sweeps_total) == 17
