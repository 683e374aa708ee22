"""GPU: the fma form of the per-launch Jacobi march (LdsMarch<T, 1, MODE, 2>)
at every launch length, on the wave-column seams and ragged row counts, and
its guard at the edge: one cell that decides, and the top of the pass window.

Everything is bitwise against oracle/cfd_oracle.c.  Model.sums_launches tells
which body ran, Model.sums_bounds (cfd_get_sums_bounds) what the publishers
left in Ctl.  The constructions of the guard's edge live in _sums_cases.py;
tests/test_sums_guard_cpu.py pins their premises with the oracle alone.

Launch lengths.  cfd_plan_block (one domain) gives a solve of n sweeps
ceil(n / 8) launches that share the sweeps evenly; the last one carries the
residual (MODE 1).  A launch that is not the last is followed by at least one
sweep, so it belongs to a solve of >= 9 sweeps and >= 2 launches and has
ceil(rem / ceil(rem / 8)) >= 5 sweeps: the planner emits MODE 0 launches of
T = 5, 6, 7, 8 only.  SWEEPS covers (T, MODE 1) for T = 1..8 and (T, MODE 0)
for T = 5..8; test_plan_coverage asserts both from the plan itself.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _sums_cases as sc
from _util import ADV_FIELDS, adversarial_state, assert_bitwise, load_state, nonfinite_share, same_f32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# POW2_SHAPES of test_gpu_adversarial.py and its 232 x 20
SHAPES = [(16, 4), (112, 9), (120, 37), (232, 20), (240, 12), (248, 13), (1024, 5), (1032, 6)]
SWEEPS = (1, 2, 3, 4, 7, 8, 9, 13, 15, 17, 24)
T_MAX = 8
MAX_NONFINITE_SHARE = 0.20
KIND5 = {"kind": 5, "name": "k_jacobi_lds<8, 1, 0>"}


def _cfd():
    import cfdamd
    return cfdamd


def _n_cu():
    """Compute units of device 0, from the HIP runtime the library runs on."""
    _cfd().load()
    hip = None
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            pass
    assert hip is not None, "libamdhip64.so not found"
    n = C.c_int(0)
    rc = hip.hipDeviceGetAttribute(C.byref(n), 63, 0)   # hipDeviceAttributeMultiprocessorCount
    assert rc == 0 and 0 < n.value <= 4096, (rc, n.value)
    return n.value


def _pair(nx, ny, **kw):
    """A cavity on dx = dy = 2^-7 with the tolerance off: model and oracle."""
    c = _cfd()
    from oracle import OracleModel
    kw = dict(dict(scheme=0, corrector_passes=0, tol_enabled=0, bc_kind=1, viscosity=0.01), **kw)
    params = c.SimulationParams(
        viscosity=kw["viscosity"], velocity_scheme=c.VelocityScheme(kw["scheme"]),
        jacobi_iters=kw["jacobi_iters"], corrector_passes=kw["corrector_passes"], tol_enabled=False,
        bc_kind=c.BoundaryKind(1))
    g = sc.grid(nx, ny)
    m = c.Model(c.Grid(nx, ny, g["lx"], g["ly"], None), params)
    o = OracleModel(nx, ny, g["lx"], g["ly"], **kw)
    assert m.jacobi_kernel == KIND5, m.jacobi_kernel
    cfg = m.kernel_config
    assert cfg["fastdiv"] == 1 and cfg["temporal"] == T_MAX, cfg
    return m, o


def _compare(tag, m, o, nan_equal=False):
    """Every ADV_FIELDS word and every scalar; returns the model's state."""
    st = m.get_state()
    for f in ADV_FIELDS:
        assert_bitwise(f"{tag}: {f}", st[f], o.field(f), nan_equal=nan_equal)
    s = o.scalars()
    assert st["simulation_step"] == s.step, tag
    assert st["jacobi_sweeps_total"] == s.jacobi_sweeps_total, tag
    for k, want in (("dt", s.dt), ("simulation_time", s.time), ("last_p_residual", s.p),
                    ("last_u_residual", s.u), ("last_v_residual", s.v)):
        assert same_f32(st[k], want) or (nan_equal and np.isnan(st[k]) and np.isnan(want)), \
            (tag, k, st[k], want)
    return st


def _check_bounds(tag, m, st):
    """After a step: its last kernels bounded the model's own p' and nothing
    else stands in the words."""
    b = m.sums_bounds
    want = max(sc.P_THR_BITS, sc.abs_bits_max(st["p_prime"]))
    assert b == {"state": 1, "m0": want, "rm": 0}, (tag, b, hex(want))
    return b


# ------------------------------------------------------------ the plan

def _plan(iters, ny):
    """[(T, MODE)] of one fixed-count solve, from cfd_plan_block as
    Model.launches_per_solve walks it."""
    L = _cfd().load()
    T, lo, hi, ex = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    it, out = 0, []
    while it < iters:
        rc = L.cfd_plan_block(0, ny, ny, 0, it, T_MAX, iters, C.byref(T), C.byref(lo), C.byref(hi),
                              C.byref(ex))
        assert rc == 0 and 1 <= T.value <= T_MAX
        it += T.value
        out.append((T.value, 1 if it == iters else 0))
    return out


def test_plan_coverage():
    found = sorted({tm for n in SWEEPS for tm in _plan(n, 37)})
    print("launches (T, MODE) of SWEEPS:", found)
    assert [t for t, mode in found if mode == 1] == list(range(1, 9)), found
    # every non-final length the planner can emit at all (solves up to 512
    # sweeps; the module docstring says why longer ones add none)
    emitted = sorted({t for n in range(1, 513) for t, mode in _plan(n, 37) if mode == 0})
    assert emitted == [5, 6, 7, 8], emitted
    assert [t for t, mode in found if mode == 0] == emitted, found
    for nx, ny in SHAPES:   # the plan of one domain does not depend on the rows
        assert all(_plan(n, ny) == _plan(n, 37) for n in SWEEPS), ny


# ----------------------------------------------- section 2: the parity matrix

def _run_matrix(nx, ny, sweeps, flavour, scheme=0, passes=0):
    tag0 = f"{nx}x{ny} sweeps {sweeps} {flavour} scheme {scheme} passes {passes}"
    m, o = _pair(nx, ny, jacobi_iters=sweeps, scheme=scheme, corrector_passes=passes)
    try:
        per_solve = m.launches_per_solve()
        assert per_solve == len(_plan(sweeps, ny)), (tag0, per_solve)
        load_state(adversarial_state(nx, ny, 1, flavour), model=m, oracle=o)
        assert m.sums_launches == 0
        assert m.sums_bounds == {"state": 0, "m0": 0, "rm": 0}, m.sums_bounds   # set_state dropped them
        seen = []
        for step in (1, 2, 3):
            m.update()
            o.update()
            st = _compare(f"{tag0} step {step}", m, o)
            seen.append((step, m.sums_launches, m.sums_bounds, st["p_prime"]))
        print(f"{tag0}: launches per solve {per_solve}, counter after steps 1..3 "
              f"{[n for _, n, _, _ in seen]}, bounds {[b for _, _, b, _ in seen]}")
        for step, n, b, pp in seen:
            tag = f"{tag0} step {step}"
            # step 1 has no valid maxima; later ones take the form in the
            # step's first solve only
            assert n == per_solve * (step - 1), (tag, n, per_solve)
            want = max(sc.P_THR_BITS, sc.abs_bits_max(pp))
            assert b == {"state": 1, "m0": want, "rm": 0}, (tag, b, hex(want))
    finally:
        m.close()


@pytest.mark.parametrize("flavour", ["signs", "range"])
@pytest.mark.parametrize("sweeps", SWEEPS)
@pytest.mark.parametrize("nx,ny", SHAPES)
def test_form_parity_matrix(nx, ny, sweeps, flavour):
    """Three steps from an adversarial state at every launch length; sweeps
    == 1 enters the second step's solve with a p' one sweep old."""
    _run_matrix(nx, ny, sweeps, flavour)


SUB_SHAPES = [(120, 37), (248, 13)]
SUB_SWEEPS = (1, 9, 17, 24)


@pytest.mark.parametrize("flavour", ["signs", "range"])
@pytest.mark.parametrize("sweeps", SUB_SWEEPS)
@pytest.mark.parametrize("nx,ny", SUB_SHAPES)
def test_form_parity_second_order(nx, ny, sweeps, flavour):
    """The second-order predictor march publishes max |rhs| (scheme 0 with no
    corrector passes is the matrix above)."""
    _run_matrix(nx, ny, sweeps, flavour, scheme=1, passes=0)


@pytest.mark.parametrize("flavour", ["signs", "range"])
@pytest.mark.parametrize("sweeps", SUB_SWEEPS)
@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("nx,ny", SUB_SHAPES)
def test_form_parity_with_corrector_passes(nx, ny, scheme, sweeps, flavour):
    """Two corrector passes: a step has three solves and only the first takes
    the form -- its finalize returns sums_state to 0 and a corrector pass
    publishes nothing -- so the counter advances by one solve's launches per
    step.  Such a step ends in k_correct_head4, not k_correct_finish4m: the
    bound words read back here are k_publish_sums_m0's."""
    _run_matrix(nx, ny, sweeps, flavour, scheme=scheme, passes=2)


_CHILD = r"""
import sys, numpy as np
sys.path[:0] = [{pkg!r}, {tests!r}]
import cfdamd
import _sums_cases as sc
from _util import ADV_FIELDS, adversarial_state, load_state
out = {{}}
for nx, ny in {shapes!r}:
    params = cfdamd.SimulationParams(viscosity=0.01, jacobi_iters={iters}, corrector_passes=0,
                                     tol_enabled=False, bc_kind=cfdamd.BoundaryKind(1))
    g = sc.grid(nx, ny)
    m = cfdamd.Model(cfdamd.Grid(nx, ny, g["lx"], g["ly"], None), params)
    load_state(adversarial_state(nx, ny, 1, "signs"), model=m)
    for _ in range(3):
        m.update()
    st = m.get_state()
    out["%dx%d" % (nx, ny)] = np.concatenate(
        [np.ascontiguousarray(st[f], np.float32).view(np.uint32).ravel() for f in ADV_FIELDS])
    print("shape", nx, ny, "launches", m.sums_launches, "bounds", sorted(m.sums_bounds.items()))
    m.close()
np.savez({out!r}, **out)
"""


def test_knob_off_same_words_counter_and_bounds_zero(tmp_path):
    """CFD_JACOBI_SUMS=0 in a child process (the environment of a process that
    holds the GPU never changes): the same state words as with the form, the
    counter 0 and the bound words all zero, on every shape."""
    iters = 9
    want = {}
    for nx, ny in SHAPES:
        m, _ = _pair(nx, ny, jacobi_iters=iters)
        try:
            load_state(adversarial_state(nx, ny, 1, "signs"), model=m)
            for _ in range(3):
                m.update()
            st = m.get_state()
            want[f"{nx}x{ny}"] = np.concatenate([sc.bits(st[f]) for f in ADV_FIELDS])
            assert m.sums_launches == 2 * m.launches_per_solve() > 0
        finally:
            m.close()
    out = str(tmp_path / "off.npz")
    code = _CHILD.format(pkg=os.path.join(ROOT, "cfd-demo_amd"), tests=os.path.join(ROOT, "tests"),
                         shapes=SHAPES, iters=iters, out=out)
    env = dict(os.environ, CFD_JACOBI_SUMS="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    for nx, ny in SHAPES:
        line = f"shape {nx} {ny} launches 0 bounds [('m0', 0), ('rm', 0), ('state', 0)]"
        assert line in r.stdout, (line, r.stdout)
        assert np.array_equal(got[f"{nx}x{ny}"], want[f"{nx}x{ny}"]), (nx, ny)


# ------------------------------- section 3: the finish's maximum sees every cell

@pytest.mark.parametrize("kind", sc.FINISH_KINDS)
@pytest.mark.parametrize("shape", sc.FINISH_SHAPES)
def test_finish_maximum_sees_the_planted_cell(shape, kind):
    """One p' word far above the rest (or one NaN / +Inf), planted at the
    first and last swept column, on both sides of k_correct_finish4m's 1024-
    column chunk, in rows 1, ny-2 and ny-1, and -- on the band shape, 16 x
    (32 n_cu + 9) -- on both sides of the first 16-row band's end and in the
    ragged last band; the columns take every word of a lane's float4.  After
    one update() the published m0 is the largest |p'| word of the model's own
    p', which the planted cell (or the boundary's copy of it) holds.  NaN and
    Inf stand above every finite value: the publishers' answer to them, read
    back here, is what a solve's guard would refuse on."""
    nonfinite = kind != "spike"
    nx, ny = sc.shape_of(shape, _n_cu() if shape == "band" else None)
    for cls, col, row in sc.finish_cells(shape, nx, ny):
        tag = f"{shape} {cls} ({col},{row}) {kind}"
        m, o = _pair(nx, ny, jacobi_iters=1)
        try:
            load_state(sc.finish_state(nx, ny, col, row, kind), model=m, oracle=o, dt=sc.SPIKE_DT)
            m.update()
            o.update()
            st = _compare(tag, m, o, nan_equal=nonfinite)
            pp = st["p_prime"]
            top = sc.abs_bits_max(pp)
            cells = sc.argmax_cells(pp, nx)
            b = m.sums_bounds
            print(f"{tag}: m0 {b['m0']:08x} max |p'| bits {top:08x} at {cells[:4]}")
            if nonfinite:
                assert top >= sc.INF_BITS, (tag, hex(top))
                assert (col, row) in cells or (col, row - 1) in cells, (tag, cells)
                share = nonfinite_share([st[f] for f in ADV_FIELDS])
                assert 0.0 < share <= MAX_NONFINITE_SHARE, (tag, share)
            else:
                assert sc.P_THR_BITS < top < sc.INF_BITS, (tag, hex(top))
                assert (col, row) in cells, (tag, cells)
                assert all(np.all(np.isfinite(st[f])) for f in ADV_FIELDS), tag
            assert b == {"state": 1, "m0": top, "rm": 0}, (tag, b, hex(top))
            assert m.sums_launches == 0, tag
        finally:
            m.close()


# --------------------------- section 4: the march's maximum decides from one cell

@pytest.mark.parametrize("scheme", [0, 1])
@pytest.mark.parametrize("shape", sc.MARCH_SHAPES)
def test_march_maximum_decides_from_one_face(shape, scheme):
    """One u face of 3 over velocities of 2^-14 with a dt so small that the
    divergence / dt of its two cells alone lifts 768 max |rhs| above 2^124,
    while R max |p'| stays under 2^118: on steps 2 and 3 the counter stands
    still.  The face sits at the first and last predicted column, between the
    last two chunks of a wave column, in the first and last predicted row and
    on rows stored by two 8-row segments and by the last one alone; 1032 x 6
    takes the 4-row segments.  _sums_cases.march_faces says why face nx has no case.
    The twin, 20 binades lower, runs the form."""
    nx, ny = sc.shape_of(shape)
    for cls, face, row in sc.march_faces(shape, nx, ny):
        for dt, decides in ((sc.MARCH_DT_HI, True), (sc.MARCH_DT_LO, False)):
            tag0 = f"{shape} scheme {scheme} {cls} face {face} row {row} dt {float(dt):.3g}"
            m, o = _pair(nx, ny, jacobi_iters=1, scheme=scheme)
            try:
                assert m.launches_per_solve() == 1
                load_state(sc.march_state(nx, ny, face, row), model=m, oracle=o, dt=dt)
                m.update()
                o.update()
                st = _compare(f"{tag0} step 1", m, o)
                assert m.sums_launches == 0, tag0
                for step in (2, 3):
                    tag = f"{tag0} step {step}"
                    pp_before = float(np.max(np.abs(st["p_prime"])))
                    m.update()
                    o.update()
                    st = _compare(tag, m, o)
                    assert all(np.all(np.isfinite(st[f])) for f in ADV_FIELDS), tag
                    rhs = np.abs(st["rhs"].astype(np.float64)).ravel()
                    k = np.nonzero(rhs >= sc.RHS_DECIDES)[0]
                    print(f"{tag}: max|p'| before 2^{np.log2(max(pp_before, 1e-300)):.1f} "
                          f"max|rhs| 2^{np.log2(rhs.max()):.1f} deciding cells {k.size}")
                    assert pp_before * sc.R < 2.0 ** 122 / 16, (tag, "max |p'| must not decide")
                    if decides:
                        assert 1 <= k.size <= 24, (tag, k.size)
                        assert all(abs(int(i) % nx - face) <= 4 and abs(int(i) // nx - row) <= 3
                                   for i in k), (tag, k)
                        assert m.sums_launches == 0, (tag, m.sums_launches)
                    else:
                        assert sc.counter_must(sc.guard_bound(np.float32(pp_before), st["rhs"])) is True, tag
                        assert m.sums_launches == step - 1, (tag, m.sums_launches)
                    _check_bounds(tag, m, st)
            finally:
                m.close()


# --------------------------------------- section 5: parity at the window's top

@pytest.mark.parametrize("name", sorted(sc.TOP_FACTORS))
@pytest.mark.parametrize("sweeps", sc.TOP_SWEEPS)
@pytest.mark.parametrize("nx,ny", sc.TOP_SHAPES)
def test_parity_at_the_top_of_the_window(nx, ny, sweeps, name):
    """p' = C (1 + a few ulps) with R C = 1.1 * 2^122 (`inside`) or 1.5 *
    2^122 (`above`) and velocities dt grad p' (sc.top_state): step 1 keeps p'
    and leaves rounding residue for velocities, so step 2 meets max |p'| R
    just above the finish's threshold and an rhs under the march's.  The
    guard's sum, formed here in f32 from the read-back p' and rhs, is then
    <= 2^123 (1 - 2^-10): the form must run, with R (h + v) near 1.1 * 2^124,
    and match; or >= 2^123 (1 + 2^-10) with neither term above its share: it
    must be refused.  Step 3 starts from the relaxed p' with an rhs near R C
    / 4, which no choice of state avoids (the corrected velocities carry the
    solve's residual); there the counter must agree with the host's bound
    whichever side it falls on."""
    m, o = _pair(nx, ny, jacobi_iters=sweeps)
    try:
        per_solve = m.launches_per_solve()
        load_state(sc.top_state(nx, ny, sc.TOP_FACTORS[name]), model=m, oracle=o, dt=sc.TOP_DT, step=0)
        count = 0
        st = None
        for step in (1, 2, 3):
            tag = f"{nx}x{ny} sweeps {sweeps} {name} step {step}"
            pp_before = None if st is None else st["p_prime"].copy()
            m.update()
            o.update()
            st = _compare(tag, m, o)
            assert all(np.all(np.isfinite(st[f])) for f in ADV_FIELDS), tag
            if step > 1:
                bound = sc.guard_bound(pp_before, st["rhs"])
                must = sc.counter_must(bound)
                print(f"{tag}: bound / 2^123 = {float(bound) / sc.LIM:.6f} must run: {must}")
                if step == 2:
                    assert float(np.max(np.abs(st["rhs"]))) < sc.R_THR, tag
                    assert 2.0 ** 122 < float(np.max(np.abs(pp_before))) * sc.R < sc.LIM, tag
                    assert must is (name == "inside"), (tag, bound)
                ran = m.sums_launches - count
                assert ran in (0, per_solve), (tag, ran)
                if must is not None:
                    assert (ran == per_solve) is must, (tag, ran, bound)
                count += ran
            else:
                assert m.sums_launches == 0, tag
            _check_bounds(tag, m, st)
    finally:
        m.close()
