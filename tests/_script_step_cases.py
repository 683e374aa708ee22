"""The case table of the script substep's and update's seam tests
(cfd_script_step.hip: k_script_predict, k_script_correct; cfd_script_update.hip:
k_script_begin, k_script_end): test_script_step_seams_cpu.py checks its
premises with the restatements alone (tests/_script_step_ref.py,
tests/_script_update_ref.py), test_gpu_script_step_seams.py and
test_gpu_script_update_seams.py run the kernels on every case a model can be
built for.

Predictor geometry (cfd_script_step.hip's header): a lane owns chunk c (columns
4c .. 4c+3), chunk nch = nx / 4 holds u face nx alone; wave column w owns chunks
62w-1 .. 62w+62 and stores from lanes 1 .. 62, so there are nwc =
ceil((nch + 1) / 62) wave columns and the face-nx chunk sits in wave column
nch // 62 on lane nch % 62 + 1.  A wave marches R rows (8, or 4 when ny < 8)
from r0 = min(seg R, ny - R); a block holds four segments.

cfd_create takes nx % 8 == 0, nx >= 16 only (include/cfd.h), although
script_step_ok would admit nx % 4 == 0, nx >= 8.  nch is therefore even on the
device: the face-nx chunk never sits on lane 62 (nx = 244) and no wave column
is exactly full (nx = 244, 492), and the two-chunk grid (nx = 8) cannot be
built.  Those widths (8, 12, 244, 252, 492) stay in the table for the
restatement -- `device` is False for them and the CPU file asserts that the
constructor refuses each -- and the nearest widths a model accepts (16, 24,
256, 488) run beside them: 16 is the smallest grid a model has (four chunks and
the face lane), 488 puts the face-nx chunk on lane 61 of the second wave column
(its right neighbour out of the domain, loading through the far offset), 248
and 496 put it alone in the next wave column, lane 63 of the previous one
supplying `east`.
"""
from collections import namedtuple

import numpy as np

import _script_step_ref as ref
import _script_update_ref as upd

NU = 0.01
SCHEMES = (ref.FIRST, ref.SECOND, ref.QUICK)
PATHS = ("pow2", "div")

# ------------------------------------------------------------------ geometry
Geometry = namedtuple("Geometry", "nch nwc face_wc face_lane R nseg starts nblocks")


def geometry(nx, ny):
    """What launch_script_predict and k_script_predict derive from (nx, ny)."""
    nch = nx // 4
    nwc = -(-(nch + 1) // 62)
    R = 8 if ny >= 8 else 4
    nseg = -(-ny // R)
    starts = tuple(min(s * R, ny - R) for s in range(nseg))
    return Geometry(nch, nwc, nch // 62, nch % 62 + 1, R, nseg, starts, nwc * -(-nseg // 4))


def on_device(nx, ny):
    """cfd_create's shape test (cfd_model_build.hip validate)."""
    return nx >= 16 and nx % 8 == 0 and ny >= 4


def spacing(nx, ny, path):
    """(lx, ly): pow2 gives dx = 1/16, dy = 1/8 (scr.fast = 1: every division by
    a spacing is a multiply by its exact reciprocal), div gives 0.06 and 0.11."""
    assert path in PATHS
    return (nx / 16.0, ny / 8.0) if path == "pow2" else (nx * 0.06, ny * 0.11)


def is_fast(g):
    """script_build's scr.fast: dx, dy and their squares exact powers of two."""
    def pow2(x):
        m, _ = np.frexp(x)
        return x > 0 and m == 0.5
    return all(pow2(x) for x in (g.dx, g.dy, g.dx * g.dx, g.dy * g.dy))


def cylinder(nx, ny, lx, ly):
    """An interior disc where the grid holds one (the CPU file asserts it
    touches no boundary face): on the seam between the first two wave columns
    (column 248) where the grid reaches past it, else at 0.3 lx."""
    if nx < 16 or ny < 9:
        return None
    dx = lx / nx
    cx = 248 * dx if nx >= 488 else 0.3 * lx
    return (cx, 0.5 * ly, min(0.22 * ly, 0.15 * lx))


# ------------------------------------------------------------ predictor shapes
WIDTHS = (8, 12, 240, 244, 248, 252, 492, 496)      # the seams
DEVICE_WIDTHS = (16, 24, 256, 488)                  # beside the widths a model refuses
HEIGHTS = (4, 5, 7, 8, 9, 16, 17, 33)

_shapes = []
for _nx in WIDTHS + DEVICE_WIDTHS:
    _shapes += [(_nx, 9), (_nx, 33)]
for _ny in HEIGHTS:
    _shapes += [(8, _ny), (16, _ny), (248, _ny)]
_shapes += [(8, 4), (16, 4), (496, 33)]
SHAPES = sorted(set(_shapes))

Case = namedtuple("Case", "name nx ny path lx ly cyl dt_sub seed device")
DT_SUB = float(np.float32(0.002))


def _case(nx, ny, path, k):
    lx, ly = spacing(nx, ny, path)
    return Case(f"{nx}x{ny}_{path}", nx, ny, path, lx, ly, cylinder(nx, ny, lx, ly), DT_SUB,
                7000 + k, on_device(nx, ny))


CASES = [_case(nx, ny, path, 2 * k + p) for k, (nx, ny) in enumerate(SHAPES)
         for p, path in enumerate(PATHS)]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
DEVICE_CASES = [c for c in CASES if c.device]
# the whole substep, one per solver, on the shape with the face-nx chunk alone
# in the second wave column and a fifth, overlapping segment in a second block
SUBSTEP_CASE = "248x33_div"
SUBSTEP_SOLVERS = (2, 4, 5)


def grid_of(c):
    return ref.Grid(c.nx, c.ny, c.lx, c.ly, NU, c.cyl)


def random_state(g, seed, dt_sub, cfl=0.6):
    """test_gpu_script_step.py's _random_state: CFL-scaled uniform velocities
    with eight 3 x 3 patches each of +0 and -0 (asserted equal on the CPU)."""
    rng = np.random.default_rng(seed)
    u = (rng.uniform(-1, 1, (g.ny, g.nx + 1)) * cfl * g.dx / dt_sub).astype(np.float32)
    v = (rng.uniform(-1, 1, (g.ny + 1, g.nx)) * cfl * g.dy / dt_sub).astype(np.float32)
    p = rng.uniform(-1, 1, (g.ny, g.nx)).astype(np.float32)
    for z in (np.float32(0.0), np.float32(-0.0)):
        for _ in range(8):
            j, i = int(rng.integers(0, g.ny)), int(rng.integers(0, g.nx))
            u[j:j + 3, i:i + 3] = z
            v[j:j + 3, i:i + 3] = z
    return u, v, p


_REF = {}


def _frozen(key, make):
    if key not in _REF:
        _REF[key] = make()
        for a in _REF[key]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _REF[key]


def predicted(c, scheme):
    """(u, v, p, u*, v*, rhs, counters) of a predictor case, computed once;
    callers leave the arrays unchanged."""
    def make():
        g = grid_of(c)
        u, v, p = random_state(g, c.seed, c.dt_sub)
        cnt = {}
        return (u, v, p) + ref.predict(g, u, v, c.dt_sub, scheme, cnt) + (cnt,)
    return _frozen(("predict", c.name, scheme), make)


# ------------------------------------------- clipped and degenerate obstacles
# 248 x 16 on 15.5 x 1 (dx = dy = 1/16, the reciprocal path) and 16 x 5 on
# 1.6 x 0.5 (dx = dy = 0.1 in f32, IEEE division); 8 x 5 on 0.8 x 0.5 beside it
# for the restatement (a model refuses the width).
# counts: obstacle faces (u column 0, u column nx, u row 0, u row ny-1, v row 0,
# v row ny, all u, all v) of the restatement, asserted on the CPU
Disc = namedtuple("Disc", "name nx ny lx ly cyl counts device")
_DISCS_248 = [
    ("inlet", (0.0, 0.5, 0.3), (10, 0, 0, 0, 0, 0, 42, 37)),
    ("outlet", (15.5, 0.5, 0.3), (0, 10, 0, 0, 0, 0, 42, 37)),
    # its outermost rows hold u face nx alone: the interval [nx, nx + 1)
    ("outlet_one_face_rows", (15.5, 0.5, 0.285), (0, 10, 0, 0, 0, 0, 36, 31)),
    ("bottom_wall", (7.0, 0.0, 0.3), (0, 0, 9, 0, 10, 0, 37, 42)),
    ("top_wall", (7.0, 1.0, 0.3), (0, 0, 0, 9, 0, 10, 37, 42)),
    ("taller_than_channel", (7.0, 0.5, 0.6), (0, 0, 11, 11, 10, 10, 264, 276)),
    ("corner_inlet_bottom", (0.0, 0.0, 0.2), (3, 0, 4, 0, 3, 0, 9, 9)),
    ("corner_outlet_top", (15.5, 1.0, 0.2), (0, 3, 0, 4, 0, 3, 9, 9)),
    ("one_u_face_no_v_face", (7.0, 0.53, 0.035), (0, 0, 0, 0, 0, 0, 1, 0)),
    ("smaller_than_any_face", (7.0, 0.5, 0.02), (0, 0, 0, 0, 0, 0, 0, 0)),
    ("outside_the_domain", (-5.0, 0.5, 0.3), (0, 0, 0, 0, 0, 0, 0, 0)),
]
# (x as a share of lx, y, radius)
_DISCS_SMALL = [
    ("inlet", (0.0, 0.25, 0.15), (3, 0, 0, 0, 0, 0, 6, 2)),
    ("outlet", (1.0, 0.25, 0.15), (0, 3, 0, 0, 0, 0, 6, 2)),
    ("taller_than_channel", (0.5, 0.25, 0.3), (0, 0, 5, 5, 4, 4, 27, 32)),
    ("corner_outlet_top", (1.0, 0.5, 0.12), (0, 1, 0, 2, 0, 1, 2, 2)),
]
DISCS = [Disc("248x16_" + n, 248, 16, 15.5, 1.0, cyl, cnt, True) for n, cyl, cnt in _DISCS_248]
for _nx in (16, 8):
    _lx = _nx * 0.1
    DISCS += [Disc(f"{_nx}x5_" + n, _nx, 5, _lx, 0.5, (cx * _lx, cy, r), cnt, _nx >= 16)
              for n, (cx, cy, r), cnt in _DISCS_SMALL]
DISC_BY_NAME = {d.name: d for d in DISCS}
assert len(DISC_BY_NAME) == len(DISCS)
DEVICE_DISCS = [d for d in DISCS if d.device]
DISC_SCHEME = ref.QUICK
PROFILES = (ref.UNIFORM, ref.PARABOLIC)
INLET = 0.8


def disc_grid(d):
    return ref.Grid(d.nx, d.ny, d.lx, d.ly, NU, d.cyl)


def face_counts(g):
    ou, ov = ref.obstacle_faces(g)
    return (int(ou[:, 0].sum()), int(ou[:, g.nx].sum()), int(ou[0].sum()), int(ou[g.ny - 1].sum()),
            int(ov[0].sum()), int(ov[g.ny].sum()), int(ou.sum()), int(ov.sum()))


def corrector_state(g, seed, dt_sub):
    """(u*, v*, p', p): CFL-scaled velocities and O(1) pressures, independent."""
    rng = np.random.default_rng(seed)
    us = (rng.uniform(-1, 1, (g.ny, g.nx + 1)) * 0.6 * g.dx / dt_sub).astype(np.float32)
    vs = (rng.uniform(-1, 1, (g.ny + 1, g.nx)) * 0.6 * g.dy / dt_sub).astype(np.float32)
    pp = rng.uniform(-1, 1, (g.ny, g.nx)).astype(np.float32)
    p = rng.uniform(-1, 1, (g.ny, g.nx)).astype(np.float32)
    return us, vs, pp, p


def disc_predicted(d):
    def make():
        g = disc_grid(d)
        u, v, p = random_state(g, 7500, DT_SUB)
        return (u, v, p) + ref.predict(g, u, v, DT_SUB, DISC_SCHEME)
    return _frozen(("disc_predict", d.name), make)


def disc_corrected(d, profile):
    def make():
        g = disc_grid(d)
        us, vs, pp, p = corrector_state(g, 7600, DT_SUB)
        return (us, vs, pp, p) + ref.correct(g, us, vs, pp, p, DT_SUB, INLET, profile)
    return _frozen(("disc_correct", d.name, profile), make)


# ------------------------------------------------------------- extreme values
FLAVOURS = ("huge", "tiny", "nonfinite")
# 12 x 7 stays with the restatement (a model refuses the width); 16 x 7 runs beside it
EXTREME_SHAPES = [(248, 17), (12, 7), (16, 7)]
EXTREME_DEVICE_SHAPES = [s for s in EXTREME_SHAPES if on_device(*s)]
CORRECTOR_SHAPE = (248, 17)
NONFINITE_CAP = 0.10
SUBNORMAL_SHARE = 0.05
# `tiny`: spacings of 4 (pow2) / 3 and 5 (div) and dt_sub = 2, so that the rhs
# quotient does not scale the 1e-39 .. 1e-37 velocities back into normal range
TINY_DT = 2.0
_NONFINITE_WORDS = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf))


def extreme_grid(nx, ny, flavour, path):
    if flavour == "tiny":
        lx, ly = (4.0 * nx, 4.0 * ny) if path == "pow2" else (3.0 * nx, 5.0 * ny)
        return ref.Grid(nx, ny, lx, ly, NU, None), TINY_DT
    lx, ly = spacing(nx, ny, path)
    return ref.Grid(nx, ny, lx, ly, NU, None), DT_SUB


def extreme_path(nx, ny, flavour, scheme):
    """Both division paths over the schemes and flavours of a shape."""
    return PATHS[(scheme + FLAVOURS.index(flavour) + (nx // 4)) % 2]


def _tiny(rng, shape):
    mag = np.power(10.0, rng.uniform(-39.0, -37.0, shape))
    return (np.where(rng.uniform(0, 1, shape) < 0.5, -mag, mag)).astype(np.float32)


def _sparse_huge(rng, a):
    """Finite words of 1e30 up to 3.3e38, either sign, at one word in 100 (at
    least four), seeded; returns their mask."""
    n = max(4, a.size // 100)
    hit = np.zeros(a.size, bool)
    hit[rng.choice(a.size, n, replace=False)] = True
    hit = hit.reshape(a.shape)
    mag = np.minimum(np.power(10.0, rng.uniform(30.0, 38.6, a.shape)), 3.3e38)
    big = np.where(rng.uniform(0, 1, a.shape) < 0.5, -mag, mag).astype(np.float32)
    a[hit] = big[hit]
    return hit


def nonfinite_positions(nx, ny, rows, cols, rng):
    """(j, i) of the planted words in a field of `rows` x `cols`: one word in
    400 at seeded positions, plus a word on each side of the wave seam (columns
    246 .. 249) and of a segment seam (rows R-1, R and the last segment's start)
    and on the first and the last column.  A grid under 400 cells takes the
    first and the last column only: one interior word spoils a tenth of it."""
    mid = rows // 2
    edge = {(1 + mid % (rows - 2), 0), (1 + (mid + 2) % (rows - 2), cols - 1)}
    if nx * ny < 400:
        return sorted(edge)[:1] if cols == nx else sorted(edge)   # v: column 0 only
    n = max(1, rows * cols // 400)
    pos = {(int(rng.integers(0, rows)), int(rng.integers(0, cols))) for _ in range(n)}
    geo = geometry(nx, ny)
    seam_rows = sorted({r for r in (geo.R - 1, geo.R, geo.starts[-1]) if 1 <= r < rows - 1})
    for k, i in enumerate((246, 247, 248, 249)):
        if i < cols - 1:
            pos.add((1 + (mid + 3 * k) % (rows - 2), i))
    for k, j in enumerate(seam_rows):
        pos.add((j, 2 + (5 * k + 3) % (cols - 4)))
    return sorted(pos | edge)


def _plant_nonfinite(rng, a, nx, ny, first=0):
    for k, (j, i) in enumerate(nonfinite_positions(nx, ny, a.shape[0], a.shape[1], rng)):
        a[j, i] = _NONFINITE_WORDS[(k + first) % 3]


def extreme_state(g, flavour, seed, dt_sub):
    """(u, v, p) for the predictor."""
    rng = np.random.default_rng([seed, FLAVOURS.index(flavour)])
    if flavour == "tiny":
        u, v = _tiny(rng, (g.ny, g.nx + 1)), _tiny(rng, (g.ny + 1, g.nx))
        p = rng.uniform(-1, 1, (g.ny, g.nx)).astype(np.float32)
        return u, v, p
    u, v, p = random_state(g, seed, dt_sub)
    if flavour == "huge":
        _sparse_huge(rng, u)
        _sparse_huge(rng, v)
    else:
        _plant_nonfinite(rng, u, g.nx, g.ny)
        _plant_nonfinite(rng, v, g.nx, g.ny, first=2)
    return u, v, p


def extreme_predicted(nx, ny, flavour, scheme):
    """(g, dt_sub, u, v, p, u*, v*, rhs), computed once."""
    def make():
        g, dt_sub = extreme_grid(nx, ny, flavour, extreme_path(nx, ny, flavour, scheme))
        u, v, p = extreme_state(g, flavour, 7700 + scheme, dt_sub)
        return (g, dt_sub, u, v, p) + ref.predict(g, u, v, dt_sub, scheme)
    return _frozen(("extreme_predict", nx, ny, flavour, scheme), make)


# `huge` in the corrector: dt_sub = 1, so that dt_sub / dx > 1 and a p' step of
# 1e38 leaves f32's range; p takes p' at the planted cells, so p + p' does too
HUGE_CORRECT_DT = 1.0


def extreme_corrected(flavour, path):
    """(g, dt_sub, u*, v*, p', p, u, v, p_new) on CORRECTOR_SHAPE."""
    def make():
        nx, ny = CORRECTOR_SHAPE
        g, dt_sub = extreme_grid(nx, ny, flavour, path)
        rng = np.random.default_rng([7800, FLAVOURS.index(flavour), PATHS.index(path)])
        if flavour == "tiny":
            us, vs = _tiny(rng, (ny, nx + 1)), _tiny(rng, (ny + 1, nx))
            pp, p = _tiny(rng, (ny, nx)), _tiny(rng, (ny, nx))
        else:
            if flavour == "huge":
                dt_sub = HUGE_CORRECT_DT
            us, vs, pp, p = (a.copy() for a in corrector_state(g, 7800, DT_SUB))
            if flavour == "huge":
                _sparse_huge(rng, us)
                _sparse_huge(rng, vs)
                hit = _sparse_huge(rng, pp)
                p[hit] = pp[hit]
            else:
                for k, a in enumerate((us, vs, pp)):
                    _plant_nonfinite(rng, a, nx, ny, first=k)
        return (g, dt_sub, us, vs, pp, p) + ref.correct(g, us, vs, pp, p, dt_sub, INLET, ref.PARABOLIC)
    return _frozen(("extreme_correct", flavour, path), make)


def subnormal_share(a):
    a = np.abs(np.asarray(a, np.float32))
    return float(np.count_nonzero((a > 0) & (a < np.finfo(np.float32).tiny))) / a.size


def nonfinite_share(a):
    return float(np.count_nonzero(~np.isfinite(a))) / np.size(a)


# ------------------------------------------------- the update's begin / end
# k_script_begin / k_script_end: nu + nv flat words, 1024 to a block, a thread
# strides by 256.
BLOCK_WORDS, THREAD_STRIDE = 1024, 256


def words(nx, ny):
    """(nu, nv)."""
    return (nx + 1) * ny, nx * (ny + 1)


def _search(pred, nx_max=64, ny_max=2048):
    """The admissible grid (nx % 8 == 0, 16 <= nx <= nx_max, ny >= 4) of the
    fewest words that satisfies pred(nu, nv)."""
    best = None
    for nx in range(16, nx_max + 1, 8):
        for ny in range(4, ny_max + 1):
            nu, nv = words(nx, ny)
            if pred(nu, nv) and (best is None or nu + nv < sum(words(*best))):
                best = (nx, ny)
                break
    return best


UPDATE_GRIDS = {
    # fewer words than one thread stride (8 x 4 has 76; a model refuses the width)
    "one_stride": (16, 4),
    # an exact multiple of the block, the u|v boundary mid-block (8 x 120 has
    # exactly 2048; a model refuses the width)
    "block_multiple": _search(lambda nu, nv: (nu + nv) % BLOCK_WORDS == 0),
    # one word into the last block
    "one_past_a_block": _search(lambda nu, nv: (nu + nv) % BLOCK_WORDS == 1),
    # the u|v boundary on a thread stride
    "boundary_on_a_stride": _search(lambda nu, nv: nu % THREAD_STRIDE == 0),
}
UPDATE_SOLVER = 5
UPDATE_SCHEME = ref.QUICK
UPDATE_PROFILE = ref.PARABOLIC
UPDATE_TARGET = 1.0
UPDATE_DT_USER = 0.5
UPDATE_STEP = 7
UPDATE_SUBSTEPS = 2
# dt at the start: above the CFL quotient of the seeded flow (about 0.11) but
# within 1.1 of it, so dt_next IS 0.5 min(dx, dy) / maxVel and the device's
# maximum is checked by value; with zero velocities dt_user itself, which the
# 1.1 limit then leaves alone
UPDATE_DT = 0.11
PLANT = 3.0     # the planted |uOld - u| or |vOld - v|; the flow's own stay under 1


def plant_words(nx, ny):
    """{name: (field, flat index in the field, flat index over u|v)}."""
    nu, nv = words(nx, ny)
    return {"first_u": ("u_prev", 0, 0), "last_u": ("u_prev", nu - 1, nu - 1),
            "first_v": ("v_prev", 0, nu), "last_v": ("v_prev", nv - 1, nu + nv - 1)}


PLANTS = ("first_u", "last_u", "first_v", "last_v")
# beside the four: every velocity zero (max_vel == 0: the dt rule returns
# dt_user); zero everywhere with the last word planted (the only non-zero
# maximum sits in the last word of the last block); a NaN in the first word (a
# lane's first delta is NaN: no maximum takes it)
SPECIALS = ("all_zero", "zero_but_last_word", "nan_first_word")
UPDATE_CASES = [(gname, k) for gname in UPDATE_GRIDS for k in PLANTS + SPECIALS]


def update_grid(gname):
    nx, ny = UPDATE_GRIDS[gname]
    return ref.Grid(nx, ny, nx / 16.0 * 1.5, ny / 16.0 * 1.5, NU, None)


def update_start(gname, kind):
    """(g, start state, target inlet velocity)."""
    g = update_grid(gname)
    nx, ny = g.nx, g.ny
    if kind in ("all_zero", "zero_but_last_word"):
        u, v = np.zeros((ny, nx + 1), np.float32), np.zeros((ny + 1, nx), np.float32)
        p = np.zeros((ny, nx), np.float32)
        up, vp = u.copy(), v.copy()
        target = 0.0
    else:
        rng = np.random.default_rng([8000, nx, ny])
        y = (np.arange(ny) + 0.5) / ny
        u = (0.4 * (4 * y * (1 - y))[:, None] + 0.02 * rng.uniform(-1, 1, (ny, nx + 1))).astype(np.float32)
        v = (0.02 * rng.uniform(-1, 1, (ny + 1, nx))).astype(np.float32)
        p = rng.uniform(-1, 1, (ny, nx)).astype(np.float32)
        up = (u * np.float32(0.99)).astype(np.float32)
        vp = (v * np.float32(0.99)).astype(np.float32)
        target = UPDATE_TARGET
    pw = plant_words(nx, ny)
    if kind in PLANTS or kind == "zero_but_last_word":
        f, k, _ = pw["last_v" if kind == "zero_but_last_word" else kind]
        a, cur = (up, u) if f == "u_prev" else (vp, v)
        # uOld = 2 u - uPrev = u + PLANT there; the boundary pass leaves 0
        a.reshape(-1)[k] = np.float32(cur.reshape(-1)[k] - np.float32(PLANT))
    elif kind == "nan_first_word":
        up.reshape(-1)[0] = np.nan
    dt = UPDATE_DT_USER if target == 0.0 else UPDATE_DT
    st = dict(u=u, v=v, p=p, u_prev=up, v_prev=vp, dt=dt, substep_count=UPDATE_SUBSTEPS,
              step_count=UPDATE_STEP)
    return g, st, target


def updated(gname, kind):
    """(g, start, target, new state, report) of the restatement, computed once."""
    def make():
        g, st, target = update_start(gname, kind)
        new, rep = upd.update(g, st, UPDATE_SCHEME, UPDATE_PROFILE, target, UPDATE_DT_USER,
                              UPDATE_SOLVER)
        return g, st, target, new, rep
    return _frozen(("update", gname, kind), make)
