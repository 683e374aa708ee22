"""GPU: the Mesh tab's images drawn by the HIP kernels (csrc/cfd_mesh_raster.hip)
against the restatement of the reference's sequential drawing
(tests/_raster_ref.py), byte for byte.  tests/test_mesh_raster_cpu.py proves
that these cases contain what they are here for (both directions of the
draw order, the `as usize` clamp, the edges() quirk, pixel centres on edges).

Where the issue's empty-mesh case pointed at test_gpu_mesh.py's
empty-filter test, which builds no mesh (it checks a refusal), the 0-cell
mesh here is the default polygon's tree filtered by a polygon far from it."""
import functools
import math

import numpy as np
import pytest

import _raster_cases as rc
import _raster_ref as rr

pytestmark = pytest.mark.gpu


def _same(got, want):
    want = np.asarray(want)
    assert got.dtype == np.uint8 and got.shape == want.shape
    diff = np.argwhere(np.any(got != want, axis=2))
    assert diff.size == 0, f"{len(diff)} pixels differ, first (y, x) = {diff[0]}: " \
                           f"{got[tuple(diff[0])]} != {want[tuple(diff[0])]}"


def _ms_ok():
    from cfdamd import quad_mesh as qm
    assert qm.last_raster_ms is not None and math.isfinite(qm.last_raster_ms)
    assert qm.last_raster_ms >= 0.0


@functools.lru_cache(maxsize=None)
def _gpu(params=rc.COARSE, polygon="default"):
    """(polygon, tree, mesh) of the product, built once and shared."""
    from cfdamd import quad_mesh as qm
    poly = rc.default(qm)
    tree = qm.tesselate(poly, *params)
    keep = poly if polygon == "default" else rc.far_rect(qm)
    return poly, tree, qm.Mesh.from_quad_tree(tree, keep)


@pytest.mark.parametrize("size", rc.POLYGON_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(rc.POLYGONS))
def test_polygon(name, size):
    from cfdamd import quad_mesh as qm
    w, h = size
    got = qm.rasterize_polygon(rc.POLYGONS[name](qm), w, h)
    _ms_ok()
    _same(got, rc.ref_polygon_image(name, w, h))
    if size != (2, 2):
        assert np.all(got == rr.LIGHT_BLUE, axis=2).any() and np.all(got == rr.BLACK, axis=2).any()


def test_quadtree_on_its_own_boundary():
    from cfdamd import quad_mesh as qm
    _, tree, _ = _gpu()
    got = qm.rasterize_quad_tree(tree, 96, 96)
    _ms_ok()
    _same(got, rr.rasterize_quad_tree_no_background(rc.ref_tree(), 96, 96).pixels)
    assert set(map(tuple, got.reshape(-1, 4))) == {rr.TRANSPARENT, rr.BLACK}


def test_quadtree_over_the_polygon_image():
    """120 x 41 on the polygon's bbox: the tree's bounding square overhangs it,
    so leaf corners are negative before the clamp and far beyond the image."""
    from cfdamd import quad_mesh as qm
    poly, tree, _ = _gpu()
    bg = qm.rasterize_polygon(poly, 120, 41)
    before = bg.copy()
    got = qm.rasterize_quad_tree(tree, background=bg, bbox=poly.bounding_box())
    assert np.array_equal(bg, before)
    _same(got, rr.rasterize_quad_tree(rc.ref_tree(), rc.ref_polygon_image("default", 120, 41),
                                      rc.ref_polygon("default").bounding_box()).pixels)


@pytest.mark.parametrize("box", ["polygon", "cut"])
def test_quadtree_over_a_random_background(box):
    """`cut`: the bbox whose top edge halves the first row of leaves, where the
    `as usize` clamp alone draws part of row 0 (test_premise_clamp_draws_row_0)."""
    from cfdamd import quad_mesh as qm
    import quad_mesh_ref as qr
    poly, tree, _ = _gpu()
    bg = rc.random_background(120, 41)
    gb = poly.bounding_box() if box == "polygon" else rc.cut_bbox(qm)
    rb = rc.ref_polygon("default").bounding_box() if box == "polygon" else rc.cut_bbox(qr)
    got = qm.rasterize_quad_tree(tree, background=bg, bbox=gb)
    _same(got, rr.rasterize_quad_tree(rc.ref_tree(), bg, rb).pixels)
    assert np.any(np.all(got == bg, axis=2)) and np.any(np.any(got != bg, axis=2))


def test_mesh_on_its_full_bounding_box():
    from cfdamd import quad_mesh as qm
    _, _, mesh = _gpu()
    got = qm.rasterize_mesh_no_background(mesh, 120, 41, mesh.full_bounding_box())
    _ms_ok()
    ref = rc.ref_mesh()
    _same(got, rr.rasterize_mesh_no_background(ref, 120, 41, ref.full_bounding_box()).pixels)
    assert {rr.TRANSPARENT, rr.BLACK, rr.ORANGE} == set(map(tuple, got.reshape(-1, 4)))


def test_mesh_on_a_smaller_bbox_over_a_background():
    """Cells map to negative and beyond-image pixels: per-pixel clipping, no clamp."""
    from cfdamd import quad_mesh as qm
    import quad_mesh_ref as qr
    _, _, mesh = _gpu()
    bg = rc.random_background(120, 41, seed=11)
    got = qm.rasterize_mesh(mesh, bg, rc.small_bbox(qm))
    _same(got, rr.rasterize_mesh(rc.ref_mesh(), bg, rc.small_bbox(qr)).pixels)
    _same(qm.rasterize_mesh_no_background(mesh, 120, 41, rc.small_bbox(qm)),
          rr.rasterize_mesh_no_background(rc.ref_mesh(), 120, 41, rc.small_bbox(qr)).pixels)


def test_mesh_at_2x2():
    """Every primitive lands on four pixels: the order decides everything."""
    from cfdamd import quad_mesh as qm
    _, _, mesh = _gpu()
    ref = rc.ref_mesh()
    _same(qm.rasterize_mesh_no_background(mesh, 2, 2, mesh.full_bounding_box()),
          rr.rasterize_mesh_no_background(ref, 2, 2, ref.full_bounding_box()).pixels)


def test_mesh_of_0_cells_is_the_background():
    from cfdamd import quad_mesh as qm
    poly, _, _ = _gpu()
    _, _, empty = _gpu(rc.COARSE, "far_rect")
    assert empty.num_cells == 0 and rc.ref_mesh(rc.COARSE, "far_rect").cell_centers_x.size == 0
    bg = rc.random_background(33, 9, seed=3)
    _same(qm.rasterize_mesh(empty, bg, poly.bounding_box()), bg)
    blank = qm.rasterize_mesh_no_background(empty, 33, 9, poly.bounding_box())
    assert not blank.any()
    _same(qm.mesh_view_image(poly, empty, 67, 23), rc.ref_polygon_image("default", 67, 23))


def test_mesh_view_is_the_two_rasterisers_composed():
    from cfdamd import quad_mesh as qm
    poly, _, mesh = _gpu()
    w, h = 120, 41
    got = qm.mesh_view_image(poly, mesh, w, h)
    _ms_ok()
    rp = rc.ref_polygon("default")
    _same(got, rr.rasterize_mesh(rc.ref_mesh(), rc.ref_polygon_image("default", w, h),
                                 rp.bounding_box()).pixels)
    _same(got, rr.mesh_view_image(rp, rc.ref_mesh(), w, h).pixels)
    _same(got, qm.rasterize_mesh(mesh, qm.rasterize_polygon(poly, w, h), poly.bounding_box()))
    _same(qm.mesh_view_image(poly, None, w, h), rc.ref_polygon_image("default", w, h))


def test_mesh_view_at_the_default_parameters():
    """default_polygon at MeshParams::default on the image draw_sketch makes
    for a 400 x 300 panel: the workload's own shape at a small panel."""
    from cfdamd import quad_mesh as qm
    poly, _, mesh = _gpu(rc.DEFAULT)
    w, h = qm.mesh_view_size(poly.bounding_box(), *rc.PANEL)
    assert (w, h) == (400, 133)
    ref = rc.ref_mesh(rc.DEFAULT)
    assert mesh.num_cells == ref.cell_centers_x.size
    _same(qm.mesh_view_image(poly, mesh, w, h),
          rr.mesh_view_image(rc.ref_polygon("default"), ref, w, h).pixels)
    box = mesh.full_bounding_box()
    w2, h2 = qm.mesh_view_size(box, *rc.PANEL)          # the second image of draw_sketch
    _same(qm.rasterize_mesh_no_background(mesh, w2, h2, box),
          rr.rasterize_mesh_no_background(ref, w2, h2, ref.full_bounding_box()).pixels)


def test_every_rasteriser_repeats_itself():
    """Atomics leave nothing order-dependent behind: a second call gives the same bytes."""
    from cfdamd import quad_mesh as qm
    poly, tree, mesh = _gpu()
    bg = rc.random_background(120, 41, seed=5)
    calls = [lambda: qm.rasterize_polygon(poly, 67, 23),
             lambda: qm.rasterize_quad_tree(tree, 96, 96),
             lambda: qm.rasterize_quad_tree(tree, background=bg, bbox=poly.bounding_box()),
             lambda: qm.rasterize_mesh(mesh, bg, rc.small_bbox(qm)),
             lambda: qm.rasterize_mesh_no_background(mesh, 2, 2, mesh.full_bounding_box()),
             lambda: qm.mesh_view_image(poly, mesh, 120, 41)]
    for call in calls:
        first = call()
        assert np.array_equal(first, call())
        _ms_ok()
