"""CPU: pins the restatement of the reference's Mesh tab drawing
(tests/_raster_ref.py) against hand-listed pixels, the host-only parts of the
rasteriser ABI (include/cfd.h: cfd_mesh_view_size, the limits refused before
any device is touched) against it, and proves on the restatement's writer
maps that the cases of tests/test_gpu_mesh_raster.py exercise what they claim.

The pixel lists were traced by hand through drawing.rs:2-41 / :45-78."""
import ctypes as C
import math

import numpy as np
import pytest

import _raster_cases as rc
import _raster_ref as rr
import quad_mesh_ref as qr


def _line(x0, y0, x1, y1, w=6, h=6):
    img = rr.Image(w, h, track=True)
    rr.draw_line(img, x0, y0, x1, y1, rr.BLACK, "line")
    lit = {(int(x), int(y)) for y, x in zip(*np.nonzero(img.pixels[:, :, 3]))}
    assert lit == set(img.writers)
    return sorted(lit)


LINES = {
    # one per octant, named by the direction of travel
    "east_south_shallow": ((0, 0, 5, 2), [(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2)]),
    "east_south_steep": ((0, 0, 2, 5), [(0, 0), (0, 1), (1, 2), (1, 3), (2, 4), (2, 5)]),
    "west_south_steep": ((5, 0, 3, 5), [(3, 4), (3, 5), (4, 2), (4, 3), (5, 0), (5, 1)]),
    "west_south_shallow": ((5, 0, 0, 2), [(0, 2), (1, 2), (2, 1), (3, 1), (4, 0), (5, 0)]),
    "west_north_shallow": ((5, 5, 0, 3), [(0, 3), (1, 3), (2, 4), (3, 4), (4, 5), (5, 5)]),
    "west_north_steep": ((5, 5, 3, 0), [(3, 0), (3, 1), (4, 2), (4, 3), (5, 4), (5, 5)]),
    "east_north_steep": ((0, 5, 2, 0), [(0, 4), (0, 5), (1, 2), (1, 3), (2, 0), (2, 1)]),
    "east_north_shallow": ((0, 5, 5, 3), [(0, 5), (1, 5), (2, 4), (3, 4), (4, 3), (5, 3)]),
    "horizontal": ((1, 2, 4, 2), [(1, 2), (2, 2), (3, 2), (4, 2)]),
    "vertical_upwards": ((3, 4, 3, 1), [(3, 1), (3, 2), (3, 3), (3, 4)]),
    "single_point": ((2, 2, 2, 2), [(2, 2)]),
    # starts at (-3, -2): (-3,-2) (-2,-1) (-1,-1) are clipped, each on its own
    "from_negative": ((-3, -2, 2, 1), [(0, 0), (1, 0), (2, 1)]),
    # ends at (8, 6) beyond the 6 x 6 image: (6,5) (7,5) (8,6) are clipped
    "beyond_the_image": ((3, 3, 8, 6), [(3, 3), (4, 4), (5, 4)]),
}


@pytest.mark.parametrize("name", sorted(LINES))
def test_draw_line_pixels(name):
    args, want = LINES[name]
    assert _line(*args) == want


def _diamond(cx, cy, w=8, h=8):
    img = rr.Image(w, h, track=True)
    rr.draw_diamond(img, cx, cy, rr.ORANGE, "d")
    assert all(tuple(img.pixels[y, x]) == rr.ORANGE for x, y in img.writers)
    return sorted(img.writers)


def test_diamond_is_the_4x4_box_without_its_corners():
    box = {(x, y) for x in range(2, 6) for y in range(2, 6)}          # cx - 2 .. cx + 1
    want = sorted(box - {(2, 2), (5, 2), (2, 5), (5, 5)})
    assert len(want) == 12 and _diamond(4, 4) == want


@pytest.mark.parametrize("centre, want", [
    ((0, 0), [(0, 0), (0, 1), (1, 0)]),
    ((7, 0), [(5, 0), (6, 0), (6, 1), (7, 0), (7, 1)]),
    ((0, 7), [(0, 5), (0, 6), (0, 7), (1, 6), (1, 7)]),
    ((7, 7), [(5, 6), (5, 7), (6, 5), (6, 6), (6, 7), (7, 5), (7, 6), (7, 7)]),
])
def test_diamond_clipped_at_each_corner(centre, want):
    assert _diamond(*centre) == want


def test_diamond_corner_is_cx_minus_2_up_to_the_limit():
    """drawing.rs computes the box corner in f32; exact for |cx| <= 2^15."""
    for cx in (-2 ** 15, -1, 0, 1, 2 ** 15):
        assert int(np.floor(np.float32(cx) - np.float32(1.5))) == cx - 2


def test_colour_constants():
    from cfdamd import quad_mesh as qm
    want = {"TRANSPARENT": (0, 0, 0, 0), "BLACK": (0, 0, 0, 255),
            "LIGHT_BLUE": (0xAD, 0xD8, 0xE6, 255), "ORANGE": (255, 165, 0, 255)}
    for name, rgba in want.items():
        assert getattr(rr, name) == rgba and getattr(qm, name) == rgba, name


def test_vectorised_fill_is_contains_point():
    """The numpy fill of the restatement against the scalar contains_point
    (polygon.rs:81-103) pixel by pixel, holes included."""
    for name, (w, h) in (("two_holes", (31, 17)), ("concave", (23, 19)), ("quirk", (9, 7))):
        poly = rc.ref_polygon(name)
        px, py = rr.polygon_pixel_points(poly, w, h)
        inside = rr._contains(poly, px, py)
        for y in range(h):
            for x in range(w):
                assert inside[y, x] == poly.contains_point(qr.Point(px[y, x], py[y, x])), (x, y)
        assert inside.any() and not inside.all()


# ------------------------------------------------------------- host-only ABI

VIEW_SIZES = {
    #                 bbox (cx, cy, hw, hh)   panel            (w, h)
    "wide_panel": ((15.0, 5.0, 15.0, 5.0), (1270.0, 300.0), (900, 300)),
    "tall_panel": ((15.0, 5.0, 15.0, 5.0), (300.0, 900.0), (300, 100)),
    "equal_aspect": ((15.0, 5.0, 15.0, 5.0), (900.0, 300.0), (900, 300)),
    # 333.3 is not an f32; 333.3f * 0.7 = 233.3... truncates to 233
    "truncation": ((5.0, 5.0, 3.5, 5.0), (1000.5, 333.3), (233, 333)),
}


@pytest.mark.parametrize("name", sorted(VIEW_SIZES))
def test_mesh_view_size(name):
    from cfdamd import quad_mesh as qm
    box, panel, want = VIEW_SIZES[name]
    assert rr.mesh_view_size(rc.aabb(qr, *box), *panel) == want
    assert qm.mesh_view_size(rc.aabb(qm, *box), *panel) == want


def test_mesh_view_size_of_the_default_view():
    from cfdamd import quad_mesh as qm
    got = qm.mesh_view_size(rc.default(qm).bounding_box(), *rc.PANEL)
    assert got == rr.mesh_view_size(rc.ref_polygon("default").bounding_box(), *rc.PANEL) == (400, 133)


def _expect_einval(fn):
    from cfdamd import CfdError
    with pytest.raises(CfdError) as e:
        fn()
    assert e.value.code == -1, e.value


@pytest.mark.parametrize("w, h", [(0, 8), (1, 8), (16385, 8), (8, 0), (8, 1), (8, 16385)])
def test_sizes_outside_the_limits_are_einval(w, h):
    from cfdamd import quad_mesh as qm
    poly = rc.default(qm)
    tree = qm.tesselate(poly, *rc.COARSE)
    _expect_einval(lambda: qm.rasterize_polygon(poly, w, h))
    _expect_einval(lambda: qm.mesh_view_image(poly, None, w, h))
    _expect_einval(lambda: qm.rasterize_quad_tree(tree, w, h))


def test_null_arguments_are_einval():
    from cfdamd import _lib
    from cfdamd import quad_mesh as qm
    L = _lib.load()
    poly = rc.default(qm)
    tree = qm.tesselate(poly, *rc.COARSE)
    box = poly.bounding_box()._c()
    out = (C.c_uint8 * (8 * 8 * 4))(*([0x5A] * 256))
    w, h = C.c_size_t(77), C.c_size_t(77)
    E = _lib.CFD_EINVAL
    assert L.cfd_raster_polygon(None, 0, 8, 8, out, None) == E
    assert L.cfd_raster_polygon(poly._h, 0, 8, 8, None, None) == E
    assert L.cfd_raster_quadtree(None, None, 0, 8, 8, None, out, None) == E
    assert L.cfd_raster_quadtree(tree._h, None, 0, 8, 8, None, None, None) == E
    assert L.cfd_raster_mesh(None, C.byref(box), 0, 8, 8, None, out, None) == E
    assert L.cfd_raster_mesh_view(None, None, 0, 8, 8, out, None) == E
    assert L.cfd_raster_mesh_view(poly._h, None, 0, 8, 8, None, None) == E
    assert L.cfd_mesh_view_size(None, 4.0, 3.0, C.byref(w), C.byref(h)) == E
    assert L.cfd_mesh_view_size(C.byref(box), 4.0, 3.0, None, C.byref(h)) == E
    assert L.cfd_mesh_view_size(C.byref(box), 4.0, 3.0, C.byref(w), None) == E
    assert bytes(out) == bytes([0x5A] * 256) and (w.value, h.value) == (77, 77)   # nothing written


@pytest.mark.parametrize("box", [
    (15.0, 5.0, math.inf, 5.0), (math.nan, 5.0, 15.0, 5.0), (15.0, math.inf, 15.0, 5.0),
    (15.0, 5.0, 15.0, math.nan), (15.0, 5.0, 0.0, 5.0), (15.0, 5.0, 15.0, 0.0),
    (15.0, 5.0, -1.0, 5.0)])
def test_bad_bbox_is_einval(box):
    from cfdamd import quad_mesh as qm
    tree = qm.tesselate(rc.default(qm), *rc.COARSE)
    _expect_einval(lambda: qm.rasterize_quad_tree(tree, 16, 16, bbox=rc.aabb(qm, *box)))


def test_zero_area_polygon_bbox_is_einval():
    from cfdamd import quad_mesh as qm
    flat = qm.Polygon.new([qm.Point(0.0, 1.0), qm.Point(1.0, 1.0), qm.Point(2.0, 1.0)], [0, 1, 2])
    _expect_einval(lambda: qm.rasterize_polygon(flat, 16, 16))


def test_endpoint_beyond_the_limit_is_einval():
    """The tree spans 30 units; on a bbox 0.005 units wide a 16 x 16 image has
    scale 3000, so leaf corners map to 9e4 > 2^15 pixels.  One that stays
    within the limit on the same call path is refused only for want of a device."""
    from cfdamd import quad_mesh as qm
    tree = qm.tesselate(rc.default(qm), *rc.COARSE)
    tiny = rc.aabb(qm, 0.0, 0.0, 0.0025, 0.0025)
    assert (30.0 - -0.0025) * (15 / 0.005) > 2 ** 15
    _expect_einval(lambda: qm.rasterize_quad_tree(tree, 16, 16, bbox=tiny))


def test_valid_call_reaches_for_the_device():
    """Past the host checks the call goes to the device: an image where there
    is one, CFD_EHIP where there is none, never a quiet host fallback."""
    from cfdamd import CfdError
    from cfdamd import quad_mesh as qm
    try:
        img = qm.rasterize_polygon(rc.default(qm), 16, 16)
    except CfdError as e:
        assert e.code == -2
    else:
        assert img.shape == (16, 16, 4)


# ------------------------------------------- premises of the GPU test's cases

def test_premise_ordering_goes_both_ways():
    """On the coarse mesh at 120 x 41 some pixels end as a later cell's outline
    over an earlier cell's diamond, and some as a diamond over an earlier
    cell's outline: both halves of the key order decide pixels."""
    mesh = rc.ref_mesh()
    img = rr.rasterize_mesh_no_background(mesh, 120, 41, mesh.full_bounding_box(), track=True)
    line_over_diamond = diamond_over_line = 0
    for hist in img.writers.values():
        last = hist[-1]
        if last[0] == "outline" and any(t[0] == "diamond" and t[1] < last[1] for t in hist):
            line_over_diamond += 1
        if last[0] == "diamond" and any(t[0] == "outline" and t[1] < last[1] for t in hist):
            diamond_over_line += 1
    assert line_over_diamond >= 1 and diamond_over_line >= 1
    # and the same holds when everything collapses onto 2 x 2
    tiny = rr.rasterize_mesh_no_background(mesh, 2, 2, mesh.full_bounding_box(), track=True)
    assert len(tiny.writers) == 4 and all(len(h) > 1 for h in tiny.writers.values())


def test_premise_clamp_draws_row_0():
    """Quadtree over a bbox whose top edge cuts the first row of leaves: their
    top sides map to negative rows, `as usize` clamps them to row 0, and the
    pixels they set there are set by nothing else (drawn with `as isize`
    instead, the image loses them).  The polygon's own bbox at 120 x 41 has
    negative coordinates too (the tree's square overhangs it), but every
    pixel they clamp to is also drawn by the leaves that end at y = 0."""
    tree, poly = rc.ref_tree(), rc.ref_polygon("default")
    blank = np.zeros((41, 120, 4), np.uint8)
    clamped = rr.rasterize_quad_tree(tree, blank, rc.cut_bbox(qr)).pixels
    kept = rr.rasterize_quad_tree(tree, blank, rc.cut_bbox(qr), _via_usize=False).pixels
    only_by_clamp = np.any(clamped != kept, axis=2)
    assert only_by_clamp[0].sum() >= 1 and not only_by_clamp[1:].any()
    assert np.all(clamped[0][only_by_clamp[0]] == rr.BLACK)
    box = poly.bounding_box()
    scale = rr._scale(120, 41, box)
    assert (tree.boundary.top_left().y - box.top_left().y) * scale < -1.0


def test_premise_quirk_edges_are_not_the_ring():
    poly = rc.ref_polygon("quirk")
    ring = [poly.vertex_buffer[i] for i in poly.vertices]
    ring_edges = {((a.x, a.y), (b.x, b.y)) for a, b in zip(ring, ring[1:] + ring[:1])}
    drawn = {((a.x, a.y), (b.x, b.y)) for a, b in poly.edges()}
    assert ((0.0, 0.0), (4.0, 3.0)) in drawn and drawn != ring_edges
    # and it shows: a diagonal's pixel inside the filled rectangle is black
    img = rr.rasterize_polygon(poly, 64, 64, track=True)
    assert any(h[0] == ("fill",) and h[-1][0] == "edge" for h in img.writers.values())


def test_premise_pixel_centres_on_edges():
    """At 64 x 64 column 63 maps exactly onto the rectangle's right edge and
    row 21 onto its bottom edge; `p.x < x_intersect` is strict, so the point
    on the right edge is outside."""
    poly = rc.ref_polygon("on_edge")
    x, y, w, h = rc.ON_EDGE_RECT
    px, py = rr.polygon_pixel_points(poly, 64, 64)
    assert px[0, 63] == x + w and py[21, 0] == y + h
    assert not poly.contains_point(qr.Point(px[10, 63], py[10, 63]))
    assert poly.contains_point(qr.Point(px[10, 62], py[10, 62]))


def test_premise_small_bbox_and_empty_mesh():
    mesh = rc.ref_mesh()
    box = rc.small_bbox(qr)
    scale = rr._scale(120, 41, box)
    xs = (mesh.cell_centers_x - mesh.cell_half_width - box.top_left().x) * scale
    assert xs.min() < -1.0 and xs.max() > 120.0          # negative and beyond the image
    assert rc.ref_mesh(rc.COARSE, "far_rect").cell_centers_x.size == 0
