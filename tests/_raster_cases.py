"""Shapes shared by tests/test_mesh_raster_cpu.py and tests/test_gpu_mesh_raster.py.

Every builder takes the module (cfdamd.quad_mesh or quad_mesh_ref) and returns
its Polygon, so the product and the restatement get the same geometry.  The
reference objects and images are built once per process and shared; nothing
may write to them.
"""
import functools

import numpy as np


def default(m):
    return m.default_polygon()


def concave(m):                      # as tests/test_gpu_mesh.py builds it
    P = m.Point
    return m.Polygon.new([P(0.0, 0.0), P(4.0, 0.0), P(4.0, 3.0), P(2.0, 1.0), P(0.0, 3.0)],
                         [0, 1, 2, 3, 4])


def two_holes(m):                    # as tests/test_gpu_mesh.py builds it
    poly = m.Polygon.new_rect(0.0, 0.0, 12.0, 6.0)
    poly.add_hole(m.Polygon.new_rect(2.0, 2.0, 2.0, 2.0))
    poly.add_hole(m.Polygon.new_polygon(m.Point(8.0, 3.0), 1.5, 6, 0.3))
    return poly


# `vertices` is a permutation of the buffer: contains_point walks the ring
# (0,0) (4,0) (4,3) (0,3), edges() pairs vertex_buffer[i] with
# vertex_buffer[(i + 1) % 4] for the index VALUE i (polygon.rs:186-196)
QUIRK_POINTS = [(0.0, 0.0), (4.0, 3.0), (4.0, 0.0), (0.0, 3.0)]
QUIRK_INDICES = [0, 2, 1, 3]


def quirk(m):
    return m.Polygon.new([m.Point(x, y) for x, y in QUIRK_POINTS], QUIRK_INDICES)


# At 64 x 64 the scale is min(63 / 63, 63 / 21) = 1: pixel column 63 maps to
# x = 63 / 1 + 1 = 64, the right edge, and pixel row 21 to y = 21 / 1 + 2 = 23,
# the bottom edge, both exactly.
ON_EDGE_RECT = (1.0, 2.0, 63.0, 21.0)


def on_edge(m):
    return m.Polygon.new_rect(*ON_EDGE_RECT)


def far_rect(m):                     # touches no leaf of the default polygon's tree
    return m.Polygon.new_rect(100.0, 100.0, 1.0, 1.0)


POLYGONS = {"default": default, "concave": concave, "two_holes": two_holes, "quirk": quirk,
            "on_edge": on_edge}
# 67 x 23: a width that is neither a wave nor a power of two, scale set by the height
POLYGON_SIZES = [(67, 23), (2, 2), (64, 64)]

COARSE = (0.3, 1.0)                  # the quadtree and mesh cases
DEFAULT = (0.1, 0.5)                 # views/mesh_view.rs MeshParams::default
PANEL = (400.0, 300.0)               # the default-sized case's available panel


def aabb(m, cx, cy, hw, hh):
    return m.AABB(m.Point(cx, cy), hw, hh)


# a bbox smaller than the mesh: cells map to negative and beyond-image pixels
def small_bbox(m):
    return aabb(m, 15.0, 5.0, 10.0, 3.0)


# a bbox whose top edge cuts the first row of unit leaves in half: their top
# sides map to -0.5 * scale, which `as usize` clamps to row 0
def cut_bbox(m):
    return aabb(m, 15.0, 5.25, 15.0, 4.75)


@functools.lru_cache(maxsize=None)
def ref_polygon(name):
    import quad_mesh_ref as qr
    return {**POLYGONS, "far_rect": far_rect}[name](qr)


@functools.lru_cache(maxsize=None)
def ref_tree(params=COARSE):
    import quad_mesh_ref as qr
    return qr.tesselate(ref_polygon("default"), *params)


@functools.lru_cache(maxsize=None)
def ref_mesh(params=COARSE, polygon="default"):
    import quad_mesh_ref as qr
    return qr.Mesh(ref_tree(params), ref_polygon(polygon))


@functools.lru_cache(maxsize=None)
def ref_polygon_image(name, w, h):
    import _raster_ref as rr
    img = rr.rasterize_polygon(ref_polygon(name), w, h).pixels
    img.setflags(write=False)
    return img


def random_background(w, h, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
