"""Pure-Python restatement of the reference's Mesh tab drawing — TEST
INFRASTRUCTURE ONLY: src/utils/drawing.rs, polygon_rasterizer.rs,
quad_tree_rasterizer.rs, mesh_rasterizer.rs and the image-size rule of
views/mesh_view.rs:75-88, over the mesher restatement oracle/quad_mesh_ref.py.

It draws as the reference does, sequentially, last writer wins, in Python
floats (IEEE double) and Python ints with Rust's cast rules spelled out
(as_usize, as_isize).  The polygon fill alone is vectorised over the pixels
with numpy (the same f64 expressions in the same order, elementwise);
tests/test_mesh_raster_cpu.py pins it against the scalar contains_point.

An Image can keep, per pixel, the list of primitives that wrote it, in order
(`track=True`): image.writers[(x, y)] is a list of tags, the last one the
"last writer".  Tags: ("fill",), ("edge", k), ("leaf", k, side),
("outline", cell, side), ("diamond", cell, q).
"""
from __future__ import annotations

import math

import numpy as np

import quad_mesh_ref as qr

# egui::Color32 constants as (r, g, b, a)
TRANSPARENT = (0, 0, 0, 0)
BLACK = (0, 0, 0, 255)
LIGHT_BLUE = (173, 216, 230, 255)      # from_rgb(0xAD, 0xD8, 0xE6)
ORANGE = (255, 165, 0, 255)            # from_rgb(255, 165, 0)


# ------------------------------------------------------------ Rust's casts

def as_usize(f: float) -> int:
    """`f64 as usize`: NaN -> 0, saturating, truncating."""
    if f != f or f <= 0.0:
        return 0
    if f >= 2.0 ** 64:
        return 2 ** 64 - 1
    return int(f)


def as_isize(f: float) -> int:
    """`f64 as isize`: NaN -> 0, saturating, truncating."""
    if f != f:
        return 0
    if f >= 2.0 ** 63:
        return 2 ** 63 - 1
    if f <= -(2.0 ** 63):
        return -(2 ** 63)
    return int(f)


def usize_as_isize(u: int) -> int:
    """`usize as isize`: reinterpretation."""
    return u - 2 ** 64 if u >= 2 ** 63 else u


# ------------------------------------------------------------------ image

class Image:
    def __init__(self, width: int, height: int, pixels=None, track: bool = False):
        self.width, self.height = width, height
        self.pixels = (np.zeros((height, width, 4), np.uint8) if pixels is None
                       else np.array(pixels, np.uint8).reshape(height, width, 4))
        self.writers = {} if track else None

    def set(self, x: int, y: int, color, tag) -> None:
        self.pixels[y, x] = color
        if self.writers is not None:
            self.writers.setdefault((x, y), []).append(tag)

    def last_writer(self, x: int, y: int):
        w = self.writers.get((x, y))
        return w[-1] if w else None


# -------------------------------------------------------------- drawing.rs

def draw_line(img: Image, x0: int, y0: int, x1: int, y1: int, color, tag=None) -> None:   # :2-41
    width, height = img.width, img.height
    dx = abs(x1 - x0)
    dy = -abs(y1 - y0)
    sx = 1 if x0 < x1 else -1
    sy = 1 if y0 < y1 else -1
    err = dx + dy
    x, y = x0, y0
    while True:
        if 0 <= x < width and 0 <= y < height:
            img.set(x, y, color, tag)
        if x == x1 and y == y1:
            break
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x += sx
        if e2 <= dx:
            err += dx
            y += sy


def draw_diamond(img: Image, cx: int, cy: int, color, tag=None) -> None:   # :45-78
    size = 4
    f32 = np.float32
    center = (f32(size) - f32(1.0)) / f32(2.0)
    top_left_x = as_isize(float(np.floor(f32(cx) - center)))
    top_left_y = as_isize(float(np.floor(f32(cy) - center)))
    for j in range(size):
        for i in range(size):
            local_x, local_y = f32(i), f32(j)
            if abs(local_x - center) + abs(local_y - center) <= center + f32(0.5):
                x, y = top_left_x + i, top_left_y + j
                if 0 <= x < img.width and 0 <= y < img.height:
                    img.set(x, y, color, tag)


# -------------------------------------------------------------- the closures

def _scale(width: int, height: int, bbox) -> float:
    return qr._fmin(float(width - 1) / bbox.width(), float(height - 1) / bbox.height())


def _to_pixel(v: float, origin: float, scale: float, via_usize: bool) -> int:
    f = (v - origin) * scale
    if math.isfinite(f):            # f64::floor keeps NaN and the infinities
        f = float(math.floor(f))
    return usize_as_isize(as_usize(f)) if via_usize else as_isize(f)


# --------------------------------------------------- polygon_rasterizer.rs

def _ring_count(poly, px, py):
    """The crossing count of contains_point (polygon.rs:81-100) for arrays of points."""
    count = np.zeros(px.shape, np.int64)
    n = len(poly.vertices)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(n):
            a = poly.vertex_buffer[poly.vertices[i]]
            b = poly.vertex_buffer[poly.vertices[(i + 1) % n]]
            cond = (a.y > py) != (b.y > py)
            x_intersect = a.x + (py - a.y) * (b.x - a.x) / (b.y - a.y)
            count += cond & (px < x_intersect)
    return count


def _contains(poly, px, py):
    inside = _ring_count(poly, px, py) % 2 == 1
    for hole in poly.holes:
        inside &= ~_contains(hole, px, py)
    return inside


def polygon_pixel_points(polygon, width: int, height: int):
    """(px, py): the polygon-space point of every pixel (:54-55), (h, w) arrays."""
    bbox = polygon.bounding_box()
    scale = _scale(width, height, bbox)
    xs = np.arange(width, dtype=np.float64) / scale + bbox.top_left().x
    ys = np.arange(height, dtype=np.float64) / scale + bbox.top_left().y
    return np.broadcast_to(xs[None, :], (height, width)), np.broadcast_to(ys[:, None], (height, width))


def polygon_edge_pixels(polygon, width: int, height: int):
    """The (x0, y0, x1, y1) draw_line gets for every edge, outer ring first (:74-102)."""
    bbox = polygon.bounding_box()
    scale = _scale(width, height, bbox)
    tl = bbox.top_left()
    edges = list(polygon.edges())
    for hole in polygon.holes:
        edges.extend(hole.edges())
    return [(_to_pixel(p0.x, tl.x, scale, True), _to_pixel(p0.y, tl.y, scale, True),
             _to_pixel(p1.x, tl.x, scale, True), _to_pixel(p1.y, tl.y, scale, True))
            for p0, p1 in edges]


def rasterize_polygon(polygon, width: int, height: int, track: bool = False) -> Image:   # :22-103
    img = Image(width, height, track=track)
    px, py = polygon_pixel_points(polygon, width, height)
    inside = _contains(polygon, px, py)
    img.pixels[inside] = LIGHT_BLUE
    if track:
        for y, x in zip(*np.nonzero(inside)):
            img.writers[(int(x), int(y))] = [("fill",)]
    for k, (x0, y0, x1, y1) in enumerate(polygon_edge_pixels(polygon, width, height)):
        draw_line(img, x0, y0, x1, y1, BLACK, ("edge", k))
    return img


# ------------------------------------------------- quad_tree_rasterizer.rs

def _bfs_leaves(root):
    queue, out = [root], []
    while queue:
        cell = queue.pop(0)
        if cell.is_leaf():
            out.append(cell)
        else:
            queue.extend(cell.children)
    return out


def _rasterize_quad_tree_impl(root, img: Image, bbox, via_usize: bool = True) -> None:   # :24-59
    scale = _scale(img.width, img.height, bbox)
    tl = bbox.top_left()
    for k, cell in enumerate(_bfs_leaves(root)):
        b = cell.boundary
        x0 = _to_pixel(b.top_left().x, tl.x, scale, via_usize)
        y0 = _to_pixel(b.top_left().y, tl.y, scale, via_usize)
        x1 = _to_pixel(b.bottom_right().x, tl.x, scale, via_usize)
        y1 = _to_pixel(b.bottom_right().y, tl.y, scale, via_usize)
        draw_line(img, x0, y0, x1, y0, BLACK, ("leaf", k, 0))
        draw_line(img, x1, y0, x1, y1, BLACK, ("leaf", k, 1))
        draw_line(img, x1, y1, x0, y1, BLACK, ("leaf", k, 2))
        draw_line(img, x0, y1, x0, y0, BLACK, ("leaf", k, 3))


def rasterize_quad_tree_no_background(root, width: int, height: int, track=False) -> Image:   # :6-13
    img = Image(width, height, track=track)
    _rasterize_quad_tree_impl(root, img, root.boundary)
    return img


def rasterize_quad_tree(root, background, bbox, track=False, _via_usize=True) -> Image:   # :15-22
    """background: (h, w, 4) uint8 array (copied).  _via_usize=False replaces the
    reference's `as usize` by `as isize`: only for tests that prove the clamp matters."""
    bg = np.asarray(background)
    img = Image(bg.shape[1], bg.shape[0], bg, track=track)
    _rasterize_quad_tree_impl(root, img, bbox, _via_usize)
    return img


# ------------------------------------------------------ mesh_rasterizer.rs

def _rasterize_mesh_impl(mesh, img: Image, bbox) -> None:   # :26-57
    scale = _scale(img.width, img.height, bbox)
    tl = bbox.top_left()
    for i in range(mesh.cell_centers_x.size):              # visit_all_cells
        quad = qr.quad_new_rect(qr.Point(float(mesh.cell_centers_x[i]), float(mesh.cell_centers_y[i])),
                                float(mesh.cell_half_width[i]), float(mesh.cell_half_height[i]))
        for k in range(4):
            start, end = quad[k], quad[(k + 1) % 4]
            draw_line(img, _to_pixel(start.x, tl.x, scale, False), _to_pixel(start.y, tl.y, scale, False),
                      _to_pixel(end.x, tl.x, scale, False), _to_pixel(end.y, tl.y, scale, False),
                      BLACK, ("outline", i, k))
        a, b = (int(v) for v in mesh.cell_intersections_range[i])
        for q in range(a, b):
            x, y = (float(v) for v in mesh.cell_intersections_points[q])
            draw_diamond(img, _to_pixel(x, tl.x, scale, False), _to_pixel(y, tl.y, scale, False),
                         ORANGE, ("diamond", i, q - a))


def rasterize_mesh_no_background(mesh, width: int, height: int, bbox, track=False) -> Image:   # :8-12
    img = Image(width, height, track=track)
    _rasterize_mesh_impl(mesh, img, bbox)
    return img


def rasterize_mesh(mesh, background, bbox, track=False) -> Image:   # :16-22
    bg = np.asarray(background)
    img = Image(bg.shape[1], bg.shape[0], bg, track=track)
    _rasterize_mesh_impl(mesh, img, bbox)
    return img


# ------------------------------------------------------ views/mesh_view.rs

def mesh_view_size(bbox, avail_w: float, avail_h: float):   # :75-88
    ax, ay = np.float32(avail_w), np.float32(avail_h)
    domain_aspect = bbox.width() / bbox.height()
    with np.errstate(divide="ignore", invalid="ignore"):
        available_aspect = float(ax / ay)
    if available_aspect > domain_aspect:
        img_width, img_height = float(ay) * domain_aspect, float(ay)
    else:
        img_width, img_height = float(ax), float(ax) / domain_aspect
    return as_usize(img_width), as_usize(img_height)


def mesh_view_image(polygon, mesh, width: int, height: int, track=False) -> Image:   # :86-94
    img = rasterize_polygon(polygon, width, height, track=track)
    if mesh is not None:
        _rasterize_mesh_impl(mesh, img, polygon.bounding_box())
    return img
