"""The case table of tests/test_mesh_seams_cpu.py and tests/test_gpu_mesh_seams.py.

Mesh::from_quad_tree on the device (csrc/cfd_mesh.hip) streams the kept cells
through 256-cell LDS tiles with one workgroup per 256 cells, scans each count
into the offsets its fill kernel writes through, and rebases the four faces'
starts on the host.  Each case here is chosen for what that code could get
wrong: the number of kept cells against the tile (1, 4, 252, 255, 256, 257,
511, 512, 867), lists that are empty at either end of a face's array, the
reference's vertex-index quirk in edges() (polygon.rs:188-197), the 1e-6
abutment test on cells narrower than 1e-6, coordinates near 2**20, edges
collinear with cell sides and a 64-edge hole.

A case is (build(m), feature_size, max_cell_size, nl, nc): build takes the
module (cfdamd.quad_mesh or quad_mesh_ref) and returns its Polygon, nl is the
number of leaves of the tesselation and nc the number of cells the mesh keeps.
The counts were found with the oracle (quad_mesh_ref) on the CPU;
test_mesh_seams_cpu.py asserts every one of them and each case's stated
property.  nl is always 1 mod 3 (a split replaces one leaf with four), so
nc == 257 has to come from dropped cells: 397 leaves, 140 of them outside.
"""
import functools

TILE = 256   # kTile in csrc/cfd_mesh.hip
FACES = ("east", "west", "north", "south")


def _square(m, holes=()):
    poly = m.Polygon.new_rect(0.0, 0.0, 16.0, 16.0)
    for h in holes:
        poly.add_hole(m.Polygon.new_rect(*h))
    return poly


def _plain(m):
    return _square(m)


def _hole_1(m):       # swallows the cell [4, 5] x [4, 5]
    return _square(m, [(3.9, 3.9, 1.2, 1.2)])


def _hole_4(m):       # swallows [4, 6] x [4, 6]
    return _square(m, [(3.9, 3.9, 2.2, 2.2)])


SUB_POINTS = [(0, 0), (9, 9), (4, 0), (7, 7), (4, 4), (0, 4)]
SUB_INDICES = [0, 2, 4, 5]
# edges() pairs vertex_buffer[i] with vertex_buffer[(i + 1) % 4] for the index
# VALUE i: not the ring (0,0)-(4,0)-(4,4)-(0,4) that contains_point walks
SUB_QUIRK_EDGES = [((0, 0), (9, 9)), ((4, 0), (7, 7)), ((4, 4), (9, 9)), ((0, 4), (4, 0))]


def _sub_selected(m):
    return m.Polygon.new([m.Point(float(x), float(y)) for x, y in SUB_POINTS], SUB_INDICES)


def _tiny(m):
    return m.Polygon.new_rect(0.0, 0.0, 4e-6, 4e-6)


def _rect_16x6_hole(m):
    poly = m.Polygon.new_rect(0.0, 0.0, 16.0, 6.0)
    poly.add_hole(m.Polygon.new_rect(0.4, 0.9, 10.7, 2.4))
    return poly


def _thin_holes(m):   # two slits that split 14 + 11 unit cells and drop none
    return _square(m, [(1.1, 3.3, 13.8, 0.2), (1.1, 6.3, 10.8, 0.2)])


def _rect_8x16_hole(m):
    poly = m.Polygon.new_rect(0.0, 0.0, 8.0, 16.0)
    poly.add_hole(m.Polygon.new_rect(4.9, 10.8, 2.4, 4.7))
    return poly


def _last_cell_alone(m):   # drops [15, 16] x [14, 15], the cell south of the last one
    return _square(m, [(14.9, 13.9, 1.0, 1.2)])


def _first_cell_alone(m):  # a 0.4-wide stem under a slab: nothing east of cell 0
    P = m.Point
    return m.Polygon.new([P(0.0, 0.0), P(0.4, 0.0), P(0.4, 4.5), P(8.0, 4.5), P(8.0, 8.0),
                          P(0.0, 8.0)], [0, 1, 2, 3, 4, 5])


def _ring(m, indices):
    P = m.Point
    return m.Polygon.new([P(0.0, 0.0), P(16.0, 0.0), P(16.0, 16.0), P(0.0, 16.0)], indices)


def _ring_forward(m):
    return _ring(m, [0, 1, 2, 3])


def _ring_reversed(m):
    return _ring(m, [3, 2, 1, 0])


FAR_X, FAR_Y = float(2 ** 20), -float(2 ** 20)


def _far_collinear(m):     # the hole's sides lie on the unit cells' sides
    poly = m.Polygon.new_rect(FAR_X, FAR_Y, 16.0, 16.0)
    poly.add_hole(m.Polygon.new_rect(FAR_X + 4.0, FAR_Y + 4.0, 2.0, 2.0))
    return poly


def _gon64(m):
    poly = _square(m)
    poly.add_hole(m.Polygon.new_polygon(m.Point(8.0, 8.0), 1.0, 64, 0.1))
    return poly


CASES = {
    #                     build             feature  max     nl    nc
    "one_cell":          (_plain,            32.0,   32.0,     1,    1),
    "2x2":               (_plain,            32.0,   8.0,      4,    4),
    "full_tile":         (_plain,            1.0,    1.0,    256,  256),
    "tile_minus_1":      (_hole_1,           1.0,    1.0,    256,  255),
    "mixed_sizes":       (_hole_1,           0.25,   1.0,    868,  867),
    "tile_minus_4":      (_hole_4,           1.0,    1.0,    256,  252),
    "sub_selected":      (_sub_selected,     0.5,    1.0,    466,  157),
    "tiny_cells":        (_tiny,             5e-7,   5e-7,    64,   64),
    "tile_plus_1":       (_rect_16x6_hole,   0.5,    2.0,    397,  257),
    "two_tiles_minus_1": (_thin_holes,       0.5,    1.0,    511,  511),
    "two_tiles":         (_rect_8x16_hole,   0.5,    0.5,   1024,  512),
    "last_cell_alone":   (_last_cell_alone,  1.0,    1.0,    256,  255),
    "first_cell_alone":  (_first_cell_alone, 1.0,    1.0,     64,   36),
    "ring_forward":      (_ring_forward,     2.0,    4.0,     52,   52),
    "ring_reversed":     (_ring_reversed,    2.0,    4.0,     52,   52),
    "far_collinear":     (_far_collinear,    1.0,    1.0,    256,  255),
    "gon64_hole":        (_gon64,            0.25,   4.0,    760,  740),
}

# faces on which the first / the last kept cell has no neighbour at all: an
# empty range at the very start / the very end of that face's index list
EMPTY_FIRST = {"first_cell_alone": ("east", "west", "south")}
EMPTY_LAST = {"last_cell_alone": ("east", "north", "south")}
TINY_ENTRIES_PER_FACE = 186     # the 1e-6 test; true adjacency would give 56
TINY_ADJACENT_PER_FACE = 56


@functools.lru_cache(maxsize=None)
def oracle_mesh(name):
    """(leaf count, quad_mesh_ref.Mesh) of a case, built once per process and
    shared; nothing may write to its arrays."""
    import quad_mesh_ref as qr
    build, f, mx = CASES[name][:3]
    poly = build(qr)
    root = qr.tesselate(poly, f, mx)
    nl = sum(1 for n in qr.preorder(root) if n.is_leaf())
    mesh = qr.Mesh(root, poly)
    for a in vars(mesh).values():
        a.setflags(write=False)
    return nl, mesh
