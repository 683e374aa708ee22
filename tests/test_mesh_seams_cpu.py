"""CPU: the premises of tests/test_gpu_mesh_seams.py, from the oracle alone, and
the host-side index check of cfd_polygon_new.

The GPU file compares Mesh.from_quad_tree (csrc/cfd_mesh.hip) with
oracle/quad_mesh_ref.py bit for bit on the cases of tests/_mesh_cases.py.  A
case only has teeth while it still is what its name says, so each premise is
asserted here:

  * every case's leaf count and kept-cell count are the table's, and the table
    holds the counts that sit on the 256-cell tile of k_mesh_neighbors:
    1, 4, 252, 255, 256, 257, one of 511..513 and one above 768;
  * leaf counts are 1 mod 3, so nl == 257 does not exist;
  * the first / the last kept cell of the two "alone" cases has empty lists
    on the stated faces: an empty range at the start / the end of a face;
  * the tiny-cell case has 186 entries per face where true adjacency gives 56;
  * the sub-selected polygon's edges are the index quirk's, not its ring's;
  * the reversed ring has the forward ring's edges in another order, and its
    intersection points come out in another order cell by cell;
  * the far case takes the collinear branch: two points per cell side lying
    on the hole, exact at 2**20;
  * the host tesselation of the product gives the same leaf counts.

Through the product library: an index whose edge end (i + 1) % vertices.len()
lies past the vertex buffer is refused by Polygon.new with CFD_EINVAL, where
edges() would read past the buffer (the reference panics there).
"""
import numpy as np
import pytest

from _mesh_cases import (CASES, EMPTY_FIRST, EMPTY_LAST, FACES, FAR_X, FAR_Y, SUB_QUIRK_EDGES,
                         TILE, TINY_ADJACENT_PER_FACE, TINY_ENTRIES_PER_FACE, oracle_mesh)


def _len(mesh, face, i):
    a, b = getattr(mesh, f"neighbors_{face}_range")[i]
    return int(b) - int(a)


@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_are_the_table(name):
    nl, mesh = oracle_mesh(name)
    assert (nl, mesh.cell_centers_x.size) == CASES[name][3:]
    assert nl % 3 == 1


def test_table_sits_on_the_tile():
    ncs = {c[4] for c in CASES.values()}
    assert {1, 4, TILE - 4, TILE - 1, TILE, TILE + 1} <= ncs
    assert ncs & {2 * TILE - 1, 2 * TILE, 2 * TILE + 1}
    assert any(3 * TILE < nc <= 1000 for nc in ncs)
    assert max(ncs) <= 1000
    assert all(c[3] % 3 == 1 for c in CASES.values())


def test_one_cell_has_four_empty_lists():
    _, mesh = oracle_mesh("one_cell")
    for face in FACES:
        assert getattr(mesh, f"neighbors_{face}_indexes").size == 0
        assert getattr(mesh, f"neighbors_{face}_range").tolist() == [[0, 0]]


@pytest.mark.parametrize("table,cell", [(EMPTY_FIRST, 0), (EMPTY_LAST, -1)])
def test_empty_lists_at_the_ends(table, cell):
    for name, faces in table.items():
        _, mesh = oracle_mesh(name)
        for face in FACES:
            total = getattr(mesh, f"neighbors_{face}_indexes").size
            assert total > 0
            assert (_len(mesh, face, cell) == 0) == (face in faces), (name, face)
            if face in faces:   # the empty range sits at the very start / end
                want = [0, 0] if cell == 0 else [total, total]
                assert getattr(mesh, f"neighbors_{face}_range")[cell].tolist() == want


def test_tiny_cells_abut_two_columns_away():
    _, mesh = oracle_mesh("tiny_cells")
    assert float(mesh.cell_half_width.max()) * 2.0 < 1e-6
    xmin = mesh.cell_centers_x - mesh.cell_half_width
    ymin = mesh.cell_centers_y - mesh.cell_half_height
    w = 2.0 * float(mesh.cell_half_width[0])
    col, row = np.rint(xmin / w).astype(int), np.rint(ymin / w).astype(int)
    for face in FACES:
        idx = getattr(mesh, f"neighbors_{face}_indexes")
        assert idx.size == TINY_ENTRIES_PER_FACE
    # true adjacency (the next column, the same row) would give far fewer
    adjacent = sum(1 for i in range(64) for j in range(64)
                   if col[j] == col[i] + 1 and row[j] == row[i])
    assert adjacent == TINY_ADJACENT_PER_FACE
    # and some east neighbour really is two columns away
    far = 0
    for i in range(64):
        a, b = mesh.neighbors_east_range[i]
        far += sum(1 for j in mesh.neighbors_east_indexes[int(a):int(b)] if col[int(j)] - col[i] == 2)
    assert far > 0


def _edge_tuples(poly):
    return [((a.x, a.y), (b.x, b.y)) for a, b in poly.edges()]


def test_sub_selected_edges_are_the_quirks():
    import quad_mesh_ref as qr
    poly = CASES["sub_selected"][0](qr)
    assert _edge_tuples(poly) == SUB_QUIRK_EDGES
    ring = [(0, 0), (4, 0), (4, 4), (0, 4)]
    assert [(poly.vertex_buffer[i].x, poly.vertex_buffer[i].y) for i in poly.vertices] == ring
    assert sorted(SUB_QUIRK_EDGES) != sorted(zip(ring, ring[1:] + ring[:1]))
    _, mesh = oracle_mesh("sub_selected")
    assert mesh.cell_intersections_points.shape[0] > 0


def test_reversed_ring_reorders_the_points():
    import quad_mesh_ref as qr
    fwd, rev = (_edge_tuples(CASES[n][0](qr)) for n in ("ring_forward", "ring_reversed"))
    assert fwd != rev and sorted(fwd) == sorted(rev)
    (_, a), (_, b) = oracle_mesh("ring_forward"), oracle_mesh("ring_reversed")
    for f in ("cell_centers_x", "cell_centers_y", "cell_half_width", "cell_intersections_range"):
        assert np.array_equal(getattr(a, f), getattr(b, f))
    pa, pb = a.cell_intersections_points, b.cell_intersections_points
    assert pa.shape == pb.shape and not np.array_equal(pa.view(np.uint64), pb.view(np.uint64))
    reordered = 0
    for s, e in a.cell_intersections_range:
        ca, cb = pa[int(s):int(e)], pb[int(s):int(e)]
        assert sorted(map(tuple, ca.tolist())) == sorted(map(tuple, cb.tolist()))
        reordered += not np.array_equal(ca, cb)
    assert reordered > 0


def test_far_case_takes_the_collinear_branch():
    _, mesh = oracle_mesh("far_collinear")
    assert float(mesh.cell_centers_x.min()) > FAR_X and float(mesh.cell_centers_y.max()) < FAR_Y + 16.0
    pts = mesh.cell_intersections_points
    hx, hy = (FAR_X + 4.0, FAR_X + 6.0), (FAR_Y + 4.0, FAR_Y + 6.0)
    on_hole = ((np.isin(pts[:, 0], hx) & (pts[:, 1] >= hy[0]) & (pts[:, 1] <= hy[1])) |
               (np.isin(pts[:, 1], hy) & (pts[:, 0] >= hx[0]) & (pts[:, 0] <= hx[1])))
    assert on_hole.sum() > 0
    # every point is an exact lattice point: the sides are collinear, no point is interpolated
    assert np.array_equal(pts, np.rint(pts))
    # a cell with a side on the hole gets that side's two ends, and a corner
    # shared by two such sides is de-duplicated, not listed twice
    two_or_more = 0
    for s, e in mesh.cell_intersections_range:
        cell = pts[int(s):int(e)][on_hole[int(s):int(e)]]
        two_or_more += cell.shape[0] >= 2
    assert two_or_more > 0


def test_gon64_has_64_hole_edges():
    import quad_mesh_ref as qr
    poly = CASES["gon64_hole"][0](qr)
    assert len(poly.holes) == 1 and len(poly.holes[0].edges()) == 64


@pytest.mark.parametrize("name", sorted(CASES))
def test_product_tesselation_has_the_tables_leaves(name):
    """The host half of the product (tesselate over the C ABI) on the same
    cases: leaf counts, and the edge list with the index quirk."""
    from cfdamd import quad_mesh as qm
    import quad_mesh_ref as qr
    build, f, mx, nl, _ = CASES[name]
    poly = build(qm)
    assert qm.tesselate(poly, f, mx).n_leaves == nl
    assert _edge_tuples(poly) == _edge_tuples(build(qr))


def test_edge_end_index_past_the_buffer_is_refused():
    """vertices [0, 0, 0] over a one-point buffer: every index is in range,
    three vertices skip the self-intersection test, and edges() would read
    vertex_buffer[(0 + 1) % 3] of a one-element buffer."""
    from cfdamd import CfdError
    from cfdamd import quad_mesh as qm
    from cfdamd._lib import CFD_EINVAL
    import quad_mesh_ref as qr
    with pytest.raises(CfdError) as ei:
        qm.Polygon.new([qm.Point(0.0, 0.0)], [0, 0, 0])
    assert ei.value.code == CFD_EINVAL
    assert "panics" in str(ei.value)
    with pytest.raises(IndexError):
        qr.Polygon.new([qr.Point(0.0, 0.0)], [0, 0, 0])
    # in range on both counts: still accepted, on both sides
    for m in (qm, qr):
        P = m.Point
        m.Polygon.new([P(0.0, 0.0), P(1.0, 0.0), P(0.0, 1.0), P(5.0, 5.0)], [0, 1, 2])
        with pytest.raises((CfdError, IndexError)):   # (3 + 1) % 5 == 4 >= 4 points
            m.Polygon.new([P(0.0, 0.0), P(4.0, 0.0), P(4.0, 4.0), P(0.0, 4.0)], [0, 1, 2, 3, 3])
