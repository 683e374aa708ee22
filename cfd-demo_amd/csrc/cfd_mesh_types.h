// cfd_mesh_types.h — the handles of the mesher block of include/cfd.h
// (cfd_polygon, cfd_quadtree, cfd_mesh), shared by the unit that builds them
// (cfd_mesh.hip) and the unit that draws them (cfd_mesh_raster.hip).
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/cfd.h"
#include "quad_geom.h"

struct cfd_polygon {
    std::vector<cfd_point> vb;      // vertex_buffer
    std::vector<uint64_t> verts;    // vertices (indices into vb)
    std::vector<cfd_polygon *> holes;
    ~cfd_polygon() {
        for (cfd_polygon *h : holes) delete h;
    }
    std::vector<cfd_point> ring() const {
        std::vector<cfd_point> r(verts.size());
        for (size_t k = 0; k < verts.size(); ++k) r[k] = vb[verts[k]];
        return r;
    }
    // contains_point (polygon.rs:81-103)
    bool contains(const cfd_point &p) const {
        const std::vector<cfd_point> r = ring();
        if (!qm::ring_contains(r.data(), (int)r.size(), p)) return false;
        for (const cfd_polygon *h : holes)
            if (h->contains(p)) return false;
        return true;
    }
    // edges (polygon.rs:186-196): the reference pairs vertex_buffer[i] with
    // vertex_buffer[(i + 1) % vertices.len()] for each vertex index i
    std::vector<cfd_point> edges() const {
        std::vector<cfd_point> e;
        const size_t n = verts.size();
        for (uint64_t i : verts) {
            e.push_back(vb[i]);
            e.push_back(vb[(i + 1) % n]);
        }
        return e;
    }
    // edges_intersect_aabb (polygon.rs:119-133); defined in cfd_mesh.hip
    bool edges_intersect(const cfd_aabb &box) const;
    // bounding_box (polygon.rs:150-178): over the whole vertex buffer
    cfd_aabb bbox() const {
        double min_x = INFINITY, max_x = -INFINITY, min_y = INFINITY, max_y = -INFINITY;
        for (const cfd_point &p : vb) {
            min_x = std::fmin(min_x, p.x);
            max_x = std::fmax(max_x, p.x);
            min_y = std::fmin(min_y, p.y);
            max_y = std::fmax(max_y, p.y);
        }
        cfd_aabb b;
        b.center = {(min_x + max_x) / 2.0, (min_y + max_y) / 2.0};
        b.half_width = (max_x - min_x) / 2.0;
        b.half_height = (max_y - min_y) / 2.0;
        return b;
    }
};

struct cfd_quadtree {
    std::vector<cfd_aabb> boxes;
    std::vector<int64_t> children;   // 4 per node, -1 for leaves
    uint64_t leaves = 0;
};

struct cfd_mesh {
    std::vector<double> cx, cy, hw, hh;
    std::vector<uint64_t> nb_range[4], nb_index[4];
    std::vector<uint64_t> x_range;
    std::vector<cfd_point> x_points;
    double build_ms = 0.0;
};
