// cfd_mesh_raster.hip — the reference's Mesh tab images behind include/cfd.h:
// src/utils/polygon_rasterizer.rs, quad_tree_rasterizer.rs, mesh_rasterizer.rs
// and drawing.rs, and the image-size rule of views/mesh_view.rs:75-88.
//
// The reference draws sequentially, last writer wins: the polygon fill, the
// polygon's edges, then every cell in ascending index (its four outline
// segments, then its diamonds).  Here every primitive carries a key that grows
// in that order,
//
//     0                     nothing drawn: the background shows
//     1                     a polygon edge                      BLACK
//     2 * (cell + 1)        an outline segment of `cell`        BLACK
//     2 * (cell + 1) + 1    a diamond of `cell`                 ORANGE
//
// and writes atomicMax(key[pixel], its key) into a u32 image on the device
// (integer atomics: exact, independent of arrival order).  The largest key
// at a pixel is the reference's last writer there; a resolve pass turns keys
// into colours and evaluates the background (the per-pixel polygon fill, the
// caller's image, or transparent) where the key is 0.  Lines of a quadtree
// are all one colour, so every leaf takes key 2 and the reference's
// breadth-first leaf order does not matter.
//
// Work mapping: the host maps every endpoint to pixels (it has to, to bound
// the work before any launch), clips axis-parallel segments to the image and
// cuts them into pieces of at most kPiece pixels; one lane walks one piece
// with draw_line's own loop.  Every cell outline and quadtree line is
// axis-parallel, so lanes of a wave run loops of similar, short length; an
// oblique polygon edge is walked whole by one lane.  A diamond takes 16
// lanes, one per pixel of its 4 x 4 box.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/cfd.h"
#include "cfd_mesh_types.h"
#include "quad_geom.h"

extern "C" void cfdrt_set_error(const char *msg);

namespace {

int err(int code, const char *msg) {
    cfdrt_set_error(msg);
    return code;
}

#define RASTER_HIP(expr)                                                                   \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess) {                                                            \
            cfdrt_set_error((std::string(#expr) + ": " + hipGetErrorString(e_)).c_str());  \
            return CFD_EHIP;                                                               \
        }                                                                                  \
    } while (0)

// Build-defined limits (include/cfd.h): the reference has none and would walk
// a far-off line for as long as it takes.
constexpr size_t kMaxSide = 16384;
constexpr double kMaxCoord = 32768.0;   // |pixel coordinate| of any endpoint or centre
constexpr int kPiece = 64;              // pixels per axis-parallel piece

// Color32 as the little-endian u32 of its (r, g, b, a) bytes
constexpr uint32_t kTransparent = 0u;
constexpr uint32_t kBlack = 0xFF000000u;
constexpr uint32_t kLightBlue = 173u | (216u << 8) | (230u << 16) | (255u << 24);
constexpr uint32_t kOrange = 255u | (165u << 8) | (0u << 16) | (255u << 24);

struct Seg {
    int x0, y0, x1, y1;
    uint32_t key;
};
struct Dia {
    int cx, cy;
    uint32_t key;
};

// polygon space <-> pixels, the closures every rasteriser of the reference opens with
struct View {
    double scale, tlx, tly;
};

struct Rings {
    const cfd_point *pts;   // outer ring, then each hole's ring
    const int *off;         // ring k = pts[off[k] .. off[k+1])
    int n_rings;            // 0: no fill
};

enum Background { kBgTransparent = 0, kBgCaller = 1, kBgFill = 2 };

// ------------------------------------------------------------------ kernels

// draw_line (drawing.rs:2-41) with the pixel write replaced by the key
__global__ void k_raster_segments(const Seg *segs, int n, int w, int h, uint32_t *key) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const Seg s = segs[i];
    const int dx = abs(s.x1 - s.x0);
    const int dy = -abs(s.y1 - s.y0);
    const int sx = s.x0 < s.x1 ? 1 : -1;
    const int sy = s.y0 < s.y1 ? 1 : -1;
    int e = dx + dy;
    int x = s.x0, y = s.y0;
    for (;;) {
        if (x >= 0 && x < w && y >= 0 && y < h) atomicMax(&key[(size_t)y * w + x], s.key);
        if (x == s.x1 && y == s.y1) break;
        const int e2 = 2 * e;
        if (e2 >= dy) {
            e += dy;
            x += sx;
        }
        if (e2 <= dx) {
            e += dx;
            y += sy;
        }
    }
}

// draw_diamond (drawing.rs:45-78): the 4 x 4 box whose corner the reference
// computes as floor(cx as f32 - 1.5), which for |cx| <= 2^15 (kMaxCoord) is
// exactly cx - 2, minus its four corners (|i - 1.5| + |j - 1.5| <= 2.0 fails
// only there).  16 lanes per diamond, lane = 4 * j + i.
__global__ void k_raster_diamonds(const Dia *dias, int n, int w, int h, uint32_t *key) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 16L * n) return;
    const Dia d = dias[t >> 4];
    const int i = (int)(t & 3), j = (int)((t >> 2) & 3);
    if ((i == 0 || i == 3) && (j == 0 || j == 3)) return;
    const int x = d.cx - 2 + i, y = d.cy - 2 + j;
    if (x >= 0 && x < w && y >= 0 && y < h) atomicMax(&key[(size_t)y * w + x], d.key);
}

// contains_point with one level of holes (polygon.rs:80-105)
__device__ bool fill_contains(const Rings &R, const cfd_point &p) {
    if (!qm::ring_contains(R.pts + R.off[0], R.off[1] - R.off[0], p)) return false;
    for (int k = 1; k < R.n_rings; ++k)
        if (qm::ring_contains(R.pts + R.off[k], R.off[k + 1] - R.off[k], p)) return false;
    return true;
}

// keys -> colours; where nothing was drawn, the background.  `rgba` holds the
// caller's image on entry when bg == kBgCaller.
__global__ void k_raster_resolve(const uint32_t *key, int w, int h, int bg, Rings R, View v,
                                 uint32_t *rgba) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)w * h) return;
    const uint32_t k = key[idx];
    if (k != 0) {
        rgba[idx] = ((k & 1u) && k >= 3u) ? kOrange : kBlack;
        return;
    }
    if (bg == kBgCaller) return;
    uint32_t c = kTransparent;
    if (bg == kBgFill) {
        const int x = (int)(idx % w), y = (int)(idx / w);
        // polygon_rasterizer.rs:54-55
        const cfd_point p = {(double)x / v.scale + v.tlx, (double)y / v.scale + v.tly};
        if (fill_contains(R, p)) c = kLightBlue;
    }
    rgba[idx] = c;
}

// ------------------------------------------------------------------ host

bool finite_box(const cfd_aabb &b) {
    return std::isfinite(b.center.x) && std::isfinite(b.center.y) && std::isfinite(b.half_width) &&
           std::isfinite(b.half_height);
}

struct Job {
    int w = 0, h = 0;
    View v{};
    int bg = kBgTransparent;
    std::vector<Seg> segs;
    std::vector<Dia> dias;
    std::vector<cfd_point> ring_pts;
    std::vector<int> ring_off;

    int begin(const cfd_aabb &box, size_t w_, size_t h_) {
        if (w_ < 2 || h_ < 2 || w_ > kMaxSide || h_ > kMaxSide)
            return err(CFD_EINVAL, "raster: width and height must be in [2, 16384]");
        const double bw = 2.0 * box.half_width, bh = 2.0 * box.half_height;   // aabb.rs:29-35
        if (!finite_box(box) || !(bw > 0.0) || !(bh > 0.0))
            return err(CFD_EINVAL, "raster: the bounding box must be finite with positive area");
        w = (int)w_;
        h = (int)h_;
        v.scale = std::fmin((double)(w_ - 1) / bw, (double)(h_ - 1) / bh);   // f64::min
        v.tlx = box.center.x - box.half_width;
        v.tly = box.center.y - box.half_height;
        if (!std::isfinite(v.scale) || !(v.scale > 0.0))
            return err(CFD_EINVAL, "raster: the bounding box is too small for the image");
        return 0;
    }

    // floor((x - top_left) * scale) cast as Rust casts it: NaN gives 0;
    // `as usize` (polygon and quadtree rasterisers) clamps negatives to 0,
    // `as isize` (mesh rasteriser) keeps them.  False beyond kMaxCoord.
    static bool to_pixel(double f, bool via_usize, int *out) {
        if (f != f || (via_usize && f < 0.0)) {
            *out = 0;
            return true;
        }
        if (f < -kMaxCoord || f > kMaxCoord) return false;
        *out = (int)f;
        return true;
    }
    bool px(double x, bool via_usize, int *out) const {
        return to_pixel(std::floor((x - v.tlx) * v.scale), via_usize, out);
    }
    bool py(double y, bool via_usize, int *out) const {
        return to_pixel(std::floor((y - v.tly) * v.scale), via_usize, out);
    }

    // An axis-parallel line sets every pixel between its ends and each pixel
    // is clipped on its own (drawing.rs:23), so the clipped pieces set the
    // same pixels.
    void line(int x0, int y0, int x1, int y1, uint32_t key) {
        if (y0 == y1) {
            if (y0 < 0 || y0 >= h) return;
            const int lo = std::max(std::min(x0, x1), 0), hi = std::min(std::max(x0, x1), w - 1);
            for (int a = lo; a <= hi; a += kPiece)
                segs.push_back({a, y0, std::min(a + kPiece - 1, hi), y0, key});
        } else if (x0 == x1) {
            if (x0 < 0 || x0 >= w) return;
            const int lo = std::max(std::min(y0, y1), 0), hi = std::min(std::max(y0, y1), h - 1);
            for (int a = lo; a <= hi; a += kPiece)
                segs.push_back({x0, a, x0, std::min(a + kPiece - 1, hi), key});
        } else {
            segs.push_back({x0, y0, x1, y1, key});
        }
    }

    int too_far() const {
        return err(CFD_EINVAL, "raster: a segment end or diamond centre maps beyond +-32768 pixels");
    }

    // polygon_rasterizer.rs:74-102: the polygon's edges, then each hole's
    int polygon_edges(const cfd_polygon &p) {
        std::vector<cfd_point> e = p.edges();
        for (const cfd_polygon *hole : p.holes) {
            const std::vector<cfd_point> he = hole->edges();
            e.insert(e.end(), he.begin(), he.end());
        }
        for (size_t k = 0; k + 1 < e.size(); k += 2) {
            int x0, y0, x1, y1;
            if (!px(e[k].x, true, &x0) || !py(e[k].y, true, &y0) || !px(e[k + 1].x, true, &x1) ||
                !py(e[k + 1].y, true, &y1))
                return too_far();
            line(x0, y0, x1, y1, 1u);
        }
        return 0;
    }

    // polygon_rasterizer.rs:59-72, evaluated per pixel by the resolve pass
    int polygon_fill(const cfd_polygon &p) {
        for (const cfd_polygon *hole : p.holes)
            if (!hole->holes.empty())
                return err(CFD_EINVAL, "raster: holes with holes are not supported");
        ring_pts = p.ring();
        ring_off = {0, (int)ring_pts.size()};
        for (const cfd_polygon *hole : p.holes) {
            const std::vector<cfd_point> r = hole->ring();
            ring_pts.insert(ring_pts.end(), r.begin(), r.end());
            ring_off.push_back((int)ring_pts.size());
        }
        bg = kBgFill;
        return 0;
    }

    // quad_tree_rasterizer.rs:40-58
    int quadtree(const cfd_quadtree &t) {
        for (size_t k = 0; k < t.boxes.size(); ++k) {
            if (t.children[4 * k] >= 0) continue;
            const cfd_aabb &b = t.boxes[k];
            int x0, y0, x1, y1;
            if (!px(b.center.x - b.half_width, true, &x0) ||
                !py(b.center.y - b.half_height, true, &y0) ||
                !px(b.center.x + b.half_width, true, &x1) ||
                !py(b.center.y + b.half_height, true, &y1))
                return too_far();
            line(x0, y0, x1, y0, 2u);
            line(x1, y0, x1, y1, 2u);
            line(x1, y1, x0, y1, 2u);
            line(x0, y1, x0, y0, 2u);
        }
        return 0;
    }

    // mesh_rasterizer.rs:35-56 over visit_all_cells (ascending index)
    int mesh(const cfd_mesh &m) {
        const size_t n = m.cx.size();
        if (n >= (size_t)1 << 30) return err(CFD_EINVAL, "raster: too many cells");
        for (size_t i = 0; i < n; ++i) {
            // Quad::new_rect (quad.rs:24-35): bottom-left, bottom-right, top-right, top-left
            int l, r, b, t;
            if (!px(m.cx[i] - m.hw[i], false, &l) || !px(m.cx[i] + m.hw[i], false, &r) ||
                !py(m.cy[i] - m.hh[i], false, &b) || !py(m.cy[i] + m.hh[i], false, &t))
                return too_far();
            const uint32_t key = 2u * (uint32_t)(i + 1);
            line(l, b, r, b, key);
            line(r, b, r, t, key);
            line(r, t, l, t, key);
            line(l, t, l, b, key);
            for (uint64_t q = m.x_range[2 * i]; q < m.x_range[2 * i + 1]; ++q) {
                int x, y;
                if (!px(m.x_points[q].x, false, &x) || !py(m.x_points[q].y, false, &y))
                    return too_far();
                dias.push_back({x, y, key + 1u});
            }
        }
        return 0;
    }
};

struct DevBuf {
    std::vector<void *> ptrs;
    ~DevBuf() {
        for (void *p : ptrs) (void)hipFree(p);
    }
    template <class T> int alloc(T **p, size_t n) {
        void *q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess)
            return err(CFD_EHIP, "hipMalloc failed (raster)");
        ptrs.push_back(q);
        *p = (T *)q;
        return 0;
    }
};

struct Events {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// Everything is validated by now: from here on only HIP can fail, and rgba is
// written by the last copy alone.
int run(const Job &job, int device, const uint8_t *background, uint8_t *rgba, double *device_ms) {
    if (job.segs.size() >= (size_t)1 << 30 || job.dias.size() >= (size_t)1 << 26)
        return err(CFD_EINVAL, "raster: too many primitives");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return err(CFD_EHIP, "no HIP device available");
    if (device < 0 || device >= ndev) return err(CFD_EINVAL, "device ordinal out of range");
    RASTER_HIP(hipSetDevice(device));
    const size_t npix = (size_t)job.w * job.h;
    const int ns = (int)job.segs.size(), nd = (int)job.dias.size();
    DevBuf db;
    uint32_t *key, *img;
    Seg *segs;
    Dia *dias;
    cfd_point *pts;
    int *off;
    int rc;
    if ((rc = db.alloc(&key, npix)) || (rc = db.alloc(&img, npix)) || (rc = db.alloc(&segs, ns)) ||
        (rc = db.alloc(&dias, nd)) || (rc = db.alloc(&pts, job.ring_pts.size())) ||
        (rc = db.alloc(&off, job.ring_off.size())))
        return rc;
    hipStream_t s;
    RASTER_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    struct StreamGuard {
        hipStream_t s;
        ~StreamGuard() { (void)hipStreamDestroy(s); }
    } sg{s};
    Events ev;
    RASTER_HIP(hipEventCreate(&ev.e0));
    RASTER_HIP(hipEventCreate(&ev.e1));
    if (ns) RASTER_HIP(hipMemcpyAsync(segs, job.segs.data(), ns * sizeof(Seg), hipMemcpyHostToDevice, s));
    if (nd) RASTER_HIP(hipMemcpyAsync(dias, job.dias.data(), nd * sizeof(Dia), hipMemcpyHostToDevice, s));
    if (job.bg == kBgFill) {
        RASTER_HIP(hipMemcpyAsync(pts, job.ring_pts.data(), job.ring_pts.size() * sizeof(cfd_point),
                                  hipMemcpyHostToDevice, s));
        RASTER_HIP(hipMemcpyAsync(off, job.ring_off.data(), job.ring_off.size() * sizeof(int),
                                  hipMemcpyHostToDevice, s));
    }
    if (job.bg == kBgCaller)
        RASTER_HIP(hipMemcpyAsync(img, background, npix * 4, hipMemcpyHostToDevice, s));
    RASTER_HIP(hipEventRecord(ev.e0, s));
    RASTER_HIP(hipMemsetAsync(key, 0, npix * 4, s));
    const int B = 256;
    if (ns)
        hipLaunchKernelGGL(k_raster_segments, dim3((unsigned)((ns + B - 1) / B)), dim3(B), 0, s,
                           (const Seg *)segs, ns, job.w, job.h, key);
    if (nd)
        hipLaunchKernelGGL(k_raster_diamonds, dim3((unsigned)((16L * nd + B - 1) / B)), dim3(B), 0, s,
                           (const Dia *)dias, nd, job.w, job.h, key);
    const Rings R{pts, off, job.bg == kBgFill ? (int)job.ring_off.size() - 1 : 0};
    hipLaunchKernelGGL(k_raster_resolve, dim3((unsigned)((npix + B - 1) / B)), dim3(B), 0, s,
                       (const uint32_t *)key, job.w, job.h, job.bg, R, job.v, img);
    RASTER_HIP(hipGetLastError());
    RASTER_HIP(hipEventRecord(ev.e1, s));
    RASTER_HIP(hipStreamSynchronize(s));
    float ms = 0.f;
    RASTER_HIP(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    RASTER_HIP(hipMemcpy(rgba, img, npix * 4, hipMemcpyDeviceToHost));
    if (device_ms) *device_ms = ms;
    return 0;
}

// Rust's `f64 as usize`: NaN and negatives give 0, large values saturate
size_t as_usize(double f) {
    if (!(f > 0.0)) return 0;
    if (f >= 18446744073709551616.0) return SIZE_MAX;
    return (size_t)f;
}

}  // namespace

// =============================================================== C ABI

extern "C" {

int cfd_raster_polygon(const cfd_polygon *p, int device, size_t w, size_t h, uint8_t *rgba,
                       double *device_ms) {
    if (!p || !rgba) return err(CFD_EINVAL, "null argument");
    Job job;
    int rc;
    if ((rc = job.begin(p->bbox(), w, h)) || (rc = job.polygon_fill(*p)) ||
        (rc = job.polygon_edges(*p)))
        return rc;
    return run(job, device, nullptr, rgba, device_ms);
}

int cfd_raster_quadtree(const cfd_quadtree *t, const cfd_aabb *bbox, int device, size_t w, size_t h,
                        const uint8_t *background, uint8_t *rgba, double *device_ms) {
    if (!t || !rgba || t->boxes.empty()) return err(CFD_EINVAL, "null argument");
    Job job;
    int rc;
    if ((rc = job.begin(bbox ? *bbox : t->boxes[0], w, h)) || (rc = job.quadtree(*t))) return rc;
    if (background) job.bg = kBgCaller;
    return run(job, device, background, rgba, device_ms);
}

int cfd_raster_mesh(const cfd_mesh *m, const cfd_aabb *bbox, int device, size_t w, size_t h,
                    const uint8_t *background, uint8_t *rgba, double *device_ms) {
    if (!m || !bbox || !rgba) return err(CFD_EINVAL, "null argument");
    Job job;
    int rc;
    if ((rc = job.begin(*bbox, w, h)) || (rc = job.mesh(*m))) return rc;
    if (background) job.bg = kBgCaller;
    return run(job, device, background, rgba, device_ms);
}

int cfd_raster_mesh_view(const cfd_polygon *p, const cfd_mesh *mesh_or_null, int device, size_t w,
                         size_t h, uint8_t *rgba, double *device_ms) {
    if (!p || !rgba) return err(CFD_EINVAL, "null argument");
    Job job;
    int rc;
    if ((rc = job.begin(p->bbox(), w, h)) || (rc = job.polygon_fill(*p)) ||
        (rc = job.polygon_edges(*p)) || (mesh_or_null && (rc = job.mesh(*mesh_or_null))))
        return rc;
    return run(job, device, nullptr, rgba, device_ms);
}

int cfd_mesh_view_size(const cfd_aabb *bbox, float avail_w, float avail_h, size_t *w, size_t *h) {
    if (!bbox || !w || !h) return err(CFD_EINVAL, "null argument");
    const double domain_aspect = (2.0 * bbox->half_width) / (2.0 * bbox->half_height);
    const double available_aspect = (double)(avail_w / avail_h);   // an f32 division, widened
    double iw, ih;
    if (available_aspect > domain_aspect) {
        iw = (double)avail_h * domain_aspect;
        ih = (double)avail_h;
    } else {
        iw = (double)avail_w;
        ih = (double)avail_w / domain_aspect;
    }
    *w = as_usize(iw);
    *h = as_usize(ih);
    return 0;
}

}  // extern "C"
