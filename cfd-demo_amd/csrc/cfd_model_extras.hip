// cfd_model_extras.hip — tracer particles and the script's substep
// (the host runtime behind include/cfd.h; see cfd_model.h)
#include <cstring>

#include "cfd_model.h"

using namespace cfd;

int cfd_model::trc_release() {
    if (!trc_pool) return 0;
    for (size_t k = 0; k < ck_segs.size(); ++k)
        if (ck_segs[k].ptr == (void *)trc_pool) {
            ck_segs.erase(ck_segs.begin() + (long)k);
            break;
        }
    if (int rc = ck_drop_pool()) return rc;
    HIP_TRY(hipFree(trc_pool));
    trc_pool = nullptr;
    trc = Tracers{};
    return 0;
}

// isPointInObstacle (:212-215) at one face position, in double
bool cfd_model::scr_in_obstacle(double x, double y) const {
    if (!grid.has_cylinder) return false;
    const double ex = x - (double)grid.cylinder_x, ey = y - (double)grid.cylinder_y;
    return std::sqrt(ex * ex + ey * ey) <= (double)grid.cylinder_radius;
}
int cfd_model::script_build() {
    if (scr_pool) return 0;
    const int nx = g.nx, ny = g.ny;
    const double dx = (double)g.dx, dy = (double)g.dy;
    // every face is evaluated; a disc under correctly rounded monotone
    // operations gives one interval per row, and that is checked, not assumed
    std::vector<int32_t> iv((size_t)2 * ny + 2 * (ny + 1), 0);
    auto row = [&](int32_t *out, int n, auto inside) -> bool {
        int lo = -1, hi = -1, cnt = 0;
        for (int i = 0; i < n; ++i)
            if (inside(i)) {
                if (lo < 0) lo = i;
                hi = i + 1;
                ++cnt;
            }
        if (cnt && hi - lo != cnt) return false;
        out[0] = cnt ? lo : 0;
        out[1] = cnt ? hi : 0;
        return true;
    };
    bool ok = true;
    for (int j = 0; j < ny && ok; ++j)
        ok = row(&iv[(size_t)2 * j], nx + 1,
                 [&](int i) { return scr_in_obstacle((double)i * dx, ((double)j + 0.5) * dy); });
    for (int j = 0; j <= ny && ok; ++j)
        ok = row(&iv[(size_t)2 * ny + 2 * j], nx,
                 [&](int i) { return scr_in_obstacle(((double)i + 0.5) * dx, (double)j * dy); });
    if (!ok) return fail(CFD_ESTATE, "script step: a row's obstacle faces are not one interval");
    const size_t ib = iv.size() * 4, bytes = ib + (size_t)ny * 4;
    HIP_TRY(hipMalloc((void **)&scr_pool, bytes));
    HIP_TRY(hipMemcpy(scr_pool, iv.data(), ib, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(scr_pool + ib, 0, (size_t)ny * 4));
    scr.obs_u = (const int32_t *)scr_pool;
    scr.obs_v = scr.obs_u + 2 * ny;
    scr.inlet = (const float *)(scr_pool + ib);
    scr.dx = dx;
    scr.dy = dy;
    scr.dxx = dx * dx;
    scr.dyy = dy * dy;
    scr.nu = (double)g.nu;
    scr.r_dx = 1.0 / scr.dx;
    scr.r_dy = 1.0 / scr.dy;
    scr.r_dxx = 1.0 / scr.dxx;
    scr.r_dyy = 1.0 / scr.dyy;
    // (dx, dy and their squares come from positive floats: exact_pow2's range
    // clauses hold for every power of two among them)
    scr.fast = exact_pow2(scr.dx) && exact_pow2(scr.dy) && exact_pow2(scr.dxx) && exact_pow2(scr.dyy) ? 1 : 0;
    scr_inlet_h.assign((size_t)ny, 0.0f);
    return 0;
}
// the call's ScriptStep: dt, viscosity (cfd_set_params may have changed
// it) and the inlet column (:873-885), uploaded in stream order
int cfd_model::script_prepare(const cfd_script_step *s, ScriptStep *out) {
    if (int rc = script_build()) return rc;
    scr.nu = (double)g.nu;
    if (scr_inlet_profile != s->inlet_profile ||
        std::memcmp(&scr_inlet_v, &s->inlet_velocity, 8) != 0) {
        const int ny = g.ny;
        const double ly = (double)grid.ly, dy = (double)g.dy;
        for (int j = 0; j < ny; ++j) {
            double val = s->inlet_velocity;
            if (s->inlet_profile == CFD_INLET_PARABOLIC) {
                const double y = ((double)j + 0.5) * dy;
                const double center = ly / 2, radius = ly / 2;
                const double t = (y - center) / radius;
                val = s->inlet_velocity * (1 - t * t);   // Math.pow(t, 2) == t * t
                val = val > 0 ? val : (val != val ? val : 0.0);   // Math.max(val, 0)
            }
            scr_inlet_h[(size_t)j] = (float)val;
        }
        // pageable source: the copy has left scr_inlet_h when the call returns
        HIP_TRY(hipMemcpyAsync((void *)scr.inlet, scr_inlet_h.data(), (size_t)ny * 4,
                               hipMemcpyHostToDevice, stream));
        scr_inlet_v = s->inlet_velocity;
        scr_inlet_profile = s->inlet_profile;
    }
    *out = scr;
    out->dt = s->dt_sub;
    return 0;
}

extern "C" {

// ---- tracer particles (index.html:1472-1543; kernels in cfd_tracers.hip) ----
namespace {

constexpr uint64_t kTrcMaxCap = 1ull << 30;

const char *const kTrcOverflowMsg =
    "tracer capacity overflow: an injection of ny tracers did not fit; the list is no longer the "
    "script's until cfd_tracers_enable or cfd_tracers_set";

// Drain the stream and fetch the tracer words; the sticky overflow is an error
// of every reading call.
int trc_read(cfd_model *m, TrcCtl *tc) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (!m->trc_pool) return fail(CFD_ESTATE, "tracers are not enabled (cfd_tracers_enable)");
    int rc = m->sync();
    if (rc) return rc;
    HIP_TRY(hipMemcpy(tc, m->trc.tc, sizeof(TrcCtl), hipMemcpyDeviceToHost));
    if (tc->overflow) return fail(CFD_ESTATE, kTrcOverflowMsg);
    return 0;
}

// The explicit calls change tracer state outside a step: they drain the stream
// first, which commits the self-recovery checkpoint, so the next step takes a
// fresh one that holds their result (no replay runs them twice).
int trc_begin_call(cfd_model *m) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (!m->trc_pool) return fail(CFD_ESTATE, "tracers are not enabled (cfd_tracers_enable)");
    return m->sync();
}

}  // namespace

int cfd_tracers_enable(cfd_model *m, uint64_t capacity, int inject_interval) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (m->sharded())
        return fail(CFD_EINVAL, "tracers run on one domain only: a tracer reads u and v rows of "
                                "other slabs");
    const uint64_t ny = (uint64_t)m->g.ny;
    if (capacity < ny || capacity > kTrcMaxCap)
        return fail(CFD_EINVAL, "tracer capacity must be in [ny, 2^30] (ny = " + std::to_string(ny) + ")");
    int rc = m->sync();
    if (rc) return rc;
    if ((rc = m->trc_release())) return rc;
    m->drop_graph();
    const size_t ntiles = (size_t)((capacity + kTrcBlock - 1) / kTrcBlock);
    const size_t head = (256 + 2 * ntiles * 4 + 255) & ~(size_t)255;
    const size_t arr = ((size_t)capacity * 8 + 255) & ~(size_t)255;
    const size_t bytes = head + 6 * arr;
    char *pool = nullptr;
    HIP_TRY(hipMalloc((void **)&pool, bytes));
    m->trc_pool = pool;
    m->trc_bytes = bytes;
    HIP_TRY(hipMemset(pool, 0, bytes));
    Tracers &t = m->trc;
    t.tc = (TrcCtl *)pool;
    t.tile_cnt = (uint32_t *)(pool + 256);
    t.tile_off = t.tile_cnt + ntiles;
    double **arrs[6] = {&t.x0, &t.y0, &t.i0, &t.x1, &t.y1, &t.i1};
    for (int k = 0; k < 6; ++k) *arrs[k] = (double *)(pool + head + (size_t)k * arr);
    t.cap = (uint32_t)capacity;
    t.interval = inject_interval <= 0 ? 100u : (uint32_t)inject_interval;   // tracerInjectionInterval :1534
    t.dx = (double)m->g.dx;
    t.dy = (double)m->g.dy;
    t.lx = (double)m->grid.lx;
    t.ly = (double)m->grid.ly;
    // grid from the capacity; CFD_TRACER_WGS=N caps it (any N >= 1 gives the same bits)
    long grid = std::min<long>((long)ntiles, 8l * std::max(1, m->g.n_cu));
    if (const long cap = env_long("CFD_TRACER_WGS", 0); cap >= 1) grid = std::min<long>(grid, cap);
    m->trc_grid = (int)std::max(1l, grid);
    if ((rc = m->ck_drop_pool())) return rc;
    m->ck_segs.push_back({pool, bytes});
    launch_trc_inject(m->g, t, m->stream);   // initTracers (:1475-1483): the list was empty
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));
    return 0;
}

int cfd_tracers_disable(cfd_model *m) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (!m->trc_pool) return 0;
    int rc = m->sync();
    if (rc) return rc;
    return m->trc_release();
}

int cfd_tracers_count(cfd_model *m, uint64_t *n) {
    TrcCtl tc;
    int rc = trc_read(m, &tc);
    if (rc) return rc;
    if (n) *n = tc.count;
    return 0;
}

int cfd_tracers_get(cfd_model *m, double *x, double *y, double *initial_y, uint64_t max,
                    uint64_t *n_out) {
    TrcCtl tc;
    int rc = trc_read(m, &tc);
    if (rc) return rc;
    const Tracers &t = m->trc;
    const size_t n = (size_t)std::min<uint64_t>(tc.count, max);
    if (x && n) HIP_TRY(hipMemcpy(x, tc.cur ? t.x1 : t.x0, n * 8, hipMemcpyDeviceToHost));
    if (y && n) HIP_TRY(hipMemcpy(y, tc.cur ? t.y1 : t.y0, n * 8, hipMemcpyDeviceToHost));
    if (initial_y && n) HIP_TRY(hipMemcpy(initial_y, tc.cur ? t.i1 : t.i0, n * 8, hipMemcpyDeviceToHost));
    if (n_out) *n_out = n;
    return 0;
}

int cfd_tracers_set(cfd_model *m, const double *x, const double *y, const double *initial_y,
                    uint64_t n) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (!m->trc_pool) return fail(CFD_ESTATE, "tracers are not enabled (cfd_tracers_enable)");
    if (n > m->trc.cap) return fail(CFD_EINVAL, "more tracers than the capacity");
    if (n && (!x || !y || !initial_y)) return fail(CFD_EINVAL, "null tracer array");
    for (uint64_t k = 0; k < n; ++k)
        if (!std::isfinite(x[k]) || !std::isfinite(y[k]) || !std::isfinite(initial_y[k]))
            return fail(CFD_EINVAL, "non-finite tracer coordinate at index " + std::to_string(k));
    int rc = m->sync();
    if (rc) return rc;
    const Tracers &t = m->trc;
    if (n) {
        HIP_TRY(hipMemcpy(t.x0, x, (size_t)n * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t.y0, y, (size_t)n * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(t.i0, initial_y, (size_t)n * 8, hipMemcpyHostToDevice));
    }
    TrcCtl tc{};
    tc.count = (uint32_t)n;   // buffer 0, no overflow, ticket 0
    HIP_TRY(hipMemcpy(t.tc, &tc, sizeof(TrcCtl), hipMemcpyHostToDevice));
    return 0;
}

int cfd_tracers_advance(cfd_model *m, double dt) {
    int rc = trc_begin_call(m);
    if (rc) return rc;
    launch_trc_step(m->g, m->f, m->trc, m->trc_grid, false, dt, m->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cfd_tracers_inject(cfd_model *m) {
    int rc = trc_begin_call(m);
    if (rc) return rc;
    launch_trc_inject(m->g, m->trc, m->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cfd_tracers_density(cfd_model *m, uint32_t *counts_nx_ny) {
    TrcCtl tc;
    int rc = trc_read(m, &tc);
    if (rc) return rc;
    if (!counts_nx_ny) return fail(CFD_EINVAL, "null counts");
    const size_t cells = (size_t)m->g.nx * (size_t)m->g.ny;
    if (!m->trc_dens) HIP_TRY(hipMalloc((void **)&m->trc_dens, cells * 4));
    HIP_TRY(hipMemsetAsync(m->trc_dens, 0, cells * 4, m->stream));
    launch_trc_density(m->g, m->trc, m->trc_grid, m->trc_dens, m->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(counts_nx_ny, m->trc_dens, cells * 4, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return 0;
}

// ---- the script's substep (index.html:366-930; kernels in cfd_script_step.hip) ----
}  // extern "C"

namespace cfd {

int script_check(cfd_model *m, const cfd_script_step *s) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (!s) return fail(CFD_EINVAL, "null cfd_script_step");
    if (m->sharded())
        return fail(CFD_EINVAL, "the script substep runs on one domain only");
    if (m->params.bc_kind != CFD_BC_CHANNEL)
        return fail(CFD_EINVAL, "the script substep has the channel boundary conditions only");
    if (m->params.pressure_solver != CFD_SOLVER_MULTIGRID &&
        m->params.pressure_solver != CFD_SOLVER_SOR_LEX &&
        m->params.pressure_solver != CFD_SOLVER_JACOBI_SCRIPT)
        return fail(CFD_EINVAL, "the script substep needs pressure_solver 2 (multigrid), 4 "
                                "(script-order SOR) or 5 (the script's Jacobi): the others are not "
                                "the script's");
    if (s->scheme != CFD_SCRIPT_FIRST && s->scheme != CFD_SCRIPT_SECOND && s->scheme != CFD_SCRIPT_QUICK)
        return fail(CFD_EINVAL, "script scheme must be 0 (first), 1 (second) or 2 (quick)");
    if (s->inlet_profile != CFD_INLET_UNIFORM && s->inlet_profile != CFD_INLET_PARABOLIC)
        return fail(CFD_EINVAL, "unknown inlet profile");
    if (!std::isfinite(s->dt_sub) || !(s->dt_sub > 0.0))
        return fail(CFD_EINVAL, "dt_sub must be finite and positive");
    if (!std::isfinite(s->inlet_velocity)) return fail(CFD_EINVAL, "inlet_velocity must be finite");
    if (!script_step_ok(m->g, m->f))
        return fail(CFD_EINVAL, "grid too large for the script substep's row loads (2 GiB per field)");
    return 0;
}

}  // namespace cfd

// one checked substep, enqueued: cfd_script_piso_step's body, and each substep
// of cfd_script_update
int cfd_model::script_substep(const cfd_script_step *s) {
    HIP_TRY(hipSetDevice(device));
    if (int rc = need_star()) return rc;
    if (int rc = invalidate_sums()) return rc;
    if (int rc = ck_begin()) return rc;
    cfd_model *m = this;
    const cfd_script_step st = *s;
    auto run = [m, st]() {
        ScriptStep k;
        if (int rc = m->script_prepare(&st, &k)) return rc;
        launch_script_predict(m->g, m->f, k, st.scheme, m->stream);
        HIP_TRY(hipGetLastError());
        if (int rc = m->enqueue_solve(-1)) return rc;
        launch_script_correct(m->g, m->f, k, m->stream);
        HIP_TRY(hipGetLastError());
        return 0;
    };
    m->ck_record(run);
    return run();
}

extern "C" {

int cfd_script_piso_step(cfd_model *m, const cfd_script_step *s) {
    if (int rc = script_check(m, s)) return rc;
    return m->script_substep(s);
}

int cfd_script_phase(cfd_model *m, int phase, const cfd_script_step *s) {
    if (int rc = script_check(m, s)) return rc;
    if (phase != CFD_SCRIPT_PHASE_PREDICT && phase != CFD_SCRIPT_PHASE_CORRECT)
        return fail(CFD_EINVAL, "unknown script phase");
    HIP_TRY(hipSetDevice(m->device));
    if (int rc = m->need_star()) return rc;
    if (int rc = m->invalidate_sums()) return rc;
    ScriptStep k;
    if (int rc = m->script_prepare(s, &k)) return rc;
    if (phase == CFD_SCRIPT_PHASE_PREDICT)
        launch_script_predict(m->g, m->f, k, s->scheme, m->stream);
    else
        launch_script_correct(m->g, m->f, k, m->stream);
    HIP_TRY(hipGetLastError());
    return m->sync();
}

}  // extern "C"
