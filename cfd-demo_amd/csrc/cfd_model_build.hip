// cfd_model_build.hip — options, validation, creation and destruction of a model
// (the host runtime behind include/cfd.h; see cfd_model.h)
#include <algorithm>
#include <cstring>

#include "cfd_model.h"

using namespace cfd;

namespace cfd {

// The model's options table (cfd_options has each field's meaning and
// default): the environment as it stands when the model is created.
cfd_options read_options() {
    cfd_options o;
    o.sor_fused = env_flag("CFD_SOR_FUSED", true);
    o.mg_partition = env_flag("CFD_MG_PARTITION", true);
    o.spec = env_flag("CFD_SPEC", true);
    o.spec_lag = env_flag("CFD_SPEC_LAG", true);
    o.spec_slabs = env_flag("CFD_SPEC_SLABS", true);
    o.persist = env_int("CFD_PERSIST", -1);
    o.persist_sharded = env_flag("CFD_PERSIST_SHARDED", false);
    o.persist_gate = env_flag("CFD_PERSIST_GATE", false);
    o.resident = env_int("CFD_RESIDENT", -1);
    o.copy_div = env_flag("CFD_COPY_DIV", true);
    o.pred_vec = env_flag("CFD_PRED_VEC", true);
    o.corr_vec = env_flag("CFD_CORR_VEC", true);
    o.corr_head = env_flag("CFD_CORR_HEAD", true);
    o.uv_fused = env_int("CFD_UV_FUSED", kEnvUnset);
    o.graph = env_flag("CFD_GRAPH", false);
    o.ckpt = env_flag("CFD_CKPT", true);
    o.fastdiv = env_int("CFD_FASTDIV", kEnvUnset);
    o.resident_div = env_int("CFD_RESIDENT_DIV", kEnvUnset);
    o.pred_div = env_int("CFD_PRED_DIV", kEnvUnset);
    o.tb_kind = env_int("CFD_TB_KIND", kEnvUnset);
    o.temporal = env_int("CFD_TEMPORAL", kEnvUnset);
    o.tb_rows = env_int("CFD_TB_ROWS", kEnvUnset);
    o.tb_bpc = env_int("CFD_TB_BPC", kEnvUnset);
    o.xcd_remap = env_int("CFD_XCD_REMAP", kEnvUnset);
    o.rccl_timeout_s = std::max(1.0, env_double("CFD_RCCL_TIMEOUT_S", 300.0));
    return o;
}

int validate(const cfd_grid *grid, const cfd_params *p) {
    if (!grid || !p) return fail(CFD_EINVAL, "null grid or params");
    if (grid->nx < 16 || grid->nx % 8 != 0)
        return fail(CFD_EINVAL, "nx must be a multiple of 8 and >= 16 (model.rs:541 precondition)");
    if (grid->ny < 4) return fail(CFD_EINVAL, "ny must be >= 4");
    if ((grid->nx + 1) * grid->ny > (1ull << 31))
        return fail(CFD_EINVAL, "grid too large for 32-bit row indexing");
    if (!(grid->lx > 0.f) || !(grid->ly > 0.f)) return fail(CFD_EINVAL, "lx, ly must be > 0");
    if (p->jacobi_iters < 0 || p->jacobi_iters > kMaxSweeps)
        return fail(CFD_EINVAL, "jacobi_iters out of range [0, 4096]");
    if (p->corrector_passes < 0 || p->corrector_passes > kMaxPasses - 1)
        return fail(CFD_EINVAL, "corrector_passes out of range [0, 63]");
    if (p->velocity_scheme != 0 && p->velocity_scheme != 1)
        return fail(CFD_EINVAL, "velocity_scheme must be 0 or 1");
    if (p->inlet_profile != 0 && p->inlet_profile != 1)
        return fail(CFD_EINVAL, "inlet_profile must be 0 or 1");
    // 3 is unassigned: it was rejected before CFD_SOLVER_SOR_LEX existed and stays so
    if (p->pressure_solver < CFD_SOLVER_JACOBI || p->pressure_solver > CFD_SOLVER_JACOBI_SCRIPT ||
        p->pressure_solver == 3)
        return fail(CFD_EINVAL, "pressure_solver must be 0 (Jacobi), 1 (SOR), 2 (multigrid), "
                                "4 (SOR in the script's order) or 5 (the script's Jacobi)");
    if (p->bc_kind != 0 && p->bc_kind != 1) return fail(CFD_EINVAL, "bc_kind must be 0 or 1");
    return 0;
}

// Sharded SOR (enqueue_sor_sharded) needs >= 1 iteration, halo depth >= 2
// and >= 16 interior rows in the slab.  Checked wherever the solver can be
// chosen (create, cfd_set_params, cfd_run_set_params), so a step never fails
// half-way through with u*, v* and rhs already written.
int validate_sharded(const cfd_model *m, const cfd_params *p) {
    if (m->n_ranks > 1 && p->pressure_solver == CFD_SOLVER_SOR_LEX)
        return fail(CFD_EINVAL, "pressure_solver 4 (SOR in the script's order) runs on one domain "
                                "only: sharded models take 0, 1 or 2");
    if (m->n_ranks > 1 && p->pressure_solver == CFD_SOLVER_JACOBI_SCRIPT)
        return fail(CFD_EINVAL, "pressure_solver 5 (the script's Jacobi) runs on one domain only: "
                                "sharded models take 0, 1 or 2");
    if (m->n_ranks <= 1 || p->pressure_solver != CFD_SOLVER_SOR) return 0;
    const int lo = std::max(0, 1 - (int)m->j0);
    const int hi = std::min((int)(m->j1 - m->j0), (int)m->grid.ny - 1 - (int)m->j0);
    if (p->jacobi_iters < 1 || m->g.hg < 2 || !sor_fused_ok((int)m->grid.nx, hi - lo))
        return fail(CFD_EINVAL, "sharded SOR needs >= 1 iteration, halo depth >= 2 and >= 16 "
                                "interior rows per slab (rank " + std::to_string(m->rank) + " has " +
                                    std::to_string(hi - lo) + ", halo depth " +
                                    std::to_string(m->g.hg) + ")");
    return 0;
}

void apply_params(cfd_model *m, const cfd_params *p) {
    m->params = *p;
    m->g.nu = p->viscosity;
    m->g.target_inlet = p->target_inlet_velocity;
    m->g.scheme = p->velocity_scheme;
    m->g.profile = p->inlet_profile;
    m->g.bc_kind = p->bc_kind;
    m->g.tol_enabled = p->tol_enabled ? 1 : 0;
    m->g.p_tol = p->p_tol;
    m->g.jacobi_iters = p->jacobi_iters;
}

// Fields::sums_track: whether the fma form of the per-launch march can ever
// run for this model -- one domain, the Jacobi solver with a fixed count, the
// grid test of lds_sums_grid (cfd_jacobi_lds.h: reciprocal multiply, dx^2 ==
// dy^2 with a power-of-two reciprocal >= 1) and the CFD_JACOBI_SUMS knob as
// it stands now.  Kernel arguments of a captured step freeze it, which is
// safe: with 0 the publishers never set Ctl::sums_state and every launch runs
// the reference's body; with 1 the launch still reads the knob itself.
// Called when the model is created and after every parameter change.
void set_sums_track(cfd_model *m) {
    const Geom &g = m->g;
    int e2 = 0;
    const bool pow2 = g.r_dx_sq >= 1.0f && std::frexp(g.r_dx_sq, &e2) == 0.5f;
    m->f.sums_track = env_flag("CFD_JACOBI_SUMS", true) && m->n_ranks == 1 && g.j0 == 0 && g.nyl == g.ny &&
                      m->params.pressure_solver == CFD_SOLVER_JACOBI && !g.tol_enabled &&
                      g.fastdiv == 1 && g.dx_sq == g.dy_sq && g.r_dx_sq == g.r_dy_sq && pow2;
}

}  // namespace cfd

namespace {

// Pick the cheapest division form that is bit-identical to IEEE `/` for ALL
// 2^32 f32 inputs, for each of the three Jacobi divisors, by exhaustive
// check on the device (a few ms; cached per divisor value).  x * RN(1/c) is
// exact e.g. for the power-of-two divisors of the 2^k cavity grids; the
// FMA-corrected form covers most other divisors; anything else keeps IEEE
// division.  CFD_FASTDIV=0 forces IEEE, CFD_FASTDIV=2 prefers the FMA-corrected form.
std::mutex g_div_mu;
std::vector<std::pair<uint32_t, int>> g_div_cache;   // divisor bits -> ok mask (bit0 m1, bit1 m2)

int division_ok_mask(hipStream_t s, float c, float r, int *mask) {
    uint32_t bits;
    std::memcpy(&bits, &c, 4);
    {
        std::lock_guard<std::mutex> lk(g_div_mu);
        for (auto &e : g_div_cache)
            if (e.first == bits) {
                *mask = e.second;
                return 0;
            }
    }
    unsigned long long *d = nullptr, h[3] = {0, 0, 0};
    HIP_TRY(hipMalloc((void **)&d, 24));
    HIP_TRY(hipMemsetAsync(d, 0, 24, s));
    launch_verify_division(c, r, d, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, d, 24, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipFree(d));
    *mask = (h[0] == 0 ? 1 : 0) | (h[1] == 0 ? 2 : 0) | (h[2] == 0 ? 4 : 0);
    std::lock_guard<std::mutex> lk(g_div_mu);
    g_div_cache.emplace_back(bits, *mask);
    return 0;
}

int choose_division(hipStream_t s, const cfd_options &opt, Geom &g) {
    g.fastdiv = 0;
    g.res_div = 0;
    if (opt.fastdiv == 0) return 0;
    int m1, m2, m3;
    int rc;
    if ((rc = division_ok_mask(s, g.dx_sq, g.r_dx_sq, &m1)) ||
        (rc = division_ok_mask(s, g.dy_sq, g.r_dy_sq, &m2)) ||
        (rc = division_ok_mask(s, g.denom, g.r_denom, &m3)))
        return rc;
    const int all = m1 & m2 & m3;
    g.fastdiv = (all & 1) ? 1 : (all & 2) ? 2 : 0;
    if (opt.fastdiv == 2 && (all & 2)) g.fastdiv = 2;   // test hook: prefer mode 2
    // the resident solve also has the guarded FMA form (3), opt-in
    // (CFD_RESIDENT_DIV=3): its per-division branch measured slower than
    // IEEE division on the reference default (3.87 vs 3.57 ms per step,
    // profiles/r4/ab_refdef_r4t.log)
    g.res_div = g.fastdiv != 0 ? g.fastdiv : (opt.resident_div == 3 && (all & 4)) ? 3 : 0;
    return 0;
}

// Model::new (model.rs:219-299), restricted to rows [j0, j1) of the slab.
int build_model(cfd_model *m, const cfd_grid *grid, const cfd_params *p, int device, int hg) {
    const cfd_options &opt = m->opt;
    m->device = device;
    m->grid = *grid;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&m->cstream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&m->ev_ov0, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&m->ev_ov1, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&m->ev_rhs, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&m->ev_uv, hipEventDisableTiming));
    HIP_TRY(hipEventCreate(&m->ev_step0));
    HIP_TRY(hipEventCreate(&m->ev_step1));
    HIP_TRY(hipEventCreate(&m->ev_prof0));
    HIP_TRY(hipEventCreate(&m->ev_prof1));
    const int nx = (int)grid->nx, ny = (int)grid->ny;
    Geom &g = m->g;
    g.nx = nx;
    g.ny = ny;
    g.j0 = (int)m->j0;
    g.nyl = (int)(m->j1 - m->j0);
    g.hg = hg;
    // the kernels address a field slab with 32-bit byte offsets
    if ((uint64_t)(g.nyl + 2 * hg + 2 * kGhostUV + 1) * (uint64_t)(nx + 1) * 4u >= (1ull << 31))
        return fail(CFD_EINVAL, "slab too large for 32-bit buffer offsets (2 GiB per field)");
    g.dx = grid->lx / (float)grid->nx;   // src/app.rs:37
    g.dy = grid->ly / (float)grid->ny;   // src/app.rs:38
    g.ly = grid->ly;
    apply_params(m, p);
    // Jacobi divisors exactly as jacobi_pressure forms them (model.rs:740-746)
    g.dx_sq = g.dx * g.dx;
    g.dy_sq = g.dy * g.dy;
    g.denom = 2.0f / (g.dx * g.dx) + 2.0f / (g.dy * g.dy);
    g.r_dx_sq = 1.0f / g.dx_sq;
    g.r_dy_sq = 1.0f / g.dy_sq;
    g.r_denom = 1.0f / g.denom;
    {
        // spacings that are exact powers of two: division == reciprocal multiply
        auto pow2f = [](float c) {
            int e;
            return c > 0.0f && std::isfinite(c) && std::frexp(c, &e) == 0.5f &&
                   std::isnormal(1.0f / c);
        };
        g.r_dx = 1.0f / g.dx;
        g.r_dy = 1.0f / g.dy;
        g.r_dxx = 1.0f / (g.dx * g.dx);
        g.r_dyy = 1.0f / (g.dy * g.dy);
        g.sp_pow2 = pow2f(g.dx) && pow2f(g.dy) && pow2f(g.dx * g.dx) && pow2f(g.dy * g.dy) ? 1 : 0;
        if (opt.fastdiv == 0) g.sp_pow2 = 0;
    }
    {
        int rc0 = choose_division(m->stream, opt, g);
        if (rc0) return rc0;
    }
    // Default Jacobi march (measured at 4096^2 on developed fields, r2:
    // profiles/r2/tune_r2b_kind5.log, ab_lds_*.log): with the proven-exact
    // reciprocal multiply, kind 5 (rhs window in LDS, DPP-folded sums) at
    // T = 8 sweeps per launch, one round of balanced segments, progress-ordered
    // issue priority and lighter boundary-row segments, 5.1-5.4 us per sweep
    // (box to box), against 7.75 for kind 4 at T = 8 and 9.04 at T = 4; under IEEE (or FMA-corrected)
    // division the march is VALU-bound and kind 4 at T = 4 stays (r1: 6144^2
    // 7.3e11 vs 6.1e11 cell-updates/s at T = 8).  Single domain and slabs alike.
    g.tb_kind = g.fastdiv == 1 ? 5 : 4;
    g.pred_div = opt.pred_div == 0 ? 0 : 2;
    if (opt.tb_kind != kEnvUnset) {
        const int k = opt.tb_kind;
        if (k != 1 && k != 4 && k != 5) return fail(CFD_EINVAL, "CFD_TB_KIND must be 1, 4 or 5");
        g.tb_kind = k;
    }
    // kind 4 parks masked lanes at a far voffset that must not wrap past 2^32
    // when the row offset is added: slabs up to 1 GiB per field (kind 5 bases
    // its descriptors at each wave's rows)
    if (g.tb_kind != 5 && (uint64_t)(g.nyl + 2 * g.hg) * (uint64_t)nx * 4u > (1ull << 30))
        g.tb_kind = 1;
    m->t_max = 4;
    {
        // kind 4 past the 256 MB Infinity Cache: 8 sweeps per launch halve the
        // HBM traffic (8192^2: 2.33e12 vs 1.38e12 cell-updates/s, r1)
        const uint64_t jac_ws = 3ull * (uint64_t)(g.nyl + 2 * g.hg) * (uint64_t)nx * 4u;
        if (g.tb_kind == 4 && g.fastdiv == 1 && m->n_ranks == 1 && jac_ws > (256ull << 20))
            m->t_max = 8;
        if (g.tb_kind == 5) m->t_max = 8;
    }
    if (opt.temporal != kEnvUnset) m->t_max = std::max(1, opt.temporal);
    m->t_max = std::min(m->t_max, g.tb_kind == 1 ? 4 : kMaxTemporal);
    // output rows per wave segment: 24 for kind 4 (12-slot unrolled march);
    // kind 5 sizes its segments to one round of resident waves (tb_rows 0,
    // cfd_jacobi_lds.hip lds_tiles; 4096^2: ~38 rows, fixed 40 rows gave
    // 6.42 us/sweep, 32 gave 6.50, 24 gave 6.68)
    g.tb_rows = g.tb_kind == 5 ? 0 : 24;
    if (opt.tb_rows != kEnvUnset) g.tb_rows = std::max(4, std::min(1024, opt.tb_rows));
    g.tb_bpc = 3;
    if (opt.tb_bpc != kEnvUnset) {   // balanced segmentation instead
        g.tb_bpc = std::max(1, std::min(16, opt.tb_bpc));
        g.tb_rows = 0;
    }
    g.xcd_remap = opt.xcd_remap == 0 ? 0 : 1;
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
            ncu <= 0)
            ncu = 256;
        g.n_cu = ncu;
    }


    const size_t W = (size_t)nx + 1, nyl = (size_t)g.nyl;
    const size_t u_alloc = round4(m->u_rows_alloc() * W);
    const size_t v_alloc = round4(m->v_rows_alloc() * (size_t)nx);
    const size_t p_n = nyl * nx;
    const size_t pp_n = (nyl + 2 * (size_t)hg) * nx;
    auto zalloc = [&](void **ptr, size_t bytes) -> int {
        HIP_TRY(hipMalloc(ptr, bytes));
        HIP_TRY(hipMemsetAsync(*ptr, 0, bytes, m->stream));
        return 0;
    };
    int rc = 0;
    if ((rc = zalloc((void **)&m->u_all, u_alloc * 4)) || (rc = zalloc((void **)&m->v_all, v_alloc * 4)) ||
        (rc = zalloc((void **)&m->uo_all, u_alloc * 4)) || (rc = zalloc((void **)&m->vo_all, v_alloc * 4)) ||
        (rc = zalloc((void **)&m->us_all, u_alloc * 4)) || (rc = zalloc((void **)&m->vs_all, v_alloc * 4)) ||
        (rc = zalloc((void **)&m->p, p_n * 4)) || (rc = zalloc((void **)&m->rhs, pp_n * 4)) ||
        (rc = zalloc((void **)&m->pp_all[0], pp_n * 4)) || (rc = zalloc((void **)&m->pp_all[1], pp_n * 4)) ||
        (rc = zalloc((void **)&m->mask_u, nyl * W + 16)) || (rc = zalloc((void **)&m->mask_v, (nyl + 1) * nx + 16)) ||
        (rc = zalloc((void **)&m->ctl, sizeof(Ctl))) ||
        (rc = zalloc((void **)&m->slots, kSlotWords * 4)))
        return rc;
    // the self-recovery checkpoint's segments (cfd_model::ck_begin)
    m->ck_segs = {{m->u_all, u_alloc * 4}, {m->v_all, v_alloc * 4}, {m->uo_all, u_alloc * 4},
                  {m->vo_all, v_alloc * 4}, {m->us_all, u_alloc * 4}, {m->vs_all, v_alloc * 4},
                  {m->p, p_n * 4},         {m->rhs, pp_n * 4},        {m->pp_all[0], pp_n * 4},
                  {m->pp_all[1], pp_n * 4}, {m->ctl, sizeof(Ctl)}};
    // word 0: first non-finite step; word 1: last finished step (watchdog)
    // [0] non-finite step, [1] progress (sharded), [2] persistent-solve timeout
    HIP_TRY(hipHostMalloc((void **)&m->h_nonfinite, 16, hipHostMallocMapped | hipHostMallocCoherent));
    *(volatile uint32_t *)m->h_nonfinite = 0u;
    *(volatile uint32_t *)(m->h_nonfinite + 1) = 0u;
    *(volatile uint32_t *)(m->h_nonfinite + 2) = 0u;
    HIP_TRY(hipHostMalloc((void **)&m->h_res, 4 * cfd_model::kResRing, hipHostMallocDefault));
    for (hipEvent_t &e : m->ev_res) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipHostMalloc((void **)&m->h_spec, 4 * cfd_model::kSpecRing * kMaxTemporal, hipHostMallocDefault));
    for (hipEvent_t &e : m->ev_spec) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));

    // obstacle masks and cell list from cell centres (model.rs:235-260)
    std::vector<uint8_t> mu(nyl * W, 0), mv((nyl + 1) * nx, 0);
    std::vector<int32_t> obs;
    if (grid->has_cylinder) {
        for (int j = 0; j < ny; ++j) {
            for (int i = 0; i < nx; ++i) {
                const float x = ((float)i + 0.5f) * g.dx;
                const float y = ((float)j + 0.5f) * g.dy;
                const float ddx = x - grid->cylinder_x;
                const float ddy = y - grid->cylinder_y;
                const float distance = std::sqrt(ddx * ddx + ddy * ddy);
                if (!(distance < grid->cylinder_radius)) continue;
                const long lj = (long)j - (long)m->j0;
                if (lj >= 0 && lj < (long)nyl) {
                    if (i > 0) mu[lj * W + i] = 1;
                    if (i < nx) mu[lj * W + i + 1] = 1;
                }
                if (j > 0 && lj >= 0 && lj <= (long)nyl) mv[lj * nx + i] = 1;
                if (j < ny && lj + 1 >= 0 && lj + 1 <= (long)nyl) mv[(lj + 1) * nx + i] = 1;
                if (lj >= 0 && lj <= (long)nyl) {
                    obs.push_back(i);
                    obs.push_back(j);
                }
            }
        }
    }
    m->h_mask_u = mu;
    m->h_mask_v = mv;
    // device masks: bit 0 = predictor mask (model.rs:235-260), bit 1 = face
    // zeroed by the obstacle loop of apply_boundary_conditions (:866-874)
    std::vector<uint8_t> dmu(mu), dmv(mv);
    for (size_t k = 0; k < obs.size(); k += 2) {
        const long oi = obs[k], lj = (long)obs[k + 1] - (long)m->j0;
        if (lj >= 0 && lj < (long)nyl) dmu[lj * W + oi] |= 2;
        if (lj >= 0 && lj <= (long)nyl) dmv[lj * nx + oi] |= 2;
    }
    m->dmask_u = std::move(dmu);
    m->dmask_v = std::move(dmv);
    HIP_TRY(hipMemcpyAsync(m->mask_u, m->dmask_u.data(), m->dmask_u.size(), hipMemcpyHostToDevice,
                           m->stream));
    HIP_TRY(hipMemcpyAsync(m->mask_v, m->dmask_v.data(), m->dmask_v.size(), hipMemcpyHostToDevice,
                           m->stream));
    if (!obs.empty()) {
        HIP_TRY(hipMalloc((void **)&m->obs, obs.size() * 4));
        HIP_TRY(hipMemcpyAsync(m->obs, obs.data(), obs.size() * 4, hipMemcpyHostToDevice, m->stream));
    }

    Fields &f = m->f;
    const size_t uoff = (size_t)kGhostUV * W, voff = (size_t)kGhostUV * nx;
    f.u_alloc_base = m->u_all;
    f.v_alloc_base = m->v_all;
    f.u_old_base = m->uo_all;
    f.v_old_base = m->vo_all;
    f.u_star_base = m->us_all;
    f.v_star_base = m->vs_all;
    f.u_alloc = u_alloc;
    f.v_alloc = v_alloc;
    f.u = m->u_all + uoff;
    f.v = m->v_all + voff;
    f.u_old = m->uo_all + uoff;
    f.v_old = m->vo_all + voff;
    f.u_star = m->us_all + uoff;
    f.v_star = m->vs_all + voff;
    f.p = m->p;
    f.rhs = m->rhs + (size_t)hg * nx;   // hg ghost rows each side (sharded solves)
    f.pp[0] = m->pp_all[0] + (size_t)hg * nx;
    f.pp[1] = m->pp_all[1] + (size_t)hg * nx;
    // the vector kernels move these rows as float4 (aligned16, cfd_internal.h)
    const std::pair<const float *, const char *> rows16[] = {
        {f.v, "v"}, {f.v_star, "v_star"}, {f.p, "p"}, {f.rhs, "rhs"}, {f.pp[0], "pp[0]"}, {f.pp[1], "pp[1]"}};
    for (const auto &r : rows16)
        if (!aligned16(r.first))
            return fail(CFD_EINVAL, std::string("field ") + r.second + " is not 16-byte aligned");
    f.mask_u = m->mask_u;
    f.mask_v = m->mask_v;
    f.obs = m->obs;
    f.n_obs = (int32_t)(obs.size() / 2);
    // without an obstacle in reach the masks are all zero and the predictors
    // skip their mask loads (a slab can hold mask rows of a cylinder whose
    // cells lie just outside it, so n_obs alone does not decide this)
    f.any_pmask = 0;
    for (uint8_t b : m->h_mask_u) f.any_pmask |= b & 1;
    for (uint8_t b : m->h_mask_v) f.any_pmask |= b & 1;
    f.ctl = m->ctl;
    {
        void *dp = nullptr;
        HIP_TRY(hipHostGetDevicePointer(&dp, m->h_nonfinite, 0));
        f.host_nonfinite = (uint32_t *)dp;
        f.host_progress = m->n_ranks > 1 ? (uint32_t *)dp + 1 : nullptr;
    }
    f.err_slots = m->slots;
    f.red_slots = m->slots + (size_t)kMaxSweeps * kResSlots * kResStride;
    f.vis_slots = f.red_slots + (size_t)4 * kResSlots * kResStride;
    f.persist = m->slots + (size_t)(kMaxSweeps + 16) * kResSlots * kResStride;

    set_sums_track(m);

    Ctl c0;
    std::memset(&c0, 0, sizeof(c0));
    c0.dt = p->dt;
    c0.go[0] = 1;
    HIP_TRY(hipMemcpyAsync(m->ctl, &c0, sizeof(Ctl), hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return 0;
}

}  // namespace

namespace cfd {

int create_model(const cfd_grid *grid, const cfd_params *params, int device, int n_ranks, int rank,
                 const void *uid, LocalHub *hub, cfd_model **out) {
    if (!out) return fail(CFD_EINVAL, "null out");
    *out = nullptr;
    int rc = validate(grid, params);
    if (rc) return rc;
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(CFD_EINVAL, "bad rank/n_ranks");
    if (n_ranks > 1 && params->pressure_solver == CFD_SOLVER_SOR_LEX)   // before any device call
        return fail(CFD_EINVAL, "pressure_solver 4 (SOR in the script's order) runs on one domain "
                                "only: sharded models take 0, 1 or 2");
    if (n_ranks > 1 && params->pressure_solver == CFD_SOLVER_JACOBI_SCRIPT)
        return fail(CFD_EINVAL, "pressure_solver 5 (the script's Jacobi) runs on one domain only: "
                                "sharded models take 0, 1 or 2");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(CFD_EHIP, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(CFD_EINVAL, "device ordinal out of range");
    cfd_model *m = new cfd_model();
    m->opt = read_options();   // once per model, here
    m->persist_on = m->opt.persist != 0;
    m->n_ranks = n_ranks;
    m->rank = rank;
    plan_slab(grid->ny, n_ranks, rank, &m->j0, &m->j1);
    int hg = 1;
    if (n_ranks > 1) {
        // Deep halos: one RCCL round every hg sweeps (a round over xGMI is
        // latency-bound, ~20-30 us) against ~hg/nyl redundant ghost-row
        // compute; default hg = nyl/32 clamped to [8, 32] (32 at the bench's
        // 1024-2048-row slabs: 7 rounds per 200-sweep step, ~3 % extra rows).
        // The floor 8 (r6; 4 before) lets the tolerance mode's speculative
        // blocks run 8 sweeps per exchange on thin slabs too (the default
        // channel on 2 ranks: 13 blocks of 4 per solve -> 7 of 8)
        uint64_t min_rows = grid->ny / (uint64_t)n_ranks;
        hg = env_int("CFD_HALO_DEPTH", (int)std::max<uint64_t>(kMaxTemporal,
                                                                std::min<uint64_t>(32, min_rows / 32)));
        if (hg < 1) hg = 1;
        if ((uint64_t)hg + 2 > min_rows) hg = (int)(min_rows > 3 ? min_rows - 2 : 1);
        if (min_rows < 4) {
            delete m;
            return fail(CFD_EINVAL, "each slab needs at least 4 rows");
        }
    }
    rc = build_model(m, grid, params, device, hg);
    if (!rc) rc = validate_sharded(m, params);
    if (!rc && n_ranks > 1 && hub) {
        if (hub->n != n_ranks) {
            rc = fail(CFD_EINVAL, "local hub size != n_ranks");
        } else {
            std::lock_guard<std::mutex> lk(hub->mu);
            hub->members[rank] = m;
            m->hub = hub;
        }
    } else if (!rc && n_ranks > 1) {
        ncclUniqueId id;
        std::memcpy(&id, uid, sizeof(id));
        rc = comm_init(m, id, n_ranks, rank);
    }
    if (rc) {
        m->destroy();
        delete m;
        return rc;
    }
    *out = m;
    return 0;
}

}  // namespace cfd

void cfd_model::destroy() {
    {   // the persistent-launch gate must not keep this model's stream
        PersistGate &gate = persist_gate(device);
        std::lock_guard<std::mutex> lk(gate.mu);
        if (gate.last == stream) gate.last = nullptr;
    }
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (comm) ncclCommDestroy(comm);
    comm = nullptr;
    for (hipEvent_t e : ev_res)
        if (e) (void)hipEventDestroy(e);
    if (h_res) (void)hipHostFree(h_res);
    for (hipEvent_t e : ev_spec)
        if (e) (void)hipEventDestroy(e);
    if (h_spec) (void)hipHostFree(h_spec);
    for (void *ptr : {(void *)u_all, (void *)v_all, (void *)uo_all, (void *)vo_all,
                      (void *)us_all, (void *)vs_all, (void *)p, (void *)rhs,
                      (void *)pp_all[0], (void *)pp_all[1], (void *)mask_u, (void *)mask_v,
                      (void *)obs, (void *)ctl, (void *)slots, (void *)vis_buf,
                      (void *)mg_pool, (void *)mg_dev, (void *)lex_pol, (void *)lex_exit,
                      (void *)res64})
        if (ptr) (void)hipFree(ptr);
    if (h_nonfinite) (void)hipHostFree(h_nonfinite);
    if (ck_pool) (void)hipFree(ck_pool);
    if (trc_pool) (void)hipFree(trc_pool);
    if (trc_dens) (void)hipFree(trc_dens);
    if (scr_pool) (void)hipFree(scr_pool);
    if (su_pool) (void)hipFree(su_pool);
    if (su_h) (void)hipHostFree(su_h);
    drop_graph();
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    if (ev_step0) (void)hipEventDestroy(ev_step0);
    if (ev_step1) (void)hipEventDestroy(ev_step1);
    if (ev_prof0) (void)hipEventDestroy(ev_prof0);
    if (ev_prof1) (void)hipEventDestroy(ev_prof1);
    if (stream) (void)hipStreamDestroy(stream);
    if (cstream) (void)hipStreamDestroy(cstream);
    if (ev_ov0) (void)hipEventDestroy(ev_ov0);
    if (ev_ov1) (void)hipEventDestroy(ev_ov1);
    if (ev_rhs) (void)hipEventDestroy(ev_rhs);
    if (ev_uv) (void)hipEventDestroy(ev_uv);
}
