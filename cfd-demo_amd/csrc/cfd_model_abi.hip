// cfd_model_abi.hip — the extern "C" surface of include/cfd.h
// (the host runtime behind include/cfd.h; see cfd_model.h)
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "cfd_model.h"

using namespace cfd;

namespace {
thread_local std::string g_last_error;   // the one object behind cfd_last_error()
}  // namespace

int cfd::fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

extern "C" {

const char *cfd_last_error(void) { return g_last_error.c_str(); }
// internal (not in cfd.h): lets the host runtime (cfd_runtime.cpp) report
// through the same thread-local message
void cfdrt_set_error(const char *msg) { g_last_error = msg ? msg : ""; }
// internal: the host-only checks cfd_set_params makes, for cfd_run_set_params
// to reject bad parameters synchronously (reads only the immutable grid)
int cfdrt_check_params(const cfd_model *m, const cfd_params *p) {
    if (!m) return fail(CFD_EINVAL, "null model");
    int rc = validate(&m->grid, p);
    if (rc) return rc;
    return validate_sharded(m, p);
}

int cfd_get_config(const cfd_model *m, cfd_grid *grid, cfd_params *params) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (grid) *grid = m->grid;
    if (params) *params = m->params;
    return 0;
}
int cfd_abi_version(void) { return CFD_ABI_VERSION; }

void cfd_default_params(cfd_params *o) {
    if (!o) return;
    o->dt = 0.005f;                  // model.rs:47
    o->viscosity = 0.000001f;        // model.rs:48
    o->target_inlet_velocity = 1.0f; // model.rs:49
    o->velocity_scheme = CFD_SCHEME_FIRST_ORDER;
    o->inlet_profile = CFD_INLET_UNIFORM;
    o->pressure_solver = CFD_SOLVER_JACOBI;
    o->jacobi_iters = 50;            // model.rs:737
    o->corrector_passes = 20;        // model.rs:696
    o->tol_enabled = 1;
    o->p_tol = 1e-4f;                // model.rs:736, 721
    o->bc_kind = CFD_BC_CHANNEL;
}

void cfd_default_grid(cfd_grid *o) {
    if (!o) return;
    o->nx = 800;                     // src/app.rs:34
    o->ny = 264;
    o->lx = 30.0f;
    o->ly = 10.0f;
    o->has_cylinder = 1;
    o->cylinder_x = 30.0f / 4.0f;    // src/app.rs:47
    o->cylinder_y = 10.0f / 2.0f;
    o->cylinder_radius = 0.75f;
}

int cfd_create(const cfd_grid *grid, const cfd_params *params, int device_ordinal, cfd_model **out) {
    return create_model(grid, params, device_ordinal, 1, 0, nullptr, nullptr, out);
}

int cfd_create_sharded(const cfd_grid *grid, const cfd_params *params, int device_ordinal,
                       int n_ranks, int rank, const void *uid, cfd_model **out) {
    if (n_ranks > 1 && !uid) return fail(CFD_EINVAL, "null rccl unique id");
    return create_model(grid, params, device_ordinal, n_ranks, rank, uid, nullptr, out);
}

int cfd_create_sharded_local(const cfd_grid *grid, const cfd_params *params, int device_ordinal,
                             int n_ranks, int rank, void *hub, cfd_model **out) {
    if (!hub) return fail(CFD_EINVAL, "null local hub");
    return create_model(grid, params, device_ordinal, n_ranks, rank, nullptr,
                         static_cast<LocalHub *>(hub), out);
}

int cfd_device_count(int *n_out) {
    if (!n_out) return fail(CFD_EINVAL, "null out");
    *n_out = 0;
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess && e != hipErrorNoDevice)
        return fail(CFD_EHIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    *n_out = e == hipSuccess ? n : 0;
    return 0;
}

int cfd_get_comm_size(const cfd_model *m, int *n_out) {
    if (!m || !n_out) return fail(CFD_EINVAL, "null model or out");
    if (m->hub) {
        *n_out = m->hub->n;
    } else if (m->comm) {
        int n = 0;
        RCCL_TRY(ncclCommCount(m->comm, &n));
        *n_out = n;
    } else if (m->n_ranks > 1) {
        return fail(CFD_ERCCL, "the RCCL communicator was aborted after an earlier failure");
    } else {
        *n_out = 1;
    }
    return 0;
}

int cfd_get_slab(const cfd_model *m, uint64_t *j0, uint64_t *j1) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (j0) *j0 = m->j0;
    if (j1) *j1 = m->j1;
    return 0;
}

int cfd_update(cfd_model *m) { return cfd_update_n(m, 1); }

int cfd_update_n(cfd_model *m, int n) {
    if (!m) return fail(CFD_EINVAL, "null model");
    HIP_TRY(hipSetDevice(m->device));
    // a solve timeout first (its junk steps may have raised the non-finite
    // flag too): recovered from the checkpoint, reported once
    if (int rc = m->persist_timeout_check(false)) return rc;
    // failure detection: a step the device has already finished left a NaN or
    // Inf in u/v (zero-copy word, no stream synchronisation)
    if (const uint32_t bad = *(volatile uint32_t *)m->h_nonfinite)
        return fail(CFD_ENONFINITE, "non-finite velocity (NaN/Inf) after step " + std::to_string(bad) +
                                        "; cfd_set_state clears it");
    if (n <= 0) return 0;
    if (int rc = m->ck_begin()) return rc;
    m->ck_record([m, n]() {
        for (int k = 0; k < n; ++k)
            if (int rc = m->enqueue_update(k == n - 1)) return rc;
        return 0;
    });
    // solve timing: one event pair around the whole batch for the step time
    if (m->timing) {
        hipEvent_t e0 = m->take_event();
        HIP_TRY(hipEventRecord(e0, m->stream));
        m->step_events.push_back(e0);
    }
    int rc = 0;
    if (m->graph_ok()) {
        rc = m->update_graph(n);
    } else {
        for (int k = 0; k < n && !rc; ++k) rc = m->enqueue_update(k == n - 1);
    }
    if (m->timing) {
        hipEvent_t e1 = m->take_event();
        HIP_TRY(hipEventRecord(e1, m->stream));
        m->step_events.push_back(e1);
    }
    return rc;
}

int cfd_piso_step(cfd_model *m, float dt_sub) {
    if (!m) return fail(CFD_EINVAL, "null model");
    HIP_TRY(hipSetDevice(m->device));
    if (int rc = m->need_star()) return rc;
    if (int rc = m->invalidate_sums()) return rc;
    if (int rc = m->ck_begin()) return rc;
    auto run = [m, dt_sub]() {
        int rc = m->exchange_uv();
        if (!rc) rc = m->enqueue_piso(dt_sub);
        return rc ? rc : m->abort_allreduce();
    };
    m->ck_record(run);
    return run();
}

int cfd_pressure_solve(cfd_model *m, float *residual_out) {
    if (!m) return fail(CFD_EINVAL, "null model");
    HIP_TRY(hipSetDevice(m->device));
    int rc;
    if ((rc = m->invalidate_sums())) return rc;
    if (m->host_driven()) {
        return m->enqueue_solve_host_driven(residual_out);
    }
    if ((rc = m->ck_begin())) return rc;
    auto run = [m]() {
        int rc2 = m->enqueue_solve(-1);
        return rc2 ? rc2 : m->abort_allreduce();
    };
    m->ck_record(run);
    rc = run();
    if (rc) return rc;
    Ctl c;
    rc = m->read_ctl(&c);
    if (rc) return rc;
    if (residual_out) *residual_out = c.last_p;
    return 0;
}

int cfd_run_phase(cfd_model *m, int phase, float dt_sub) {
    if (!m) return fail(CFD_EINVAL, "null model");
    HIP_TRY(hipSetDevice(m->device));
    if (int rc = m->need_star()) return rc;
    if (int rc = m->invalidate_sums()) return rc;
    switch (phase) {
    case CFD_PHASE_U_PREDICTOR: {
        int rc = m->exchange_uv();
        if (rc) return rc;
        launch_u_predictor(m->g, m->f, dt_sub, m->stream);
        break;
    }
    case CFD_PHASE_V_PREDICTOR: {
        int rc = m->exchange_uv();
        if (rc) return rc;
        launch_v_predictor(m->g, m->f, dt_sub, m->stream);
        break;
    }
    case CFD_PHASE_DIVERGENCE: launch_divergence(m->g, m->f, -1, dt_sub, m->stream); break;
    case CFD_PHASE_CORRECTOR: launch_corrector(m->g, m->f, -1, dt_sub, m->opt.corr_vec, m->stream); break;
    case CFD_PHASE_BOUNDARY: launch_boundary(m->g, m->f, m->stream); break;
    default: return fail(CFD_EINVAL, "unknown phase");
    }
    HIP_TRY(hipGetLastError());
    return m->sync();
}

int cfd_set_params(cfd_model *m, const cfd_params *p) {
    if (!m) return fail(CFD_EINVAL, "null model");
    int rc = validate(&m->grid, p);
    if (rc) return rc;
    rc = validate_sharded(m, p);
    if (rc) return rc;
    rc = m->need_star();   // with the parameters the step ran under
    if (rc) return rc;
    rc = m->sync();
    if (rc) return rc;
    m->drop_graph();   // kernel arguments follow the parameters
    {
        // host mirror of the current p' buffer (the tolerance-driven Jacobi
        // solve flips it on the device); fixed-count and in-place solves use it
        Ctl c;
        rc = m->read_ctl(&c);
        if (rc) return rc;
        m->host_cur = c.cur;
    }
    apply_params(m, p);
    set_sums_track(m);
    rc = m->invalidate_sums();
    if (rc) return rc;
    // set_parameters overwrites dt (model.rs:1252)
    HIP_TRY(hipMemcpy(&m->ctl->dt, &p->dt, 4, hipMemcpyHostToDevice));
    return 0;
}

int cfd_get_snapshot(cfd_model *m, float *u, float *v, float *p, float *dt_out) {
    if (!m) return fail(CFD_EINVAL, "null model");
    int rc = m->sync();
    if (rc) return rc;
    const size_t W = (size_t)m->g.nx + 1, nx = (size_t)m->g.nx, nyl = (size_t)m->g.nyl;
    if (u) HIP_TRY(hipMemcpy(u, m->f.u, nyl * W * 4, hipMemcpyDeviceToHost));
    if (v) HIP_TRY(hipMemcpy(v, m->f.v, (nyl + 1) * nx * 4, hipMemcpyDeviceToHost));
    if (p) HIP_TRY(hipMemcpy(p, m->f.p, nyl * nx * 4, hipMemcpyDeviceToHost));
    if (dt_out) HIP_TRY(hipMemcpy(dt_out, &m->ctl->dt, 4, hipMemcpyDeviceToHost));
    return 0;
}

namespace {

float decode_key(uint32_t k, bool is_min) {   // inverse of ord_key (cfd_render.hip)
    if (is_min) {
        if (!k) return INFINITY;
        k = ~k;
    } else if (!k) {
        return -INFINITY;
    }
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float x;
    std::memcpy(&x, &b, 4);
    return x;
}

// cfd_render / cfd_derive_field: field or image of `mode` for the model's
// slab, min/max reduced over ranks, one D2H copy of nx*nyl words.
int render_common(cfd_model *m, int mode, bool field, void *host_out, float *min_max_out) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (mode < CFD_VIS_PRESSURE || mode > CFD_VIS_VORTICITY)
        return fail(CFD_EINVAL, "unknown visualisation mode");
    HIP_TRY(hipSetDevice(m->device));
    const size_t n = (size_t)m->g.nx * (size_t)m->g.nyl;
    if (!m->vis_buf) HIP_TRY(hipMalloc((void **)&m->vis_buf, n * 4));
    if (mode == CFD_VIS_VORTICITY) {   // reads u/v one row above the slab
        int rc = m->exchange_uv();
        if (rc) return rc;
    }
    Fields &f = m->f;
    launch_vis_field(m->g, f, mode, field ? m->vis_buf : nullptr, f.vis_slots, m->stream);
    launch_fold_slots(f.ctl->vis, f.vis_slots, 2, m->stream);
    int rc = m->allreduce_max_u32(f.ctl->vis, 2);
    if (rc) return rc;
    const cfd_grid &gr = m->grid;
    if (!field && host_out)
        launch_vis_color(m->g, f, mode, nullptr, (uint32_t *)m->vis_buf, f.ctl->vis,
                         gr.has_cylinder, gr.cylinder_x, gr.cylinder_y, gr.cylinder_radius,
                         m->stream);
    HIP_TRY(hipGetLastError());
    uint32_t keys[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(keys, f.ctl->vis, 8, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipMemsetAsync(f.ctl->vis, 0, 8, m->stream));
    if (host_out) HIP_TRY(hipMemcpyAsync(host_out, m->vis_buf, n * 4, hipMemcpyDeviceToHost, m->stream));
    if (int rc2 = m->wait_done(nullptr)) return rc2;
    if (min_max_out) {
        min_max_out[0] = decode_key(keys[1], true);
        min_max_out[1] = decode_key(keys[0], false);
    }
    return 0;
}

}  // namespace

int cfd_render(cfd_model *m, int mode, uint8_t *rgba, float *min_max_out) {
    return render_common(m, mode, false, rgba, min_max_out);
}

int cfd_derive_field(cfd_model *m, int mode, float *out, float *min_max_out) {
    return render_common(m, mode, true, out, min_max_out);
}

int cfd_get_residuals(cfd_model *m, cfd_residuals *out) {
    if (!m || !out) return fail(CFD_EINVAL, "null argument");
    Ctl c;
    int rc = m->read_ctl(&c);
    if (rc) return rc;
    out->simulation_step = c.step;
    out->simulation_time = c.time;
    out->dt = c.dt;
    out->p = c.last_p;
    out->u = c.res_u;
    out->v = c.res_v;
    out->piso_substeps = 1;   // substep_count (model.rs:267)
    out->jacobi_sweeps_total = c.sweeps_total;
    float ms = 0.f;
    if (m->stepped && hipEventElapsedTime(&ms, m->ev_step0, m->ev_step1) == hipSuccess)
        out->step_time_s = ms * 1e-3;
    else
        out->step_time_s = 0.0;
    if (c.nonfinite_step)   // *out is filled all the same
        return fail(CFD_ENONFINITE, "non-finite velocity (NaN/Inf) after step " +
                                        std::to_string(c.nonfinite_step));
    return 0;
}

int cfd_get_state(cfd_model *m, cfd_state *st) {
    if (!m || !st) return fail(CFD_EINVAL, "null argument");
    Ctl c;
    int rc = m->need_star();
    if (rc) return rc;
    rc = m->read_ctl(&c);
    if (rc) return rc;
    const size_t W = (size_t)m->g.nx + 1, nx = (size_t)m->g.nx, nyl = (size_t)m->g.nyl;
    if (st->u) HIP_TRY(hipMemcpy(st->u, m->f.u, nyl * W * 4, hipMemcpyDeviceToHost));
    if (st->v) HIP_TRY(hipMemcpy(st->v, m->f.v, (nyl + 1) * nx * 4, hipMemcpyDeviceToHost));
    if (st->p) HIP_TRY(hipMemcpy(st->p, m->f.p, nyl * nx * 4, hipMemcpyDeviceToHost));
    if (st->u_star) HIP_TRY(hipMemcpy(st->u_star, m->f.u_star, nyl * W * 4, hipMemcpyDeviceToHost));
    if (st->v_star) HIP_TRY(hipMemcpy(st->v_star, m->f.v_star, (nyl + 1) * nx * 4, hipMemcpyDeviceToHost));
    if (st->p_prime) HIP_TRY(hipMemcpy(st->p_prime, m->f.pp[c.cur], nyl * nx * 4, hipMemcpyDeviceToHost));
    if (st->rhs) HIP_TRY(hipMemcpy(st->rhs, m->f.rhs, nyl * nx * 4, hipMemcpyDeviceToHost));
    st->dt = c.dt;
    st->simulation_time = c.time;
    st->simulation_step = c.step;
    st->last_p_residual = c.last_p;
    st->last_u_residual = c.res_u;
    st->last_v_residual = c.res_v;
    st->jacobi_sweeps_total = c.sweeps_total;
    return 0;
}

int cfd_set_state(cfd_model *m, const cfd_state *st) {
    if (!m || !st) return fail(CFD_EINVAL, "null argument");
    Ctl c;
    int rc = m->need_star();   // the fields the caller leaves out keep their values
    if (rc) return rc;
    rc = m->read_ctl(&c);
    if (rc) return rc;
    const size_t W = (size_t)m->g.nx + 1, nx = (size_t)m->g.nx, nyl = (size_t)m->g.nyl;
    if (st->u) HIP_TRY(hipMemcpy(m->f.u, st->u, nyl * W * 4, hipMemcpyHostToDevice));
    if (st->v) HIP_TRY(hipMemcpy(m->f.v, st->v, (nyl + 1) * nx * 4, hipMemcpyHostToDevice));
    if (st->p) HIP_TRY(hipMemcpy(m->f.p, st->p, nyl * nx * 4, hipMemcpyHostToDevice));
    if (st->u_star) HIP_TRY(hipMemcpy(m->f.u_star, st->u_star, nyl * W * 4, hipMemcpyHostToDevice));
    if (st->v_star) HIP_TRY(hipMemcpy(m->f.v_star, st->v_star, (nyl + 1) * nx * 4, hipMemcpyHostToDevice));
    if (st->p_prime) HIP_TRY(hipMemcpy(m->f.pp[c.cur], st->p_prime, nyl * nx * 4, hipMemcpyHostToDevice));
    if (st->rhs) HIP_TRY(hipMemcpy(m->f.rhs, st->rhs, nyl * nx * 4, hipMemcpyHostToDevice));
    c.dt = st->dt;
    c.time = st->simulation_time;
    c.step = (uint32_t)st->simulation_step;
    c.last_p = st->last_p_residual;
    c.res_u = st->last_u_residual;
    c.res_v = st->last_v_residual;
    c.sweeps_total = st->jacobi_sweeps_total;
    c.nonfinite_step = 0;   // a new state: failure detection starts over
    c.red[4] = 0;
    c.red[6] = 0;           // and an old solve timeout with it
    c.sums_state = 0;       // a new p' / rhs: the fma form's maxima describe the old ones
    c.sums_m0 = 0;
    rc = m->clear_abort_words();
    if (rc) return rc;
    HIP_TRY(hipMemcpy(m->f.ctl, &c, offsetof(Ctl, go), hipMemcpyHostToDevice));
    // a new state: no solve has published its double residual
    HIP_TRY(hipMemset(&m->f.ctl->last_p64, 0, 8));
    m->p64_valid = false;
    *(volatile uint32_t *)m->h_nonfinite = 0u;
    m->host_cur = c.cur;
    // ghosts of the injected slab
    rc = m->exchange_uv();
    if (rc) return rc;
    rc = m->exchange_pp(c.cur, m->g.hg);
    if (rc) return rc;
    return m->sync();
}

int cfd_script_set_options(cfd_model *m, const cfd_script_options *o) {
    if (!m || !o) return fail(CFD_EINVAL, "null argument");
    if (m->sharded()) return fail(CFD_EINVAL, "script options need a single-domain model");
    if ((o->residual_f64 != 0 && o->residual_f64 != 1) ||
        (o->residual_scaling != 0 && o->residual_scaling != 1))
        return fail(CFD_EINVAL, "script options take 0 or 1");
    if (int rc = m->sync()) return rc;
    m->drop_graph();   // the solve's kernels follow the option
    cfd_script_options n = *o;
    if (n.residual_scaling) n.residual_f64 = 1;
    if (n.residual_f64 && !m->res64) {
        HIP_TRY(hipMalloc((void **)&m->res64, kRes64Words * 8));
        if (int rc = m->clear_res64()) return rc;
    }
    if (!n.residual_f64) {
        m->p64_valid = false;
        if (m->res64) HIP_TRY(hipFree(m->res64));   // the device is idle (sync above)
        m->res64 = nullptr;
    }
    m->sopt = n;
    return 0;
}

int cfd_script_get_options(const cfd_model *m, cfd_script_options *o) {
    if (!m || !o) return fail(CFD_EINVAL, "null argument");
    *o = m->sopt;
    return 0;
}

int cfd_get_p_residual_f64(cfd_model *m, double *last, double *step_max) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (!m->sopt.residual_f64) return fail(CFD_ESTATE, "residual_f64 is off (cfd_script_set_options)");
    if (!m->p64_valid)
        return fail(CFD_ESTATE, "no solve has published a double residual: none has run since the option "
                                "was set or the state was replaced, or the last one was solver 0 or 1");
    if (int rc = m->sync()) return rc;
    if (last) HIP_TRY(hipMemcpy(last, &m->f.ctl->last_p64, 8, hipMemcpyDeviceToHost));
    if (step_max) *step_max = m->su_pmax64;
    return 0;
}

int cfd_get_masks(cfd_model *m, uint8_t *mask_u, uint8_t *mask_v) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (mask_u) std::memcpy(mask_u, m->h_mask_u.data(), m->h_mask_u.size());
    if (mask_v) std::memcpy(mask_v, m->h_mask_v.data(), m->h_mask_v.size());
    return 0;
}

int cfd_synchronize(cfd_model *m) {
    if (!m) return fail(CFD_EINVAL, "null model");
    return m->sync();
}

int cfd_profile_sweeps(cfd_model *m, int n_sweeps, double *avg_ms_out) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (n_sweeps < 1 || n_sweeps > kMaxSweeps) return fail(CFD_EINVAL, "n_sweeps out of range");
    HIP_TRY(hipSetDevice(m->device));
    // sweeps p' outside a step, like the other entry points that drop the fma
    // form's bounds (its finalize below resets them as well)
    if (int rc = m->invalidate_sums()) return rc;
    const int lo = std::max(0, 1 - (int)m->j0), hi = std::min(m->g.nyl, (int)m->g.ny - 1 - (int)m->j0);
    hipEvent_t a = m->ev_prof0, b = m->ev_prof1;
    Geom g = m->g;
    g.tol_enabled = 0;
    HIP_TRY(hipEventRecord(a, m->stream));
    for (int it = 0; it < n_sweeps; ++it)
        launch_jacobi_sweep(g, m->f, -1, it, lo, hi, it == n_sweeps - 1, m->stream);
    HIP_TRY(hipEventRecord(b, m->stream));
    launch_finalize_solve(g, m->f, -1, n_sweeps, 0, n_sweeps, m->stream);
    HIP_TRY(hipGetLastError());
    m->host_cur = (m->host_cur + n_sweeps) & 1;
    m->pp_ghosts_shallow = m->sharded();   // owned rows only were swept
    int rc = m->sync();
    if (rc) return rc;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
    if (avg_ms_out) *avg_ms_out = ms / n_sweeps;
    return 0;
}

// Timing of the pressure solves inside cfd_update (HIP events on the model's
// stream): enable, run steps, then read the totals.
int cfd_timing_begin(cfd_model *m) {
    if (!m) return fail(CFD_EINVAL, "null model");
    int rc = m->sync();
    if (rc) return rc;
    m->timing = true;
    m->ev_next = 0;
    m->solve_events.clear();
    m->step_events.clear();
    for (auto &pe : m->phase_events) pe.clear();
    m->timed_sweeps = 0;
    m->timed_launches = 0;
    m->timed_steps = 0;
    return 0;
}

int cfd_timing_end(cfd_model *m, double *solve_ms, uint64_t *sweeps, double *step_ms, uint64_t *steps) {
    if (!m) return fail(CFD_EINVAL, "null model");
    int rc = m->sync();
    if (rc) return rc;
    double s_ms = 0.0, t_ms = 0.0;
    for (auto &pr : m->solve_events) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
        s_ms += ms;
    }
    for (size_t k = 0; k + 1 < m->step_events.size(); k += 2) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, m->step_events[k], m->step_events[k + 1]));
        t_ms += ms;
    }
    for (int ph = 0; ph < 3; ++ph) {
        m->phase_ms[ph] = 0.0;
        m->phase_count[ph] = 0;
        for (auto &pr : m->phase_events[ph]) {
            float ms = 0.f;
            if (!pr.second) continue;
            HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
            m->phase_ms[ph] += ms;
            ++m->phase_count[ph];
        }
        m->phase_events[ph].clear();
    }
    if (solve_ms) *solve_ms = s_ms;
    if (sweeps) *sweeps = m->timed_sweeps;
    if (step_ms) *step_ms = t_ms;
    if (steps) *steps = m->timed_steps;
    m->timing = false;
    m->ev_next = 0;
    m->solve_events.clear();
    m->step_events.clear();
    return 0;
}

int cfd_timing_phases(cfd_model *m, int on) {
    if (!m) return fail(CFD_EINVAL, "null model");
    m->timing_phases = on != 0;
    return 0;
}

int cfd_timing_phase_ms(const cfd_model *m, double *predict_ms, double *finish_ms) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (predict_ms) *predict_ms = m->phase_ms[0];
    if (finish_ms) *finish_ms = m->phase_ms[1];
    return 0;
}

int cfd_timing_exchange_ms(const cfd_model *m, double *exchange_ms, uint64_t *exchanges) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (exchange_ms) *exchange_ms = m->phase_ms[2];
    if (exchanges) *exchanges = m->phase_count[2];
    return 0;
}

int cfd_get_halo_depth(const cfd_model *m) { return m ? m->g.hg : 0; }

int cfd_get_kernel_config(const cfd_model *m, int *fastdiv, int *temporal) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (fastdiv) *fastdiv = m->g.fastdiv;
    if (temporal) *temporal = m->spec_mode() ? kMaxTemporal : m->g.tol_enabled ? 1 : m->t_max;
    return 0;
}

int cfd_get_jacobi_kernel(const cfd_model *m, int *kind, char *name, size_t name_len) {
    if (!m) return fail(CFD_EINVAL, "null model");
    const bool spec = m->spec_mode();
    const bool resident = m->resident_mode();
    const int T = spec ? kMaxTemporal : m->g.tol_enabled ? 1 : m->t_max;
    const int k = resident ? 6 : spec ? 5 : T <= 1 ? 0 : m->g.tb_kind;
    if (kind) *kind = k;
    if (name && name_len) {
        char buf[96];
        if (resident)
            snprintf(buf, sizeof buf, "k_jacobi_resident<%d>", m->g.res_div);
        else if (spec)
            snprintf(buf, sizeof buf, "k_jacobi_lds<%d, %d, 2>", T, m->g.fastdiv);
        else if (k == 0)
            snprintf(buf, sizeof buf, "k_jacobi<%d, %d>", kJacRowsPerWave, m->g.fastdiv);
        else if (k == 1)
            snprintf(buf, sizeof buf, "k_jacobi_tb<%d, %d>", T, m->g.fastdiv);
        else if (k == 5)
            snprintf(buf, sizeof buf, "k_jacobi_lds<%d, %d, 0>", T, m->g.fastdiv);
        else
            snprintf(buf, sizeof buf, "k_jacobi_pipe<%d, %d>", T, m->g.fastdiv);
        snprintf(name, name_len, "%s", buf);
    }
    return 0;
}

int cfd_get_jacobi_geometry(const cfd_model *m, int persist, int *lds_pad, int *wgs_per_cu,
                            int *wave_cols, int *segments) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (hipSetDevice(m->device) != hipSuccess) return fail(CFD_EHIP, "hipSetDevice");
    // the rows of the solve's first 8-sweep block (a slab's owned rows plus
    // the ghost rows that block recomputes)
    int T, lo, hi, exch;
    plan_block((int)m->j0, m->g.nyl, m->g.ny, m->sharded() ? m->g.hg : 0, 0, 8,
               std::max(8, m->params.jacobi_iters), &T, &lo, &hi, &exch);
    if (!m->sharded()) lo = 1 - (int)m->j0, hi = (int)m->g.ny - 1 - (int)m->j0;
    int pad = 0, occ = 0, nwc = 0, nseg = 0;
    lds_geometry8(m->g, lo, hi, persist != 0, &pad, &occ, &nwc, &nseg);
    if (lds_pad) *lds_pad = pad;
    if (wgs_per_cu) *wgs_per_cu = occ;
    if (wave_cols) *wave_cols = nwc;
    if (segments) *segments = nseg;
    return 0;
}

int cfd_get_persist_steals(cfd_model *m, uint64_t *steals) {
    if (!m || !steals) return fail(CFD_EINVAL, "null argument");
    int rc = m->sync();
    if (rc) return rc;
    uint32_t v = 0;
    HIP_TRY(hipMemcpy(&v, m->f.persist + 2, 4, hipMemcpyDeviceToHost));
    *steals = v;
    return 0;
}

int cfd_get_persist_sums(cfd_model *m, uint64_t *blocks) {
    if (!m || !blocks) return fail(CFD_EINVAL, "null argument");
    int rc = m->sync();
    if (rc) return rc;
    uint32_t v = 0;
    HIP_TRY(hipMemcpy(&v, m->f.persist + 3, 4, hipMemcpyDeviceToHost));
    *blocks = v;   // persistent blocks run in the SUMS form
    return 0;
}

int cfd_get_sums_launches(cfd_model *m, uint64_t *launches) {
    if (!m || !launches) return fail(CFD_EINVAL, "null argument");
    Ctl c;
    int rc = m->read_ctl(&c);
    if (rc) return rc;
    *launches = c.sums_launches;   // per-launch marches run in the fma form
    return 0;
}

int cfd_get_sums_bounds(cfd_model *m, uint32_t *state, uint32_t *m0_bits, uint32_t *rm_bits) {
    if (!m || !state || !m0_bits || !rm_bits) return fail(CFD_EINVAL, "null argument");
    Ctl c;
    int rc = m->read_ctl(&c);
    if (rc) return rc;
    // the fma form's guard words as the next solve would read them; a model
    // that never keeps them (Fields::sums_track 0) reports zeros
    const bool on = m->f.sums_track != 0;
    *state = on ? c.sums_state : 0u;
    *m0_bits = on ? c.sums_m0 : 0u;
    *rm_bits = on ? c.sums_rm : 0u;
    return 0;
}

int cfd_get_comm_calls(const cfd_model *m, uint64_t *n) {
    if (!m || !n) return fail(CFD_EINVAL, "null argument");
    *n = m->comm_calls;
    return 0;
}

int cfd_get_recoveries(const cfd_model *m, uint64_t *n) {
    if (!m || !n) return fail(CFD_EINVAL, "null argument");
    *n = m->recoveries;
    return 0;
}

int cfd_get_resident_solves(const cfd_model *m, uint64_t *solves) {
    if (!m || !solves) return fail(CFD_EINVAL, "null argument");
    *solves = m->resident_solves;
    return 0;
}

int cfd_get_resident_geometry(const cfd_model *m, int *br, int *bc, int *tiles, int *wgs) {
    if (!m) return fail(CFD_EINVAL, "null model");
    int v[4] = {0, 0, 0, 0};
    if (!m->resident_mode() || !jacobi_resident_geometry(m->g, &v[0], &v[1], &v[2], &v[3]))
        return fail(CFD_ESTATE, "the model does not take the resident solve");
    if (br) *br = v[0];
    if (bc) *bc = v[1];
    if (tiles) *tiles = v[2];
    if (wgs) *wgs = v[3];
    return 0;
}

int cfd_get_persist_blocks(const cfd_model *m, int *blocks) {
    if (!m || !blocks) return fail(CFD_EINVAL, "null argument");
    *blocks = m->last_persist_blocks;
    return 0;
}

// ---- host-only slab plan (no device needed) ----
int cfd_plan_slab(uint64_t ny, int n_ranks, int rank, uint64_t *j0, uint64_t *j1) {
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks || !j0 || !j1)
        return fail(CFD_EINVAL, "bad plan_slab arguments");
    plan_slab(ny, n_ranks, rank, j0, j1);
    return 0;
}

int cfd_plan_sweep(int j0, int nyl, int ny, int halo_depth, int it, int iters, int *lo, int *hi,
                   int *exchange) {
    if (halo_depth < 1 || !lo || !hi || !exchange) return fail(CFD_EINVAL, "bad plan_sweep arguments");
    plan_sweep(j0, nyl, ny, halo_depth, it, iters, lo, hi, exchange);
    return 0;
}

int cfd_plan_block(int j0, int nyl, int ny, int halo_depth, int it, int t_max, int iters, int *T,
                   int *out_lo, int *out_hi, int *exchange) {
    if (t_max < 1 || !T || !out_lo || !out_hi || !exchange)
        return fail(CFD_EINVAL, "bad plan_block arguments");
    plan_block(j0, nyl, ny, halo_depth, it, t_max, iters, T, out_lo, out_hi, exchange);
    return 0;
}

int cfd_plan_overlap(int nyl, int halo_depth, int rank, int n_ranks, int lo, int hi, int *out6) {
    if (!out6 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(CFD_EINVAL, "bad plan_overlap arguments");
    return plan_overlap(nyl, halo_depth, rank, n_ranks, lo, hi, out6);
}

int cfd_plan_halo(int kind, int nyl, int depth, int rank, int n_ranks, int *out6) {
    if (kind < 0 || kind > 2 || !out6) return fail(CFD_EINVAL, "bad plan_halo arguments");
    plan_halo(kind, nyl, depth, rank, n_ranks, out6);
    return 0;
}

void cfd_destroy(cfd_model *m) {
    if (!m) return;
    m->destroy();
    delete m;
}

}  // extern "C"
