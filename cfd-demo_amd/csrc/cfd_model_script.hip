// cfd_model_script.hip — the script's time step: one updateSimulation()
// (index.html:261-363) around cfd_script_piso_step's substeps
// (the host runtime behind include/cfd.h; see cfd_model.h)
#include <cstring>

#include "cfd_model.h"

using namespace cfd;

namespace {

constexpr uint64_t kRampUpSteps = 1000;   // rampUpSteps (:162)
constexpr int kMaxSubsteps = 20;          // the cap of :314

inline size_t pad256(size_t n) { return (n + 255) & ~(size_t)255; }

int su_config_check(const cfd_script_config *c) {
    if (!c) return fail(CFD_EINVAL, "null cfd_script_config");
    if (!std::isfinite(c->dt_user) || !(c->dt_user > 0.0))
        return fail(CFD_EINVAL, "dt_user must be finite and positive");
    if (!std::isfinite(c->target_inlet_velocity))
        return fail(CFD_EINVAL, "target_inlet_velocity must be finite");
    return 0;
}

int su_state_check(const cfd_script_state *st) {
    if (!std::isfinite(st->dt) || st->dt < 0.0)
        return fail(CFD_EINVAL, "script state: dt must be finite and >= 0 (0: unset)");
    if (st->substep_count < 1 || st->substep_count > kMaxSubsteps)
        return fail(CFD_EINVAL, "script state: substep_count must be in [1, 20]");
    return 0;
}

// the model-side conditions of the script path, before any state exists
int su_model_check(cfd_model *m) {
    if (!m) return fail(CFD_EINVAL, "null model");
    const cfd_script_step probe = {CFD_SCRIPT_FIRST, CFD_INLET_UNIFORM, 0.0, 1.0};
    return script_check(m, &probe);
}

}  // namespace

int cfd_model::su_alloc() {
    if (su_pool) return 0;
    const size_t nu = ((size_t)g.nx + 1) * g.ny, nv = (size_t)g.nx * ((size_t)g.ny + 1);
    const size_t bu = pad256(nu * 4), bv = pad256(nv * 4), br = pad256((size_t)kScrRedWords * 8);
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipMalloc((void **)&su_pool, 2 * bu + 2 * bv + br));
    HIP_TRY(hipMemset(su_pool, 0, 2 * bu + 2 * bv + br));
    su_uprev = (float *)su_pool;
    su_uold = (float *)(su_pool + bu);
    su_vprev = (float *)(su_pool + 2 * bu);
    su_vold = (float *)(su_pool + 2 * bu + bv);
    su_red = (unsigned long long *)(su_pool + 2 * bu + 2 * bv);
    HIP_TRY(hipHostMalloc((void **)&su_h, (size_t)kScrRedWords * 8));
    return 0;
}

// One updateSimulation(); the caller has checked the model, the config and
// that the path has begun.
int cfd_model::su_update(const cfd_script_config *c, cfd_script_report *out) {
    if (!su_dt_set) {   // `let dt = parseFloat(timeStepInput.value)` (:158)
        su_dt = c->dt_user;
        su_dt_set = true;
    }
    // :277-281, and dt_sub of :282, checked before anything is enqueued
    su_inlet = su_steps < kRampUpSteps
                   ? ((double)su_steps / (double)kRampUpSteps) * c->target_inlet_velocity
                   : c->target_inlet_velocity;
    const int nsub = su_substeps;
    const cfd_script_step s = {c->scheme, c->inlet_profile, su_inlet, su_dt / (double)nsub};
    if (int rc = script_check(this, &s)) return rc;
    HIP_TRY(hipSetDevice(device));
    const long nu = ((long)g.nx + 1) * g.ny, nv = (long)g.nx * ((long)g.ny + 1);
    // the substeps' solves publish the script's double (script_check admits
    // solvers 2, 4 and 5 only): every decision below is then taken from it
    const bool p64 = res64_on() != nullptr;
    // From the begin pass on u and v are no longer the step's start: a failure
    // before the step's end (a solve that timed out, a HIP error) leaves them
    // extrapolated or part-way through the substeps, so the path then refuses
    // to step on until the caller restores a state (su_failed).
    auto enqueue = [&]() -> int {
        HIP_TRY(hipMemsetAsync(su_red, 0, (size_t)kScrRedWords * 8, stream));
        launch_script_begin(f, su_uprev, su_uold, su_vprev, su_vold, nu, nv, su_steps > 0 ? 1 : 0, stream);
        HIP_TRY(hipGetLastError());
        for (int sub = 0; sub < nsub; ++sub) {   // :288-293
            if (int rc = script_substep(&s)) return rc;
            if (p64)
                launch_script_pmax64(f, su_red, stream);
            else
                launch_script_pmax(f, su_red, stream);
            HIP_TRY(hipGetLastError());
        }
        launch_script_end(f, su_uprev, su_uold, su_vprev, su_vold, nu, nv, su_red, stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(su_h, su_red, (size_t)kScrRedWords * 8, hipMemcpyDeviceToHost, stream));
        return sync();   // the step's one synchronisation
    };
    if (int rc = enqueue()) {
        su_failed = true;
        return rc;
    }

    double mx[3];
    for (int q = 0; q < 3; ++q) {
        unsigned long long b = 0;
        for (int k = 0; k < kResSlots; ++k)
            b = std::max(b, su_h[((size_t)q * kResSlots + k) * kScrRedStride]);
        std::memcpy(&mx[q], &b, 8);
    }
    float pmax_f;
    std::memcpy(&pmax_f, &su_h[kScrRedPmax], 4);
    double pmax_d;
    std::memcpy(&pmax_d, &su_h[kScrRedPmax + 1], 8);
    const double res_u = mx[0], res_v = mx[1], max_vel = mx[2], res_p = p64 ? pmax_d : (double)pmax_f;
    if (p64) su_pmax64 = pmax_d;

    ++su_steps;   // :307
    // :310-317
    double error_norm = res_u;   // Math.max of three numbers none of which is NaN
    if (res_v > error_norm) error_norm = res_v;
    if (res_p > error_norm) error_norm = res_p;
    const double tolerance = 1e-3;
    int next = nsub;
    if (error_norm > tolerance) {
        const double factor = error_norm / tolerance;
        const double want = std::ceil((double)nsub * factor);
        next = want < (double)kMaxSubsteps ? (int)want : kMaxSubsteps;   // Math.min(.., 20); Inf too
    } else if (error_norm < tolerance / 10 && nsub > 1) {
        next = std::max((int)std::floor((double)nsub / 2), 1);
    }
    // computeAutomaticTimeStep (:1322-1342)
    double dt_cfl;
    if (max_vel == 0.0) {
        dt_cfl = c->dt_user;
    } else {
        const double dx = (double)g.dx, dy = (double)g.dy;
        dt_cfl = 0.5 * (dx < dy ? dx : dy) / max_vel;
        if (c->dt_user < dt_cfl) dt_cfl = c->dt_user;   // Math.min, neither is NaN
    }
    // :337-350: residualScalingEnabled scales dt_cfl by the pressure residual
    double new_dt = dt_cfl;
    if (sopt.residual_scaling) {
        const double pressure_tol = 1e-3;
        double dt_pressure = dt_cfl;
        if (res_p > pressure_tol) dt_pressure = dt_cfl * (pressure_tol / (res_p + 1e-10));
        new_dt = dt_pressure < dt_cfl ? dt_pressure : dt_cfl;   // Math.min, neither is NaN
    }
    // :352-357
    const double previous = su_dt;
    if (new_dt > previous) {
        const double lim = previous * 1.1;
        if (lim < new_dt) new_dt = lim;
    }
    su_substeps = next;
    su_dt = new_dt;
    if (out) {
        out->step_count = su_steps;
        out->substeps_run = nsub;
        out->substep_count_next = next;
        out->residual_u = res_u;
        out->residual_v = res_v;
        out->residual_p = res_p;
        out->dt_next = new_dt;
        out->inlet_velocity = su_inlet;
    }
    if (!std::isfinite(res_u) || !std::isfinite(res_v) || !std::isfinite(res_p) ||
        !std::isfinite(new_dt) || !(new_dt > 0.0)) {
        su_bad = true;
        return fail(CFD_ENONFINITE, "script update " + std::to_string(su_steps) +
                                        ": a residual or the next dt is not finite and positive; "
                                        "cfd_script_begin or cfd_script_set_state clears it");
    }
    // simulationLoop's tail (:1233-1238)
    if (trc_pool) {
        if (int rc = cfd_tracers_advance(this, new_dt)) return rc;
        if (su_steps % (uint64_t)trc.interval == 0)
            if (int rc = cfd_tracers_inject(this)) return rc;
    }
    return 0;
}

extern "C" {

int cfd_script_set_state(cfd_model *m, const cfd_script_state *st) {
    if (int rc = su_model_check(m)) return rc;
    if (!st) return fail(CFD_EINVAL, "null cfd_script_state");
    if (!m->su_begun) return fail(CFD_ESTATE, "cfd_script_begin has not been called");
    if (int rc = su_state_check(st)) return rc;
    if (int rc = m->sync()) return rc;
    const size_t nu = ((size_t)m->g.nx + 1) * m->g.ny, nv = (size_t)m->g.nx * ((size_t)m->g.ny + 1);
    if (st->u_prev) HIP_TRY(hipMemcpy(m->su_uprev, st->u_prev, nu * 4, hipMemcpyHostToDevice));
    if (st->v_prev) HIP_TRY(hipMemcpy(m->su_vprev, st->v_prev, nv * 4, hipMemcpyHostToDevice));
    m->su_dt = st->dt;
    m->su_dt_set = st->dt > 0.0;
    m->su_substeps = st->substep_count;
    m->su_steps = st->step_count;
    m->su_bad = false;
    m->su_failed = false;
    return 0;
}

int cfd_script_begin(cfd_model *m, const cfd_script_state *st) {
    if (int rc = su_model_check(m)) return rc;
    if (st)
        if (int rc = su_state_check(st)) return rc;
    if (int rc = m->sync()) return rc;
    if (int rc = m->su_alloc()) return rc;
    m->drop_graph();
    // initSimulation (:226-228): uPrev, vPrev = u, v
    const size_t nu = ((size_t)m->g.nx + 1) * m->g.ny, nv = (size_t)m->g.nx * ((size_t)m->g.ny + 1);
    HIP_TRY(hipMemcpy(m->su_uprev, m->f.u, nu * 4, hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(m->su_vprev, m->f.v, nv * 4, hipMemcpyDeviceToDevice));
    m->su_begun = true;
    m->su_bad = false;
    m->su_failed = false;
    m->su_inlet = 0.0;
    if (st) return cfd_script_set_state(m, st);
    m->su_dt = 0.0;
    m->su_dt_set = false;
    m->su_substeps = 5;   // :157
    m->su_steps = 0;
    return 0;
}

int cfd_script_get_state(cfd_model *m, cfd_script_state *st) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (!st) return fail(CFD_EINVAL, "null cfd_script_state");
    if (!m->su_begun) return fail(CFD_ESTATE, "cfd_script_begin has not been called");
    if (int rc = m->sync()) return rc;
    const size_t nu = ((size_t)m->g.nx + 1) * m->g.ny, nv = (size_t)m->g.nx * ((size_t)m->g.ny + 1);
    if (st->u_prev) HIP_TRY(hipMemcpy(st->u_prev, m->su_uprev, nu * 4, hipMemcpyDeviceToHost));
    if (st->v_prev) HIP_TRY(hipMemcpy(st->v_prev, m->su_vprev, nv * 4, hipMemcpyDeviceToHost));
    st->dt = m->su_dt_set ? m->su_dt : 0.0;
    st->substep_count = m->su_substeps;
    st->step_count = m->su_steps;
    return 0;
}

int cfd_script_update_n(cfd_model *m, const cfd_script_config *c, int n, cfd_script_report *out_n) {
    if (!m) return fail(CFD_EINVAL, "null model");
    if (int rc = su_config_check(c)) return rc;
    if (n < 1) return fail(CFD_EINVAL, "n must be >= 1");
    {
        const cfd_script_step probe = {c->scheme, c->inlet_profile, 0.0, 1.0};
        if (int rc = script_check(m, &probe)) return rc;
    }
    if (!m->su_begun) return fail(CFD_ESTATE, "cfd_script_begin has not been called");
    if (m->su_bad)
        return fail(CFD_ENONFINITE, "an earlier script update left a non-finite residual or dt; "
                                    "cfd_script_begin or cfd_script_set_state clears it");
    if (m->su_failed)
        return fail(CFD_ESTATE, "an earlier script update failed part-way: u and v are not a step's "
                                "start; restore them (cfd_set_state) and call cfd_script_begin or "
                                "cfd_script_set_state");
    for (int k = 0; k < n; ++k)
        if (int rc = m->su_update(c, out_n ? out_n + k : nullptr)) return rc;
    return 0;
}

int cfd_script_update(cfd_model *m, const cfd_script_config *c, cfd_script_report *out) {
    return cfd_script_update_n(m, c, 1, out);
}

}  // extern "C"
