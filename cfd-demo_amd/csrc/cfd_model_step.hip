// cfd_model_step.hip — piso_step, Model::update, graph capture, synchronisation, checkpoint
// (the host runtime behind include/cfd.h; see cfd_model.h)
#include <cstddef>

#include "cfd_model.h"

using namespace cfd;

namespace {
const float kNaN = std::nanf("");
}  // namespace

hipEvent_t cfd_model::take_event() {
    if (ev_next == ev_pool.size()) {
        hipEvent_t e;
        (void)hipEventCreate(&e);
        ev_pool.push_back(e);
    }
    return ev_pool[ev_next++];
}

hipEvent_t cfd_model::phase_mark(int ph, bool end, hipStream_t st) {
    if (!(timing && timing_phases)) return nullptr;
    hipEvent_t e = take_event();
    (void)hipEventRecord(e, st ? st : stream);
    if (end) phase_events[ph].back().second = e;
    else phase_events[ph].emplace_back(e, nullptr);
    return e;
}

void cfd_model::begin_solve_timing(int pass, hipEvent_t *e0) {
    *e0 = nullptr;
    if (timing && pass <= 0) {
        *e0 = take_event();
        (void)hipEventRecord(*e0, stream);
    }
}
void cfd_model::end_solve_timing(hipEvent_t e0, uint64_t sweeps, uint64_t launches) {
    if (!e0) return;
    hipEvent_t e1 = take_event();
    (void)hipEventRecord(e1, stream);
    solve_events.emplace_back(e0, e1);
    timed_sweeps += sweeps;
    timed_launches += launches;
}

// u* <- u, v* <- v and the divergence at the head of a corrector pass
// (model.rs:698-704): one fused launch (CFD_COPY_DIV=0: the two launches)
void cfd_model::pass_head(int pass, float dt_override) {
    if (opt.copy_div) {
        launch_copy_star_div(g, f, pass, dt_override, stream);
    } else {
        launch_copy_star(g, f, pass, stream);
        launch_divergence(g, f, pass, dt_override, stream);
    }
}

// The uv-fused step applies: one domain, a Jacobi solve, the predictor march.
// By default only where it was measured against the step it replaces (DESIGN
// §5 r11): the first-order scheme on a grid whose march has at least 4
// workgroups per CU (4096^2: 8.5).  The second-order finish (4-row segments,
// two waves per SIMD) and small grids, where the march's few fat workgroups
// replace k_correct_finish4m's one-row bands, run it only with CFD_UV_FUSED=1.
bool cfd_model::uv_fused_ok() const {
    if (opt.uv_fused == 0 || sharded() || host_driven() ||
        params.pressure_solver != CFD_SOLVER_JACOBI || !predict_march_ok(g, f))
        return false;
    if (opt.uv_fused != kEnvUnset) return true;
    return g.scheme == 0 && predict_march_workgroups(g) >= 4 * g.n_cu;
}
void cfd_model::swap_uv() {
    std::swap(f.u, f.u_old);
    std::swap(f.v, f.v_old);
    std::swap(f.u_alloc_base, f.u_old_base);
    std::swap(f.v_alloc_base, f.v_old_base);
    uv_flip ^= 1;
}
// u*, v* of the last uv-fused step, which stored none: the storing march over
// that step's old u, v (f.u_old / f.v_old since the swap) with its dt
// (Ctl::star_dt) -- the values the step formed in registers, bit for bit.
// Called before anything outside a uv-fused step reads or writes u*, v*.
int cfd_model::need_star() {
    if (!star_lazy) return 0;
    HIP_TRY(hipSetDevice(device));
    Fields fm = f;
    fm.u = f.u_old;
    fm.v = f.v_old;
    fm.u_alloc_base = f.u_old_base;
    fm.v_alloc_base = f.v_old_base;
    fm.sums_track = 0;
    launch_predict_march(g, fm, kNaN, stream, false, 0, -1, 0, true);
    HIP_TRY(hipGetLastError());
    star_lazy = false;
    return 0;
}

// piso_step (model.rs:529-730).
// finish = inside update() with no extra corrector passes: the corrector,
// the boundaries and the step reductions run as one fused pass.
int cfd_model::enqueue_piso(float dt_override, bool finish) {
    // K1-K3: the fused march when it applies, else predictors + divergence
    const bool march = predict_march_ok(g, f);
    // the fixed-count step that keeps u*, v* out of memory: the march stores
    // rhs only, and the finish forms u*, v* again from the old u, v it reads
    // anyway and stores the new u, v into the other pair of arrays
    const bool uvf = finish && uv_fused_ok();
    if (!uvf)
        if (int rc = need_star()) return rc;
    phase_mark(0, false);
    if (uvf) {
        launch_predict_march(g, f, dt_override, stream, step_begin_folded, 0, -1, 1);
        phase_mark(0, true);
        if (int rc = enqueue_solve(0)) return rc;
        phase_mark(1, false);
        launch_predict_march(g, f, dt_override, stream, false, 0, -1, 2);
        phase_mark(1, true);
        HIP_TRY(hipGetLastError());
        swap_uv();
        star_lazy = true;
        return 0;
    }
    if (march && finish && uv_async) {
        // rows [2, nyl-2) read u rows >= 0 and <= nyl-1 and v rows <= nyl;
        // the edge rows (4-row launches overlapping the interior ones:
        // identical values) follow the ghost exchange
        launch_predict_march(g, f, dt_override, stream, true, 2, g.nyl - 2);
        HIP_TRY(hipStreamWaitEvent(stream, ev_uv, 0));
        launch_predict_march(g, f, dt_override, stream, false, 0, 4);
        launch_predict_march(g, f, dt_override, stream, false, g.nyl - 4, g.nyl);
    } else if (march)
        launch_predict_march(g, f, dt_override, stream, finish && step_begin_folded);
    else
        launch_predict(g, f, dt_override, opt.pred_vec, stream);
    auto first_divergence = [&](int pass) {
        if (!march) launch_divergence(g, f, pass, dt_override, stream);
        phase_mark(0, true);
    };
    if (finish) {
        first_divergence(host_driven() ? -1 : 0);
        // a fixed-count step on slabs needs the solve's residual only for
        // reporting: it rides the step-end all-reduce (Ctl::red[5]) instead
        // of an all-reduce of its own
        merge_res_allreduce = sharded() && !host_driven();
        int rc = host_driven() ? enqueue_solve_host_driven(nullptr) : enqueue_solve(0);
        merge_res_allreduce = false;
        if (rc) return rc;
        phase_mark(1, false);
        launch_correct_finish(g, f, dt_override, stream);
        phase_mark(1, true);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    if (!host_driven()) {
        first_divergence(0);
        int rc = enqueue_solve(0);
        if (rc) return rc;
        // single domain: each corrector that a further pass follows also
        // does that pass's head, as the device's go flag decides
        // (k_correct_head4; every pass, the last included, runs it: the
        // passes alternate the u* / v* arrays)
        const int passes = params.corrector_passes;
        const bool fuse = !sharded() && passes >= 1 && opt.corr_head && correct_head_ok(g, f);
        auto corrector = [&](int pass) {
            if (fuse)
                launch_correct_head(g, f, pass, dt_override, pass < passes, stream);
            else
                launch_corrector(g, f, pass, dt_override, opt.corr_vec, stream);
        };
        corrector(0);
        const bool spec_slabs = sharded() && g.tol_enabled && spec_slab_ok();
        for (int pass = 1; pass <= passes; ++pass) {
            if (!fuse) pass_head(pass, dt_override);
            rc = enqueue_solve(pass);
            if (rc) return rc;
            corrector(pass);
            // slabs: the host knows where the loop ends (enqueue_spec_slabs)
            // and enqueues no pass the device would skip (model.rs:721-723)
            if (spec_slabs && spec_converged) break;
        }
    } else {
        first_divergence(-1);
        float res = 0.f;
        int rc = enqueue_solve_host_driven(&res);
        if (rc) return rc;
        launch_corrector(g, f, -1, dt_override, opt.corr_vec, stream);
        for (int pass = 1; pass <= params.corrector_passes; ++pass) {
            pass_head(-1, dt_override);
            rc = enqueue_solve_host_driven(&res);
            if (rc) return rc;
            launch_corrector(g, f, -1, dt_override, opt.corr_vec, stream);
            if (res < params.p_tol) break;
        }
    }
    launch_boundary(g, f, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Model::update (model.rs:304-379).
// rec_step: record the step's GPU time for cfd_get_residuals (the last
// step of a cfd_update_n batch only: every event record on the stream
// costs the step a few microseconds of dispatch)
int cfd_model::enqueue_update(bool rec_step) {
    if (rec_step) HIP_TRY(hipEventRecord(ev_step0, stream));
    const bool fused = params.corrector_passes == 0;
    // one launch less where the predictor march can carry the work: it
    // sets the inlet ramp (all k_step_begin does when nothing is copied)
    step_begin_folded = fused && predict_march_ok(g, f);
    if (!step_begin_folded) launch_step_begin(g, f, fused ? 0 : 1, stream);
    // slabs: the u/v ghost exchange runs on cstream while the predictor
    // march forms the rows that read no ghost (enqueue_piso)
    uv_async = sharded() && overlap && fused && step_begin_folded && g.nyl >= 8;
    int rc;
    if (uv_async) {
        HIP_TRY(hipEventRecord(ev_ov0, stream));   // u, v final (last step's finish)
        HIP_TRY(hipStreamWaitEvent(cstream, ev_ov0, 0));
        rc = exchange_uv(cstream);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(ev_uv, cstream));
    } else {
        rc = exchange_uv();
    }
    if (rc) return rc;
    rc = enqueue_piso(kNaN, fused);
    if (rc) return rc;
    if (!fused) launch_step_reduce(g, f, stream);
    // a step with corrector passes ends in k_correct_head4, which publishes
    // no max |p'|: bound the p' the next step's first solve starts from
    if (!fused && f.sums_track) launch_publish_sums_m0(g, f, stream);
    if (sharded()) launch_fold_slots(f.ctl->red, f.red_slots, 4, stream);
    // slabs with persistent runs: a rank whose persistent solve timed out
    // tells every rank through the step all-reduce (red[6])
    if (sharded() && persist_on && opt.persist_sharded) launch_abort_to_red(f, stream);
    rc = allreduce_max_u32(f.ctl->red, 7);   // maxima, non-finite flag, solve residual, abort
    if (rc) return rc;
    launch_step_finalize(g, f, stream);
    // updateTracers(dt) with the dt and step count the finalize has just
    // written, then the injection (index.html:1231-1238)
    if (trc_pool) launch_trc_step(g, f, trc, trc_grid, true, 0.0, stream);
    HIP_TRY(hipGetLastError());
    if (rec_step) HIP_TRY(hipEventRecord(ev_step1, stream));
    if (timing) timed_steps++;
    if (rec_step) stepped = true;   // ev_step0 / ev_step1 hold a step
    return 0;
}

// ------------------------------------------------------------ hipGraph
// The launch sequence of a step is the same every step for an unsharded
// Jacobi model: every data-dependent choice (buffers, early exits, pass
// gating, dt) is read from Ctl on the device, so kernel arguments never
// change.  cfd_update_n then captures graph_steps steps once and replays
// the instantiated graph.  Dropped when the parameters
// change; not used while solve timing is on (its events are per solve).
// Opt-in (CFD_GRAPH=1): measured 1.2486 vs 1.2507 ms per step at 4096^2
// (r2, tools/graph_ab.py) — the inter-kernel gaps are not launch overhead.
bool cfd_model::graph_ok() const {
    return opt.graph && !sharded() && !timing && !trc_pool &&
           params.pressure_solver == CFD_SOLVER_JACOBI;
}
void cfd_model::drop_graph() {
    if (step_graph) (void)hipGraphExecDestroy(step_graph);
    step_graph = nullptr;
}
int cfd_model::update_graph(int n) {
    if (!step_graph) {
        const int hc0 = host_cur, fl0 = uv_flip;
        const bool sl0 = star_lazy;
        HIP_TRY(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
        int rc = 0;
        capturing = true;
        for (int k = 0; k < graph_steps && !rc; ++k) rc = enqueue_update(false);
        capturing = false;
        hipGraph_t graph = nullptr;
        const hipError_t ce = hipStreamEndCapture(stream, &graph);
        if (rc || ce != hipSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            host_cur = hc0;
            if (uv_flip != fl0) swap_uv();
            star_lazy = sl0;
            return rc ? rc : fail(CFD_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
        }
        const hipError_t ie = hipGraphInstantiate(&step_graph, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ie != hipSuccess) {
            step_graph = nullptr;
            host_cur = hc0;
            if (uv_flip != fl0) swap_uv();
            star_lazy = sl0;
            return fail(CFD_EHIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
        }
        graph_cur_delta = (host_cur - hc0) & 1;
        host_cur = hc0;   // captured, not executed
        // the captured kernels hold the u / v pairs as they were at the
        // capture's first step: a replay starts from that arrangement
        graph_uv_flip = fl0;
        graph_uv_delta = uv_flip ^ fl0;
        if (uv_flip != fl0) swap_uv();
        star_lazy = sl0;
    }
    int k = 0;
    if (uv_flip != graph_uv_flip && n > 1) {   // a plain step brings the pairs back
        int rc = enqueue_update(false);
        if (rc) return rc;
        k = 1;
    }
    for (; uv_flip == graph_uv_flip && k + graph_steps <= n - 1; k += graph_steps) {
        HIP_TRY(hipGraphLaunch(step_graph, stream));       // the last step stays out: it records the step time
        host_cur = (host_cur + graph_cur_delta) & 1;
        if (graph_uv_delta) swap_uv();
        if (uv_fused_ok() && params.corrector_passes == 0) star_lazy = true;
    }
    for (; k < n; ++k) {
        int rc = enqueue_update(k == n - 1);
        if (rc) return rc;
    }
    return 0;
}

// Slabs with persistent runs, entry points outside Model::update
// (cfd_piso_step, cfd_pressure_solve): a rank whose persistent solve timed
// out tells every rank through an all-reduce of the abort word, so every
// rank recovers at its next synchronisation and replays the same calls
// (inside a step the step all-reduce carries it, enqueue_update)
int cfd_model::abort_allreduce() {
    if (!(sharded() && persist_on && opt.persist_sharded)) return 0;
    launch_abort_to_red(f, stream);
    int rc = allreduce_max_u32(f.ctl->red + 6, 1);
    if (rc) return rc;
    launch_abort_from_red(f, stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int cfd_model::sync() {
    HIP_TRY(hipSetDevice(device));
    int rc = wait_done(nullptr);
    if (rc) return rc;
    rc = persist_timeout_check(true);
    if (rc) return rc;
    ck_commit();   // everything enqueued so far is final: no replay needed
    return 0;
}
// A persistent (k_jacobi_persist) or resident (k_jacobi_resident) solve
// that gave up waiting left an invalid p' and every step after it
// computed from it.  r5: the model recovers by itself -- it restores the
// checkpoint it took before the first entry since its last
// synchronisation (ck_begin) and re-runs those entries with one launch
// per block -- and reports the fault once (CFD_ETIMEOUT; the state is
// valid when it returns).  Solves run per launch from then on.
// at_sync: the stream has drained (slabs detect only there, so every rank
// re-runs the same entries)
int cfd_model::persist_timeout_check(bool at_sync) {
    if (!h_nonfinite || !*(volatile uint32_t *)(h_nonfinite + 2)) return 0;
    if (!at_sync && sharded()) return 0;
    if (params.pressure_solver == CFD_SOLVER_SOR_LEX) {
        // no checkpoint is kept for this solver: p' is invalid until cfd_set_state
        HIP_TRY(hipStreamSynchronize(stream));
        *(volatile uint32_t *)(h_nonfinite + 2) = 0u;
        clear_abort_words();
        clear_res64();
        return fail(CFD_ETIMEOUT, "script-order SOR solve timed out waiting for a workgroup; "
                                  "its result is invalid until cfd_set_state");
    }
    const char *which = last_abort_resident ? "resident tolerance-mode" : "persistent";
    HIP_TRY(hipStreamSynchronize(stream));
    if (cstream) HIP_TRY(hipStreamSynchronize(cstream));
    *(volatile uint32_t *)(h_nonfinite + 2) = 0u;
    persist_on = false;
    resident_off = true;
    if (ck_open) {
        const size_t n_entries = ck_replay.size();
        int rc = recover();
        if (rc) return rc;
        return fail(CFD_ETIMEOUT, std::string(which) + " Jacobi solve timed out waiting for a "
                                  "workgroup; recovered: the state was restored from the "
                                  "model's checkpoint and " + std::to_string(n_entries) +
                                  " call(s) re-run with one launch per block (the state is "
                                  "valid); per-launch solves from now on");
    }
    clear_abort_words();
    return fail(CFD_ETIMEOUT, std::string(which) + " Jacobi solve timed out waiting for a "
                              "workgroup (no checkpoint was open); its result is invalid; "
                              "per-launch solves from now on");
}

// ---- self-recovery checkpoint (r5) ---------------------------------
// Taken (stream-ordered device copies) at the first cfd_update_n /
// cfd_pressure_solve / cfd_piso_step after a synchronisation, when the
// model may run a persistent or resident solve; the entries enqueued
// since are kept as replays.  A synchronisation that finds no fault
// commits (drops) them.
bool cfd_model::ckpt_needed() const {
    if (!opt.ckpt || params.pressure_solver != CFD_SOLVER_JACOBI) return false;
    if (persist_on && (sharded() ? opt.persist_sharded : opt.persist > 0)) return true;
    return resident_mode();
}
int cfd_model::ck_begin() {
    if (ck_open || !ckpt_needed()) return 0;
    if (!ck_pool) {
        size_t tot = 0;
        for (const CkSeg &sg : ck_segs) tot += (sg.bytes + 255) & ~(size_t)255;
        HIP_TRY(hipMalloc((void **)&ck_pool, tot));
        ck_bytes = tot;
    }
    size_t off = 0;
    for (const CkSeg &sg : ck_segs) {
        HIP_TRY(hipMemcpyAsync(ck_pool + off, sg.ptr, sg.bytes, hipMemcpyDeviceToDevice, stream));
        off += (sg.bytes + 255) & ~(size_t)255;
    }
    ck_host_cur = host_cur;
    ck_shallow = pp_ghosts_shallow;
    ck_uv_flip = uv_flip;
    ck_star_lazy = star_lazy;
    ck_replay.clear();
    ck_open = true;
    return 0;
}
void cfd_model::ck_record(std::function<int()> fn) {
    if (ck_open) ck_replay.push_back(std::move(fn));
}
void cfd_model::ck_commit() {
    ck_open = false;
    ck_replay.clear();
}
// The fma form's maxima (Ctl::sums_state) describe the p' and rhs of
// "finish of step n-1, then predictor march of step n": every entry point
// that can change either outside that sequence drops them first.
int cfd_model::invalidate_sums() {
    HIP_TRY(hipMemsetAsync(&ctl->sums_state, 0, 4, stream));
    return 0;
}
// the abort word and the resident solve's barrier lines (its counters,
// generations and exit ticket stay where an aborted launch left them)
int cfd_model::clear_abort_words() {
    HIP_TRY(hipMemset(f.persist, 0, (size_t)kPersistHeadLines * kPersistFlagStride * 4));
    return 0;
}
int cfd_model::recover() {
    size_t off = 0;
    for (const CkSeg &sg : ck_segs) {
        HIP_TRY(hipMemcpy(sg.ptr, ck_pool + off, sg.bytes, hipMemcpyDeviceToDevice));
        off += (sg.bytes + 255) & ~(size_t)255;
    }
    // residual slot sets are zero between solves; an aborted solve may
    // have left some behind
    HIP_TRY(hipMemset(f.err_slots, 0, (size_t)kMaxSweeps * kResSlots * kResStride * 4));
    int rc = clear_abort_words();
    if (rc) return rc;
    rc = clear_res64();
    if (rc) return rc;
    *(volatile uint32_t *)h_nonfinite = 0u;
    host_cur = ck_host_cur;
    pp_ghosts_shallow = ck_shallow;
    if (uv_flip != ck_uv_flip) swap_uv();
    star_lazy = ck_star_lazy;
    ++recoveries;
    std::vector<std::function<int()>> replay;
    replay.swap(ck_replay);
    ck_open = false;
    const bool tm = timing;
    timing = false;   // the re-run is not a measurement
    for (auto &fn : replay) {
        rc = fn();
        if (rc) break;
    }
    timing = tm;
    if (rc) return rc;
    rc = wait_done(nullptr);
    if (rc) return rc;
    if (*(volatile uint32_t *)(h_nonfinite + 2))   // per-launch solves cannot time out
        return fail(CFD_ETIMEOUT, "the re-run after a solve timeout timed out");
    return 0;
}

// the checkpoint pool is sized for its segments when ck_begin allocates it:
// whoever changes ck_segs (after a sync(): no checkpoint is open) drops it
int cfd_model::ck_drop_pool() {
    if (ck_pool) HIP_TRY(hipFree(ck_pool));
    ck_pool = nullptr;
    ck_bytes = 0;
    return 0;
}

int cfd_model::read_ctl(Ctl *out) {
    int rc = sync();
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out, f.ctl, offsetof(Ctl, go), hipMemcpyDeviceToHost));
    return 0;
}
