// cfd_model_jacobi.hip — the Jacobi pressure solve: single domain, slabs, speculative blocks
// (the host runtime behind include/cfd.h; see cfd_model.h)
#include <cstring>

#include "cfd_model.h"

using namespace cfd;

PersistGate &cfd::persist_gate(int device) {
    static PersistGate gates[64];
    return gates[device & 63];
}

// Speculative temporal blocking for the tolerance mode (single domain,
// Jacobi, kind-5 kernels at any field size); CFD_SPEC=0
// keeps one launch per sweep with the per-sweep early exit.
bool cfd_model::spec_mode() const {
    return opt.spec && !sharded() && g.tol_enabled &&
           params.pressure_solver == CFD_SOLVER_JACOBI;
}

// The tolerance-mode solve of a small grid as ONE resident launch
// (k_jacobi_resident, cfd_jacobi_resident.hip): CFD_RESIDENT=1 on any
// grid, 0 never; default on up to kResidentAutoCells cells, where the
// per-launch row march is latency-bound.  Off after a timeout.
bool cfd_model::resident_mode() const {
    if (opt.resident == 0 || resident_off || !spec_mode()) return false;
    if (opt.resident < 0 && (long)g.nx * g.ny > kResidentAutoCells) return false;
    int br, bc, nt, wg;
    if (!jacobi_resident_geometry(g, &br, &bc, &nt, &wg)) return false;
    // by default one tile per workgroup (C2's 1024^2 needs 2-3 per
    // workgroup and ran 3.65 -> 7.07 ms per step resident,
    // profiles/r4/ab_c2_r4j.log)
    return opt.resident > 0 || nt <= wg;
}

// r5: the tolerance-mode Jacobi solve on slabs as speculative T-sweep
// blocks (enqueue_solve): per block one T-row p' exchange, one speculative
// launch publishing every sweep's residual, one all-reduce of the block's
// T residuals and the device-side check -- instead of a launch, a fold,
// an all-reduce, an exchange and a host read per sweep.  The default
// since r6 (the host-side stop below): the default_grid() channel on 2
// RCCL ranks (loopback) 102.3 -> 33.5 ms per step, 2,102 -> 569
// collective calls (profiles/r6/prof_r6e/tolbench_*.log), bitwise;
// CFD_SPEC_SLABS=0 keeps the host-driven per-sweep loop.
bool cfd_model::spec_slab_ok() const {
    // (k_spec_align moves float4s from pp + hg * nx: 16-B aligned rows)
    return sharded() && opt.spec && opt.spec_slabs && params.pressure_solver == CFD_SOLVER_JACOBI &&
           g.hg >= 2 && g.nyl >= 2 * kMaxTemporal && ((size_t)g.nyl * g.nx) % 4 == 0 &&
           ((size_t)g.hg * g.nx) % 4 == 0;
}

bool cfd_model::host_driven() const { return sharded() && params.tol_enabled && !spec_slab_ok(); }

// Wait for the device's last persistent or resident launch of this process:
// after another model's stream ran it, `stream` waits for everything that
// stream has enqueued so far (a stream orders its own launches).  The
// resident solve waits always (all its workgroups must be resident at once);
// the persistent launch only under CFD_PERSIST_GATE=1 -- off by default
// since r4: the ticketed launch completes beside any other kernel
// (k_jacobi_persist), so the gate is no longer needed for correctness.
// The caller holds gate.mu, and keeps it until it has written gate.last.
int cfd_model::gate_wait(PersistGate &gate, bool always) {
    if (!(always || opt.persist_gate) || !gate.last || gate.last == stream) return 0;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(gate.last, &cs);
    if (cs == hipStreamCaptureStatusNone) {
        if (!gate.ev) HIP_TRY(hipEventCreateWithFlags(&gate.ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(gate.ev, gate.last));
        HIP_TRY(hipStreamWaitEvent(stream, gate.ev, 0));
    }
    return 0;
}

// Persistent fixed-count solve (k_jacobi_persist); CFD_PERSIST=0 opts out
// everywhere.  Single domain: opt-in (CFD_PERSIST=1) since r4 -- the
// per-launch march with the guarded SUMS form is faster there (profiles/r4).
// Slabs: the blocks between two p' exchanges as one persistent launch,
// opt-in (CFD_PERSIST_SHARDED=1).  r5 same-geometry A/B (the rank slabs'
// owned rows + 2 x 32 ghost rows, the 24 KiB pad they get; medians of 3,
// profiles/r5/prof_r5b/slab_*.log): per launch 5.08 / 5.30 / 5.18 us per
// sweep against persistent 5.42 / 5.72 / 5.44 on the 4096^2, 8192 x 2112
// and 16384 x 1088 shapes, so every slab of the weak-scaling series runs
// one launch per 8-sweep block between its exchanges.
//
// nblk >= 2 eight-sweep blocks on rows [lo, hi) in one persistent launch
// (k_jacobi_persist); *done = false when it does not apply.
int cfd_model::launch_persist(int pass, int par0, int nblk, int lo, int hi, int res_it, bool *done) {
    *done = false;
    if (nblk < 2 || !persist_on || capturing || g.tb_kind != 5) return 0;
    if (persist_epoch + 1 >= (1u << (32 - kPersistBlockBits))) {
        // epochs wrap: clear the flags (stream-ordered) and restart
        HIP_TRY(hipMemsetAsync(f.persist, 0, kPersistWords * 4, stream));
        persist_epoch = 0;
    }
    PersistGate &gate = persist_gate(device);
    std::lock_guard<std::mutex> lk(gate.mu);
    if (int rc = gate_wait(gate, false)) return rc;
    if (!launch_jacobi_persist(g, f, pass, par0, nblk, lo, hi, persist_epoch + 1, res_it, stream))
        return 0;
    last_abort_resident = false;
    gate.last = stream;
    ++persist_epoch;
    *done = true;
    return 0;
}

int cfd_model::enqueue_solve(int pass) {
    // solvers 2, 4 and 5 publish the script's double when the option is on
    p64_valid = res64_on() && (params.pressure_solver == CFD_SOLVER_MULTIGRID ||
                               params.pressure_solver == CFD_SOLVER_SOR_LEX ||
                               params.pressure_solver == CFD_SOLVER_JACOBI_SCRIPT);
    if (params.pressure_solver == CFD_SOLVER_SOR) return enqueue_sor(pass);
    if (params.pressure_solver == CFD_SOLVER_MULTIGRID) return enqueue_mg(pass);
    if (params.pressure_solver == CFD_SOLVER_SOR_LEX) return enqueue_sor_lex(pass);
    if (params.pressure_solver == CFD_SOLVER_JACOBI_SCRIPT) return enqueue_jacobi_script(pass);
    if (!sharded()) return enqueue_jacobi_single(pass);
    if (g.tol_enabled && spec_slab_ok()) return enqueue_spec_slabs(pass);
    return enqueue_jacobi_slabs(pass);
}

// One domain: over global rows 1..=ny-2 as one resident launch, speculative
// blocks (both: the tolerance mode), one launch per sweep, or temporally
// blocked launches behind an optional persistent lead-in.  The solve's timed
// span ends before the finalize (sweeps only).
int cfd_model::enqueue_jacobi_single(int pass) {
    const int iters = params.jacobi_iters;
    const int lo_g = 1 - (int)j0, hi_g = (int)g.ny - 1 - (int)j0;   // global rows 1..ny-2
    hipEvent_t e0;
    begin_solve_timing(pass, &e0);
    const bool spec = spec_mode();
    const int tmax = g.tol_enabled ? 1 : t_max;
    int launches = 0;   // buffers flip once per launch
    bool resident = false;   // the resident launch also finalizes the solve
    // (never under hipGraph capture: its workgroups must be resident
    // at once, and the device gate orders only eager launches)
    if (spec && resident_mode() && !capturing) {
        // the whole solve in one launch, the early exit decided on the
        // device; in-process resident / persistent launches of
        // different models on one device are ordered (all its
        // workgroups must be resident at once)
        PersistGate &gate = persist_gate(device);
        std::lock_guard<std::mutex> lk(gate.mu);
        if (int rc = gate_wait(gate, true)) return rc;
        resident = launch_jacobi_resident(g, f, pass, iters, 1, pass >= 1 ? 1 : 0, stream);
        if (resident) {
            ++resident_solves;
            last_abort_resident = true;
            gate.last = stream;
            // launches the per-launch path would count (host_cur is
            // not tracked with the tolerance on; Ctl::spec_launches is)
            for (int it = 0; it < iters;) {
                int T, lo, hi, exch;
                plan_block((int)j0, g.nyl, g.ny, 0, it, kMaxTemporal, iters, &T, &lo, &hi, &exch);
                it += T;
                ++launches;
            }
        }
    }
    if (resident) {
    } else if (spec) {
        // the tolerance mode, temporally blocked (speculative): each
        // launch runs kSpecT sweeps with every sweep's residual, a check
        // finds the reference's early exit (model.rs:816), and the
        // converged launch is re-run with exactly its sweeps
        // the check (r6 default, spec_lag_first): each launch checks
        // the previous one and the re-run checks the last;
        // CFD_SPEC_LAG=0: a one-workgroup k_spec_check launch after
        // every launch
        const bool lag = opt.spec_lag;
        int prev_T = 0, last_it = 0;
        for (int it = 0; it < iters;) {
            int T, lo, hi, exch;
            plan_block((int)j0, g.nyl, g.ny, 0, it, kMaxTemporal, iters, &T, &lo, &hi, &exch);
            launch_jacobi_spec(g, f, pass, it, launches, T, lo, hi, stream, lag ? prev_T : 0);
            if (!lag) launch_spec_check(g, f, pass, it, T, launches, stream);
            prev_T = T;
            last_it = it;
            it += T;
            ++launches;
        }
        if (iters > 0)
            launch_jacobi_redo(g, f, pass, lo_g, hi_g, stream, last_it, launches - 1,
                               lag ? prev_T : 0);
    } else if (tmax <= 1) {
        for (int it = 0; it < iters; ++it)
            launch_jacobi_sweep(g, f, pass, it, lo_g, hi_g,
                                g.tol_enabled || it == iters - 1, stream);
        launches = iters;
    } else {
        int it = 0;
        last_persist_blocks = 0;
        if (persist_on && opt.persist > 0 && !capturing && tmax == 8 && g.tb_kind == 5) {
            // the leading run of full 8-sweep blocks as one persistent
            // launch, the solve's last block (which publishes the
            // residual) included when it is a full block too
            int nblk = 0, res_it = -1;
            for (int k = 0; k < iters;) {
                int T, lo, hi, exch;
                plan_block((int)j0, g.nyl, g.ny, 0, k, tmax, iters, &T, &lo, &hi, &exch);
                if (T != 8) break;
                if (k + T >= iters) res_it = iters - 1;
                k += T;
                ++nblk;
            }
            bool done = false;
            int rc = launch_persist(pass, launches, nblk, lo_g, hi_g, res_it, &done);
            if (rc) return rc;
            if (done) {
                last_persist_blocks = nblk;
                it = 8 * nblk;
                launches = nblk;
            }
        }
        for (; it < iters;) {
            int T, lo, hi, exch;
            plan_block((int)j0, g.nyl, g.ny, 0, it, tmax, iters, &T, &lo, &hi, &exch);
            launch_jacobi_block(g, f, pass, it, launches, T, lo, hi, it + T == iters,
                                stream);
            it += T;
            ++launches;
        }
    }
    end_solve_timing(e0, (uint64_t)iters, (uint64_t)launches);   // sweeps only
    // (k_jacobi_resident's last workgroup finalized the solve)
    if (!resident)
        launch_finalize_solve(g, f, pass, iters, pass >= 1 ? 1 : 0, launches, stream, spec ? 2 : 0);
    HIP_TRY(hipGetLastError());
    host_cur = (host_cur + launches) & 1;
    return 0;
}

// Slabs with a fixed count: halo depth hg, p' exchanged every hg sweeps;
// between exchanges each launch also recomputes a shrinking band of ghost
// rows, so results equal the single-domain sweep bit for bit.  The solve's
// timed span covers the sweeps, the halo rounds and the residual all-reduce.
int cfd_model::enqueue_jacobi_slabs(int pass) {
    const int iters = params.jacobi_iters;
    hipEvent_t e0;
    begin_solve_timing(pass, &e0);
    const int tmax = g.tol_enabled ? 1 : t_max;
    int launches = 0;   // buffers flip once per launch
    // the deep-halo sweeps recompute ghost rows, which read rhs there.
    // Overlapped (r2): the rhs exchange runs on cstream while the first
    // launch's interior rows, whose T sweeps read no rhs ghost row
    // (the march for output rows [a, b) loads rhs rows [a-T, b+T)),
    // run on stream; the edge rows follow once the ghosts are in.
    last_persist_blocks = 0;
    const bool rhs_ovl = overlap && tmax > 1 && !pp_ghosts_shallow && iters > 0;
    bool rhs_pending = false;
    // whatever path leaves this block, stream waits for the rhs exchange
    // on cstream (so a sync of stream also covers that RCCL group)
    struct JoinRhs {
        cfd_model *m;
        bool *pending;
        ~JoinRhs() {
            if (*pending) (void)hipStreamWaitEvent(m->stream, m->ev_rhs, 0);
        }
    } join_rhs{this, &rhs_pending};
    int rc0;
    if (rhs_ovl) {
        HIP_TRY(hipEventRecord(ev_ov0, stream));   // rhs written
        HIP_TRY(hipStreamWaitEvent(cstream, ev_ov0, 0));
        rc0 = exchange(FLD_RHS, HALO_PP, g.hg, cstream);
        if (rc0) return rc0;
        HIP_TRY(hipEventRecord(ev_rhs, cstream));
        rhs_pending = true;
    } else {
        rc0 = exchange(FLD_RHS, HALO_PP, g.hg);
        if (rc0) return rc0;
    }
    if (pp_ghosts_shallow) {   // sweep 0 reads p' ghosts hg rows deep
        rc0 = exchange_pp(host_cur, g.hg);
        if (rc0) return rc0;
        pp_ghosts_shallow = false;
    }
    for (int it = 0; it < iters;) {
        int T, lo, hi, exch;
        plan_block(g.j0, g.nyl, g.ny, g.hg, it, tmax, iters, &T, &lo, &hi, &exch);
        const int res = it + T == iters;
        if (rhs_pending) {
            rhs_pending = false;
            // the kernel's march loads rhs rows [a-T, b+T) (prefetch
            // included), so no loaded row is an exchanged ghost row
            const int a = std::max(lo, T), b = std::min(hi, g.nyl - T);
            const bool split = a < b && !exch;
            if (split) launch_jacobi_block(g, f, pass, it, launches, T, a, b, res, stream);
            HIP_TRY(hipStreamWaitEvent(stream, ev_rhs, 0));
            if (split) {
                if (lo < a) launch_jacobi_block(g, f, pass, it, launches, T, lo, a, res, stream);
                if (b < hi) launch_jacobi_block(g, f, pass, it, launches, T, b, hi, res, stream);
                it += T;
                ++launches;
                continue;
            }
        }
        // Overlap: the block before an exchange first
        // computes the hg-row bands the exchange sends, on cstream, which
        // then runs the exchange, while the interior rows run on stream.
        // Ghost rows need no compute here: the exchange replaces them.
        int ov[6];
        const bool ovl = overlap && exch && tmax > 1 &&
                         plan_overlap(g.nyl, g.hg, rank, n_ranks, lo, hi, ov);
        if (ovl) {
            HIP_TRY(hipEventRecord(ev_ov0, stream));
            HIP_TRY(hipStreamWaitEvent(cstream, ev_ov0, 0));
            for (int b = 0; b < 2; ++b)   // empty bands launch nothing
                launch_jacobi_block(g, f, pass, it, launches, T, ov[2 * b], ov[2 * b + 1], res,
                                    cstream);
            launch_jacobi_block(g, f, pass, it, launches, T, ov[4], ov[5], res, stream);
            int rc = exchange_pp((host_cur + launches + 1) & 1, g.hg, cstream);
            if (rc) return rc;
            HIP_TRY(hipEventRecord(ev_ov1, cstream));
            HIP_TRY(hipStreamWaitEvent(stream, ev_ov1, 0));
        } else if (tmax == 1) {
            launch_jacobi_sweep(g, f, pass, it, lo, hi, res, stream);
        } else {
            // a run of 8-sweep blocks between two exchanges as one
            // persistent launch over the first block's rows: later
            // blocks recompute ghost rows past their valid band too,
            // which only feed ghost rows and are replaced by the next
            // exchange (owned rows stay inside every block's band)
            int nrun = 0;
            if (T == 8 && tmax == 8 && !exch && !res && opt.persist_sharded)
                for (int k = it; k < iters;) {
                    int T2, lo2, hi2, ex2;
                    plan_block(g.j0, g.nyl, g.ny, g.hg, k, tmax, iters, &T2, &lo2, &hi2, &ex2);
                    if (T2 != 8 || ex2 || k + T2 == iters) break;
                    k += T2;
                    ++nrun;
                }
            bool done = false;
            if (nrun >= 2) {
                int rc = launch_persist(pass, launches, nrun, lo, hi, -1, &done);
                if (rc) return rc;
            }
            if (done) {
                it += 8 * nrun;
                launches += nrun;
                last_persist_blocks += nrun;
                continue;
            }
            launch_jacobi_block(g, f, pass, it, launches, T, lo, hi, res, stream);
        }
        it += T;
        ++launches;
        if (exch && !ovl) {
            int rc = exchange_pp((host_cur + launches) & 1, g.hg);
            if (rc) return rc;
        }
    }
    const int last = iters > 0 ? iters - 1 : 0;
    if (!merge_res_allreduce) {
        launch_fold_slots(f.ctl->err + last,
                          f.err_slots + (size_t)last * kResSlots * kResStride, 1, stream);
        int rc = allreduce_max_u32(f.ctl->err + last, 1);
        if (rc) return rc;
    }
    end_solve_timing(e0, (uint64_t)iters, (uint64_t)launches);   // sweeps + halo rounds
    launch_finalize_solve(g, f, pass, iters, pass >= 1 ? 1 : 0, launches, stream, 0);
    HIP_TRY(hipGetLastError());
    host_cur = (host_cur + launches) & 1;
    return 0;
}

// Sharded with the tolerance on: the reference's early exit (model.rs:816)
// needs the all-reduced residual of every sweep.  Sweep k's residual is
// copied to a pinned host word behind its all-reduce; the host enqueues
// sweep k+1 (kernel, residual fold, all-reduce, 1-row p' exchange) BEFORE
// it waits for sweep k's word, so the GPU and the xGMI link never idle on
// the host's decision (one-sweep-lagged convergence).  When sweep k has
// converged, sweep k+1 is already queued: its kernel reads sweep k's
// all-reduced residual on the device and returns without writing
// (k_jacobi's early exit), so p' and the sweep count are the reference's;
// only its all-reduce and exchange of an untouched buffer run in vain.
int cfd_model::enqueue_solve_host_driven(float *residual_out) {
    if (params.pressure_solver == CFD_SOLVER_SOR) {
        hipEvent_t e0;
        begin_solve_timing(-1, &e0);
        return enqueue_sor_sharded(sor_consts(), -1, residual_out, e0);
    }
    if (params.pressure_solver == CFD_SOLVER_MULTIGRID) {
        float r = 0.f;
        return enqueue_mg(-1, residual_out ? residual_out : &r);
    }
    const int iters = params.jacobi_iters;
    const int lo = std::max(0, 1 - (int)j0), hi = std::min(g.nyl, (int)g.ny - 1 - (int)j0);
    constexpr int kLag = 1;
    static_assert(kLag < kResRing, "lag ring");
    int n = iters;   // sweeps the reference executes
    auto converged = [&](int k, bool *yes) -> int {
        int rc = wait_done(ev_res[k % kResRing]);
        if (rc) return rc;
        float e;
        std::memcpy(&e, (const void *)&h_res[k % kResRing], 4);
        *yes = e < params.p_tol;
        return 0;
    };
    int checked = 0;   // sweeps whose residual the host has read
    bool done = false;
    for (int it = 0; it < iters && !done; ++it) {
        launch_jacobi_sweep(g, f, -1, it, lo, hi, 1, stream);
        launch_fold_slots(f.ctl->err + it, f.err_slots + (size_t)it * kResSlots * kResStride, 1,
                          stream);
        int rc = allreduce_max_u32(f.ctl->err + it, 1);
        if (rc) return rc;
        rc = exchange_pp((host_cur + it + 1) & 1, 1);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(&h_res[it % kResRing], f.ctl->err + it, 4, hipMemcpyDeviceToHost,
                               stream));
        HIP_TRY(hipEventRecord(ev_res[it % kResRing], stream));
        while (checked <= it - kLag && !done) {
            bool yes = false;
            rc = converged(checked, &yes);
            if (rc) return rc;
            if (yes) {
                n = checked + 1;
                done = true;
            }
            ++checked;
        }
    }
    while (!done && checked < iters) {
        bool yes = false;
        int rc = converged(checked, &yes);
        if (rc) return rc;
        if (yes) {
            n = checked + 1;
            done = true;
        }
        ++checked;
    }
    if (iters == 0) n = 0;
    // the device finalize recomputes n from the (identical) all-reduced slots
    launch_finalize_solve(g, f, -1, iters, 0, n, stream);
    HIP_TRY(hipGetLastError());
    host_cur = (host_cur + n) & 1;
    pp_ghosts_shallow = true;
    float res = 0.f;
    HIP_TRY(hipMemcpyAsync(&res, &f.ctl->last_p, 4, hipMemcpyDeviceToHost, stream));
    int rc = wait_done(nullptr);
    if (rc) return rc;
    if (residual_out) *residual_out = res;
    return 0;
}

// r6: the host's view of the speculative blocks.  After its all-reduce a
// block's T residuals -- the same values on every rank -- are copied to
// pinned host words; the host reads block 0 at once (from rest a solve
// usually ends in its first sweeps) and every later block one block
// behind, and enqueues no block (and, in enqueue_piso, no corrector pass)
// past the one where the solve has ended.  Every rank reads the same
// values, so every rank stops at the same block and the collective
// sequences stay matched; the device's own check (k_spec_check, the
// go flags) stays authoritative for the bits.  So a solve's collectives
// track its convergence (r5 enqueued all blocks of all 20 passes:
// 1,014 calls against the host-driven loop's 30, GPUTEST_r05).
int cfd_model::enqueue_spec_slabs(int pass) {
    const int iters = params.jacobi_iters;
    hipEvent_t e0;
    begin_solve_timing(pass, &e0);
    const int Tm = std::min(kMaxTemporal, g.hg);
    const int lo = std::max(0, 1 - (int)j0), hi = std::min(g.nyl, (int)g.ny - 1 - (int)j0);
    const int nb = iters > 0 ? (iters + Tm - 1) / Tm : 0;
    int it = 0, launches = 0, checked = 0, rc = 0;
    int blk_T[kSpecRing] = {};
    bool stop = false;
    // reads block `checked`'s all-reduced residuals (waits for them)
    auto check_next = [&]() -> int {
        const int slot = checked % kSpecRing;
        int rc2 = wait_done(ev_spec[slot]);
        if (rc2) return rc2;
        for (int k = 0; k < blk_T[slot] && !stop; ++k) {
            float e;
            std::memcpy(&e, (const void *)&h_spec[slot * kMaxTemporal + k], 4);
            stop = e < params.p_tol;   // model.rs:816 (NaN: no exit)
        }
        ++checked;
        return 0;
    };
    for (int b = 0; b < nb && !stop; ++b) {
        const int T = iters / nb + (b < iters % nb ? 1 : 0);   // even split, no short tail
        // the block's source, T rows deep; every block reads rhs rows T
        // deep into the ghosts: the first block's exchange carries them
        rc = b == 0 ? exchange_rhs_pp(g.hg, (host_cur + launches) & 1, T)
                    : exchange_pp((host_cur + launches) & 1, T);
        if (rc) return rc;
        launch_jacobi_spec(g, f, pass, it, launches, T, lo, hi, stream);
        launch_fold_slots(f.ctl->err + it, f.err_slots + (size_t)it * kResSlots * kResStride, T,
                          stream);
        rc = allreduce_max_u32(f.ctl->err + it, (size_t)T);   // every rank decides alike
        if (rc) return rc;
        launch_spec_check(g, f, pass, it, T, launches, stream);
        const int slot = b % kSpecRing;
        HIP_TRY(hipMemcpyAsync(&h_spec[slot * kMaxTemporal], f.ctl->err + it, 4 * (size_t)T,
                               hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(ev_spec[slot], stream));
        blk_T[slot] = T;
        it += T;
        ++launches;
        while (!stop && checked <= (b == 0 ? 0 : b - 1)) {
            rc = check_next();
            if (rc) return rc;
        }
    }
    // the pass loop's break (pass >= 1 with a pass after it) needs the
    // solve's outcome: the last blocks too
    const bool need = pass >= 1 && pass < params.corrector_passes;
    while (need && !stop && checked < launches) {
        rc = check_next();
        if (rc) return rc;
    }
    spec_converged = stop;
    if (iters > 0) {
        launch_jacobi_redo(g, f, pass, lo, hi, stream);
        launch_spec_align(g, f, pass, launches, stream);
        // the corrector reads one p' ghost row of the result (the re-run
        // and the alignment wrote owned rows only)
        rc = exchange_pp((host_cur + launches) & 1, 1);
        if (rc) return rc;
    }
    end_solve_timing(e0, (uint64_t)iters, (uint64_t)launches);
    launch_finalize_solve(g, f, pass, iters, pass >= 1 ? 1 : 0, launches, stream, 3);
    HIP_TRY(hipGetLastError());
    host_cur = (host_cur + launches) & 1;
    pp_ghosts_shallow = true;   // the converged block's re-run: ghosts stale
    return 0;
}
