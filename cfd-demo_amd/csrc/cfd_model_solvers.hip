// cfd_model_solvers.hip — SOR (red-black and script order) and multigrid
// (the host runtime behind include/cfd.h; see cfd_model.h)
#include <cstring>

#include "cfd_model.h"

using namespace cfd;

// The script's constants for spacing (dx, dy) (index.html:181-183, 1349).
void cfd_model::level_consts(double dx, double dy, double *dx2, double *dy2, double *denom,
                         double *r, int32_t *fast) {
    *dx2 = dx * dx;
    *dy2 = dy * dy;
    *denom = 2.0 / (dx * dx) + 2.0 / (dy * dy);
    r[0] = 1.0 / *dx2;
    r[1] = 1.0 / *dy2;
    r[2] = 1.0 / *denom;
    *fast = exact_pow2(*dx2) && exact_pow2(*dy2) && exact_pow2(*denom) ? 1 : 0;
    if (env_int("CFD_FASTDIV", 1) == 0) *fast = 0;   // read at every call
}

SorConst cfd_model::sor_consts() const {
    SorConst k;
    double r[3];
    level_consts((double)g.dx, (double)g.dy, &k.dx2, &k.dy2, &k.denom, r, &k.fast);
    k.r_dx2 = r[0];
    k.r_dy2 = r[1];
    k.r_denom = r[2];
    return k;
}

// SOR on a slab (k_sor_march over the owned interior rows): each
// iteration reads 2 p' ghost rows per side (the red rows just outside the
// slab are recomputed from them) and 1 rhs ghost row, so the written
// buffer's 2 boundary rows go to the neighbours after every iteration.
// Fixed count: only the last iteration's residual is all-reduced.  With
// the tolerance on (residual_out != null, the host-driven corrector loop)
// every iteration's is, and the host checks them one iteration behind
// the launches, as the sharded Jacobi does (model.rs:816 / index.html:772).
int cfd_model::enqueue_sor_sharded(const SorConst &k, int pass, float *residual_out, hipEvent_t e0) {
    const int iters = params.jacobi_iters;
    const int lo = std::max(0, 1 - (int)j0), hi = std::min(g.nyl, (int)g.ny - 1 - (int)j0);
    if (iters < 1 || g.hg < 2 || !sor_fused_ok(g.nx, hi - lo))
        return fail(CFD_EINVAL, "sharded SOR needs >= 1 iteration, halo depth >= 2 and >= 16 "
                                "interior rows per slab");
    const bool tol = g.tol_enabled != 0;
    float res_local = 0.f;
    if (tol && !residual_out) residual_out = &res_local;
    if (!tol) return enqueue_sor_sharded_deep(k, pass, e0);
    int rc = exchange(FLD_RHS, HALO_PP, 1);
    if (rc) return rc;
    int n = iters, checked = 0;
    bool done = false;
    auto converged = [&](int it, bool *yes) -> int {
        int rc2 = wait_done(ev_res[it % kResRing]);
        if (rc2) return rc2;
        float e;
        std::memcpy(&e, (const void *)&h_res[it % kResRing], 4);
        *yes = e < params.p_tol;
        return 0;
    };
    for (int it = 0; it < iters && !done; ++it) {
        const int res = tol || it == iters - 1;
        launch_sor_fused(f.pp[0], f.pp[1], f.rhs, g.nx, g.ny, k, f.ctl, f.err_slots, pass, it,
                         tol, g.p_tol, res, lo, hi, (int)j0, -g.hg, g.nyl + g.hg - 1, stream);
        if (res) {
            launch_fold_slots(f.ctl->err + it, f.err_slots + (size_t)it * kResSlots * kResStride,
                              1, stream);
            rc = allreduce_max_u32(f.ctl->err + it, 1);
            if (rc) return rc;
        }
        rc = exchange_pp((host_cur + it + 1) & 1, 2);
        if (rc) return rc;
        if (!tol) continue;
        HIP_TRY(hipMemcpyAsync(&h_res[it % kResRing], f.ctl->err + it, 4, hipMemcpyDeviceToHost,
                               stream));
        HIP_TRY(hipEventRecord(ev_res[it % kResRing], stream));
        while (checked <= it - 1 && !done) {
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
    while (tol && !done && checked < iters) {
        bool yes = false;
        rc = converged(checked, &yes);
        if (rc) return rc;
        if (yes) {
            n = checked + 1;
            done = true;
        }
        ++checked;
    }
    end_solve_timing(e0, (uint64_t)n, (uint64_t)n);
    // with the tolerance on the finalize recounts n from the (identical)
    // all-reduced residuals and flips the buffer n times
    launch_finalize_solve(g, f, tol ? -1 : pass, iters, !tol && pass >= 1 ? 1 : 0, iters,
                          stream);
    HIP_TRY(hipGetLastError());
    host_cur = (host_cur + (tol ? n : iters)) & 1;
    pp_ghosts_shallow = true;
    if (tol) {
        float r = 0.f;
        HIP_TRY(hipMemcpyAsync(&r, &f.ctl->last_p, 4, hipMemcpyDeviceToHost, stream));
        rc = wait_done(nullptr);
        if (rc) return rc;
        *residual_out = r;
    }
    return 0;
}

// Fixed-count SOR on a slab with deep ghosts: an iteration's output rows
// [a, b) read p' rows [a-2, b+2) and rhs rows [a-1, b+1), so after an
// exchange of hg p' rows (and hg rhs rows once per solve) the next
// K = hg/2 iterations can each recompute a band of ghost rows two rows
// narrower than the one before, and p' crosses the link once every K
// iterations instead of after every one.  Iteration 0 reads no p' (the
// solve starts from 0).  Every ghost row is computed from the same values
// as its owner computes it, so the result is bitwise the single domain's.
int cfd_model::enqueue_sor_sharded_deep(const SorConst &k, int pass, hipEvent_t e0) {
    const int iters = params.jacobi_iters;
    const int glo = 1 - (int)j0, ghi = (int)g.ny - 1 - (int)j0;   // global rows 1..ny-2
    const int K = std::max(1, g.hg / 2);
    int rc = exchange(FLD_RHS, HALO_PP, g.hg);
    if (rc) return rc;
    for (int it = 0; it < iters; ++it) {
        const int d = it % K;
        const int a = std::max(glo, -g.hg + 2 * (d + 1));
        const int b = std::min(ghi, g.nyl + g.hg - 2 * (d + 1));
        const int res = it == iters - 1;
        launch_sor_fused(f.pp[0], f.pp[1], f.rhs, g.nx, g.ny, k, f.ctl, f.err_slots, pass, it,
                         0, g.p_tol, res, a, b, (int)j0, -g.hg, g.nyl + g.hg - 1, stream);
        if (res) {
            launch_fold_slots(f.ctl->err + it, f.err_slots + (size_t)it * kResSlots * kResStride,
                              1, stream);
            rc = allreduce_max_u32(f.ctl->err + it, 1);
            if (rc) return rc;
        }
        if (d == K - 1 && it + 1 < iters) {
            rc = exchange_pp((host_cur + it + 1) & 1, g.hg);
            if (rc) return rc;
        }
    }
    // the corrector reads p' ghost rows -1 and nyl (the shared v faces):
    // a last iteration that recomputed no ghost row (d == K-1) is
    // followed by a full exchange; otherwise its recomputed band covers
    // both, and only the deeper ghosts are stale
    const bool last_bare = iters > 0 && (iters - 1) % K == K - 1;
    if (last_bare) {
        rc = exchange_pp((host_cur + iters) & 1, g.hg);
        if (rc) return rc;
    }
    end_solve_timing(e0, (uint64_t)iters, (uint64_t)iters);
    launch_finalize_solve(g, f, pass, iters, pass >= 1 ? 1 : 0, iters, stream);
    HIP_TRY(hipGetLastError());
    host_cur = (host_cur + iters) & 1;
    pp_ghosts_shallow = !last_bare;
    return 0;
}

// SOR (index.html:741-774) swept red-black: fused iterations ping-pong
// (opt.sor_fused), else two color passes in place on the current p'.
int cfd_model::enqueue_sor(int pass) {
    const int iters = params.jacobi_iters;
    hipEvent_t e0;
    begin_solve_timing(pass, &e0);
    const SorConst k = sor_consts();
    if (sharded()) return enqueue_sor_sharded(k, pass, nullptr, e0);
    if (iters > 0 && opt.sor_fused && sor_fused_ok(g.nx, g.ny - 2)) {
        // one launch per iteration, ping-pong from the device's current
        // buffer; the finalize flips it once per executed iteration
        for (int it = 0; it < iters; ++it)
            launch_sor_fused(f.pp[0], f.pp[1], f.rhs, g.nx, g.ny, k, f.ctl, f.err_slots, pass,
                             it, g.tol_enabled, g.p_tol, g.tol_enabled || it == iters - 1, 1,
                             g.ny - 1, 0, -g.hg, g.nyl + g.hg - 1, stream);
        end_solve_timing(e0, (uint64_t)iters, (uint64_t)iters);
        launch_finalize_solve(g, f, pass, iters, pass >= 1 ? 1 : 0, iters, stream);
        if (!g.tol_enabled) host_cur = (host_cur + iters) & 1;
        HIP_TRY(hipGetLastError());
        return 0;
    }
    float *pp = f.pp[host_cur];
    launch_fill_zero(pp, (size_t)g.nx * g.ny, f.ctl, pass, stream);
    for (int it = 0; it < iters; ++it) {
        const int res = g.tol_enabled || it == iters - 1;
        for (int color = 0; color < 2; ++color)
            launch_sor_color(pp, f.rhs, g.nx, g.ny, k, color, f.ctl, f.err_slots, pass, it,
                             g.tol_enabled, g.p_tol, res, stream);
    }
    end_solve_timing(e0, (uint64_t)iters, 2 * (uint64_t)iters + 1);
    launch_finalize_solve(g, f, pass, iters, pass >= 1 ? 1 : 0, 0, stream, 1);
    HIP_TRY(hipGetLastError());
    return 0;
}

// SOR in the script's own order (index.html:741-774; cfd_sor_lex.hip):
// one ticketed launch for the whole solve, a replay launch behind it with
// the tolerance on.  The buffers flip once per iteration run, as in the
// fused red-black solve; one domain only (validate_sharded).
int cfd_model::enqueue_sor_lex(int pass) {
    const int iters = params.jacobi_iters;
    if (sharded()) return fail(CFD_EINVAL, "pressure_solver 4 (script-order SOR) runs on one domain only");
    hipEvent_t e0;
    begin_solve_timing(pass, &e0);
    unsigned long long *const r64 = res64_on();
    int launches = 0;
    if (iters < 1) {
        // p' = 0 (index.html:743) in whichever buffer is current
        launch_fill_zero(f.pp[0], (size_t)g.nx * g.ny, f.ctl, pass, stream);
        launch_fill_zero(f.pp[1], (size_t)g.nx * g.ny, f.ctl, pass, stream);
        launches = 2;
    } else {
        const size_t need = sor_lex_words(iters, g.ny);
        if (need > lex_words) {
            if (lex_pol) HIP_TRY(hipFree(lex_pol));   // waits for the device
            lex_pol = nullptr;
            lex_words = 0;
            HIP_TRY(hipMalloc((void **)&lex_pol, need * 4));
            lex_words = need;
        }
        if (!lex_exit) HIP_TRY(hipMalloc((void **)&lex_exit, 16));
        HIP_TRY(launch_sor_lex(f.pp[0], f.pp[1], f.rhs, g.nx, g.ny, sor_consts(), f.ctl, lex_pol,
                               lex_exit, f.host_nonfinite ? f.host_nonfinite + 2 : nullptr, pass,
                               iters, g.tol_enabled, g.p_tol, g.n_cu, &launches, stream, r64));
    }
    end_solve_timing(e0, (uint64_t)iters, (uint64_t)launches);
    launch_finalize_solve(g, f, pass, iters, pass >= 1 ? 1 : 0, iters, stream);
    // every iteration publishes, those that ran past an exit included
    if (r64) launch_publish_f64(f, r64, pass, iters, 0, 0, stream);
    if (!g.tol_enabled) host_cur = (host_cur + iters) & 1;
    HIP_TRY(hipGetLastError());
    return 0;
}

// The script's default solver, Jacobi with omega 0.7 (index.html:796-838;
// cfd_jacobi_script.hip): one launch per iteration, ping-pong from the
// device's current buffer, launches after the early exit predicated on the
// device; the finalize flips the buffer once per iteration run, as in the
// fused red-black solve.  One domain only (validate_sharded).
int cfd_model::enqueue_jacobi_script(int pass) {
    const int iters = params.jacobi_iters;
    if (sharded()) return fail(CFD_EINVAL, "pressure_solver 5 (the script's Jacobi) runs on one domain only");
    hipEvent_t e0;
    begin_solve_timing(pass, &e0);
    int launches = iters;
    if (iters < 1) {
        // p' = 0 (index.html:798) in whichever buffer is current
        launch_fill_zero(f.pp[0], (size_t)g.nx * g.ny, f.ctl, pass, stream);
        launch_fill_zero(f.pp[1], (size_t)g.nx * g.ny, f.ctl, pass, stream);
        launches = 2;
    }
    const SorConst k = sor_consts();
    unsigned long long *const r64 = res64_on();
    for (int it = 0; it < iters; ++it)
        launch_jacobi_script(f.pp[0], f.pp[1], f.rhs, g.nx, g.ny, k, f.ctl, f.err_slots, pass, it,
                             g.tol_enabled, g.p_tol, g.tol_enabled || it == iters - 1, stream, r64);
    end_solve_timing(e0, (uint64_t)iters, (uint64_t)launches);
    launch_finalize_solve(g, f, pass, iters, pass >= 1 ? 1 : 0, iters, stream);
    // with the tolerance on every iteration up to the exit publishes (later
    // launches return first); a fixed count publishes its last iteration only
    if (r64)
        launch_publish_f64(f, r64, pass, iters, g.tol_enabled ? 0 : std::max(iters - 1, 0),
                           g.tol_enabled ? 1 : 0, stream);
    if (!g.tol_enabled) host_cur = (host_cur + iters) & 1;
    HIP_TRY(hipGetLastError());
    return 0;
}

// Level table of mgVcycle's recursion: sizes floor((n+1)/2) down to the
// first level with nx <= 4 or ny <= 4 (index.html:1444-1451), spacing
// doubling per level (:1458).
//
// Sharded models partition the fine levels too (mg_P levels; see
// enqueue_mg_partitioned): level l of rank r owns global rows
// [J0 / 2^l, J1 / 2^l) of its slab [J0, J1) and stores kMgGhost ghost
// rows each side.  A level is partitioned when every rank's boundary is
// divisible by 2^(l+1) (the restriction maps owned rows onto owned rows),
// every slab keeps >= 2 kMgGhost rows there, and the level lies above the
// single-workgroup tail; the coarser levels are gathered whole to every
// rank.  Every level pointer is biased to global row 0.
// owned rows of level l for `rank` (partitioned levels)
void cfd_model::mg_rows(int l, int r, int *j0o, int *j1o) const {
    uint64_t a, b;
    plan_slab(g.ny, n_ranks, r, &a, &b);
    *j0o = (int)(a >> l);
    *j1o = r == n_ranks - 1 ? mg[l].ny : (int)(b >> l);
}
int cfd_model::mg_partition_levels(const std::vector<std::pair<int, int>> &dims, int tail) const {
    if (!sharded() || !opt.mg_partition || !mg_smooth_wave_form()) return 0;
    if (!env_flag("CFD_MG_TB", true)) return 0;
    int P = 0;
    for (int l = 0; l < tail && l + 1 < (int)dims.size(); ++l) {
        bool ok = true;
        for (int r = 0; r < n_ranks && ok; ++r) {
            uint64_t a, b;
            plan_slab(g.ny, n_ranks, r, &a, &b);
            const uint64_t m = 1ull << (l + 1);
            const int j0l = (int)(a >> l);
            const int j1l = r == n_ranks - 1 ? dims[l].second : (int)(b >> l);
            ok = a % m == 0 && j1l - j0l >= 2 * kMgGhost;
        }
        if (!ok) break;
        P = l + 1;
    }
    return P;
}

int cfd_model::mg_build() {
    if (!mg.empty()) return 0;
    std::vector<std::pair<int, int>> dims{{g.nx, g.ny}};
    while (!(dims.back().first <= 4 || dims.back().second <= 4)) {
        if ((int)dims.size() >= kMgMaxLevels) return fail(CFD_EINVAL, "multigrid: too many levels");
        dims.push_back({(dims.back().first + 1) / 2, (dims.back().second + 1) / 2});
    }
    const int nl = (int)dims.size();
    // levels of at most CFD_MG_TAIL cells (default 64 x 64) run inside k_mg_tail
    const long thr = env_long("CFD_MG_TAIL", 4096);
    mg_tail = nl - 1;
    for (int l = 0; l < nl; ++l)
        if ((long)dims[l].first * dims[l].second <= thr) {
            mg_tail = l;
            break;
        }
    mg_P = mg_partition_levels(dims, mg_tail);
    mg.resize(nl);
    for (int l = 0; l < nl; ++l) {
        std::memset(&mg[l], 0, sizeof(MgLevel));
        mg[l].nx = dims[l].first;
        mg[l].ny = dims[l].second;
        mg[l].ys = 0;
        mg[l].ye = mg[l].ny;
        if (l < mg_P) {
            int a, b;
            mg_rows(l, rank, &a, &b);
            mg[l].ys = std::max(0, a - kMgGhost);
            mg[l].ye = std::min(mg[l].ny, b + kMgGhost);
        }
    }
    // level 0: the residual; a sharded model also keeps its own solution
    // buffers and rhs (the gathered whole grid when no level partitions:
    // every rank then solves the whole grid redundantly, see enqueue_mg)
    auto rows_of = [&](int l) { return (size_t)(mg[l].ye - mg[l].ys); };
    size_t total = (sharded() ? 4 : 1) * round4((size_t)g.nx * rows_of(0));
    for (int l = 1; l < nl; ++l) total += 4 * round4((size_t)dims[l].first * rows_of(l));
    HIP_TRY(hipMalloc((void **)&mg_pool, total * 4));
    HIP_TRY(hipMemsetAsync(mg_pool, 0, total * 4, stream));
    float *cur = mg_pool;
    for (int l = 0; l < nl; ++l) {
        MgLevel &L = mg[l];
        const size_t n = (size_t)L.nx * rows_of(l);
        const long bias = (long)L.ys * L.nx;   // pointers address global rows
        auto take = [&]() {
            float *p0 = cur - bias;
            cur += round4(n);
            return p0;
        };
        if (l == 0 && !sharded()) {
            L.rhs = f.rhs;
            L.r = take();
        } else {
            L.a = take();
            L.b = take();
            L.rhs = take();
            L.r = take();
        }
        const double scale = std::ldexp(1.0, l);   // 2*dx per recursion, exact
        double r[3];
        level_consts((double)g.dx * scale, (double)g.dy * scale, &L.dx2, &L.dy2, &L.denom, r,
                     &L.fast);
        L.r_dx2 = r[0];
        L.r_dy2 = r[1];
        L.r_denom = r[2];
        L.lo = L.ys;
        L.hi = L.ye;
    }
    HIP_TRY(hipMalloc((void **)&mg_dev, sizeof(MgLevel) * nl));
    HIP_TRY(hipMemcpy(mg_dev, mg.data(), sizeof(MgLevel) * nl, hipMemcpyHostToDevice));
    return 0;
}

// The multigrid branch (index.html:775-795): p' = 0, 3 V-cycles on the
// current p' buffer, residual max |A p' - rhs| into the solve's slot set.
// Sharded multigrid: the V-cycle's coarse levels shrink below one row per
// slab, so every rank gathers the whole rhs (point-to-point all-gather),
// solves the whole grid redundantly with the single-domain kernels — the
// same arithmetic on the same data, so every rank holds the single-domain
// result bit for bit — and keeps its slab's rows plus hg ghost rows of it.
int cfd_model::gather_rhs() {
    float *full = mg[0].rhs;
    const size_t nx = (size_t)g.nx;
    if (hub) {
        HIP_TRY(hipStreamSynchronize(stream));
        hub->barrier();   // every member's rhs is final
        for (cfd_model *peer : hub->members)
            HIP_TRY(hipMemcpyAsync(full + (size_t)peer->j0 * nx, peer->f.rhs,
                                   (size_t)peer->g.nyl * nx * 4, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        hub->barrier();   // nobody overwrites an rhs a peer is still copying
        return 0;
    }
    if (!comm) return fail(CFD_ERCCL, "the RCCL communicator was aborted after an earlier failure");
    HIP_TRY(hipMemcpyAsync(full + (size_t)j0 * nx, f.rhs, (size_t)g.nyl * nx * 4,
                           hipMemcpyDeviceToDevice, stream));
    RCCL_TRY(ncclGroupStart());
    for (int r = 0; r < n_ranks; ++r) {
        if (r == rank) continue;
        uint64_t a, b;
        plan_slab(g.ny, n_ranks, r, &a, &b);
        RCCL_OP(ncclSend(f.rhs, (size_t)g.nyl * nx, ncclFloat, r, comm, stream));
        RCCL_OP(ncclRecv(full + a * nx, (size_t)(b - a) * nx, ncclFloat, r, comm, stream));
    }
    RCCL_OP(ncclGroupEnd());
    return 0;
}

// ---- multigrid on slabs with partitioned fine levels (mg_P > 0) ----
// Ghost rows of level arrays with both neighbours (which: 0 a, 1 b, 2 rhs):
// rows [J0-d, J0) come from rank-1's owned rows, [J1, J1+d) from rank+1's,
// every item in one RCCL group (LocalHub: device copies from the peers).
static float *mg_arr(const MgLevel &L, int which) {
    return which == 0 ? L.a : which == 1 ? L.b : L.rhs;
}
int cfd_model::mg_exchange(std::initializer_list<MgX> items) {
    if (hub) {
        HIP_TRY(hipStreamSynchronize(stream));
        hub->barrier();   // every member's rows are final
        for (const MgX &x : items) {
            const size_t nx = (size_t)mg[x.l].nx, d = (size_t)x.depth;
            int j0, j1;
            mg_rows(x.l, rank, &j0, &j1);
            float *mine = mg_arr(mg[x.l], x.which);
            if (rank > 0) {
                const float *peer = mg_arr(hub->members[rank - 1]->mg[x.l], x.which);
                HIP_TRY(hipMemcpyAsync(mine + (j0 - (long)d) * nx, peer + (j0 - (long)d) * nx,
                                       d * nx * 4, hipMemcpyDeviceToDevice, stream));
            }
            if (rank < n_ranks - 1) {
                const float *peer = mg_arr(hub->members[rank + 1]->mg[x.l], x.which);
                HIP_TRY(hipMemcpyAsync(mine + (long)j1 * nx, peer + (long)j1 * nx, d * nx * 4,
                                       hipMemcpyDeviceToDevice, stream));
            }
        }
        HIP_TRY(hipStreamSynchronize(stream));
        hub->barrier();   // nobody overwrites rows a peer is still copying
        return 0;
    }
    if (!comm) return fail(CFD_ERCCL, "the RCCL communicator was aborted after an earlier failure");
    RCCL_TRY(ncclGroupStart());
    for (const MgX &x : items) {
        const size_t nx = (size_t)mg[x.l].nx, n = (size_t)x.depth * nx;
        int j0, j1;
        mg_rows(x.l, rank, &j0, &j1);
        float *a = mg_arr(mg[x.l], x.which);
        if (rank > 0) {
            RCCL_OP(ncclSend(a + (long)j0 * nx, n, ncclFloat, rank - 1, comm, stream));
            RCCL_OP(ncclRecv(a + (long)(j0 - x.depth) * nx, n, ncclFloat, rank - 1, comm, stream));
        }
        if (rank < n_ranks - 1) {
            RCCL_OP(ncclSend(a + (long)(j1 - x.depth) * nx, n, ncclFloat, rank + 1, comm, stream));
            RCCL_OP(ncclRecv(a + (long)j1 * nx, n, ncclFloat, rank + 1, comm, stream));
        }
    }
    RCCL_OP(ncclGroupEnd());
    return 0;
}
// every rank's owned rows of the (whole, not partitioned) level l's rhs
int cfd_model::mg_allgather_rhs(int l) {
    const size_t nx = (size_t)mg[l].nx;
    int j0, j1;
    mg_rows(l, rank, &j0, &j1);
    if (hub) {
        HIP_TRY(hipStreamSynchronize(stream));
        hub->barrier();
        for (int r = 0; r < n_ranks; ++r) {
            if (r == rank) continue;
            int a, b;
            mg_rows(l, r, &a, &b);
            HIP_TRY(hipMemcpyAsync(mg[l].rhs + (long)a * nx, hub->members[r]->mg[l].rhs + (long)a * nx,
                                   (size_t)(b - a) * nx * 4, hipMemcpyDeviceToDevice, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));
        hub->barrier();
        return 0;
    }
    if (!comm) return fail(CFD_ERCCL, "the RCCL communicator was aborted after an earlier failure");
    RCCL_TRY(ncclGroupStart());
    for (int r = 0; r < n_ranks; ++r) {
        if (r == rank) continue;
        int a, b;
        mg_rows(l, r, &a, &b);
        RCCL_OP(ncclSend(mg[l].rhs + (long)j0 * nx, (size_t)(j1 - j0) * nx, ncclFloat, r, comm, stream));
        RCCL_OP(ncclRecv(mg[l].rhs + (long)a * nx, (size_t)(b - a) * nx, ncclFloat, r, comm, stream));
    }
    RCCL_OP(ncclGroupEnd());
    return 0;
}

// The V-cycles (index.html:1444-1470) with levels 0..P-1 partitioned:
// down  each rank smooths (5 sweeps) and forms the residual over its rows
//       plus the row below (the restriction reads it), restricts onto its
//       coarse rows and exchanges that level's rhs ghosts; level P is
//       gathered whole (all-gather of the restricted rhs rows);
// coarse levels P..Lc run whole on every rank with the single-domain
//       kernels and the tail (identical arithmetic on identical data);
// up    each rank exchanges its pre-smoothed field's 5 ghost rows (and
//       the coarse correction's 3), prolong-adds and smooths its rows.
// Every level-l row is computed from the same values as in the
// single-domain solve, so the result is bitwise the same; the whole grid
// is touched only on the small gathered levels.
int cfd_model::enqueue_mg_partitioned(int pass, float *residual_out, hipEvent_t e0) {
    const int lc = (int)mg.size() - 1, P = mg_P;
    int J0[kMgMaxLevels + 1], J1[kMgMaxLevels + 1];
    for (int l = 0; l <= P; ++l) mg_rows(l, rank, &J0[l], &J1[l]);
    auto lvl = [&](int l, int lo, int hi) {
        MgLevel L = mg[l];
        L.lo = lo;
        L.hi = hi;
        return L;
    };
    // (the allocation of a level array is rounded up to 4 floats)
    auto zero = [&](const MgLevel &L) {
        launch_fill_zero(L.a + (long)L.ys * L.nx, round4((size_t)(L.ye - L.ys) * L.nx), f.ctl, pass,
                         stream);
    };
    const size_t nx = (size_t)g.nx;
    int launches = 1;
    // level 0: the slab's rhs rows and their ghosts; p' = 0 (index.html:777)
    HIP_TRY(hipMemcpyAsync(mg[0].rhs + (long)J0[0] * nx, f.rhs, (size_t)g.nyl * nx * 4,
                           hipMemcpyDeviceToDevice, stream));
    zero(mg[0]);
    int rc = mg_exchange({{0, 2, kMgGhost}});
    if (rc) return rc;
    for (int cycle = 0; cycle < 3; ++cycle) {
        if (cycle > 0) {   // the last up-leg wrote level 0's rows only
            rc = mg_exchange({{0, 0, kMgGhost}});
            if (rc) return rc;
        }
        for (int l = 0; l < P; ++l) {
            const MgLevel L = lvl(l, std::max(0, J0[l] - 1), J1[l]);
            launch_mg_smooth5_residual(L, L.a, L.b, f.ctl, pass, stream);
            const MgLevel Cl = lvl(l + 1, J0[l + 1], J1[l + 1]);
            if (l + 1 < P) {
                zero(Cl);
                launch_mg_restrict(L, Cl, f.ctl, pass, stream);
                rc = mg_exchange({{l + 1, 2, kMgGhost}});
            } else {
                zero(Cl);
                launch_mg_restrict(L, Cl, f.ctl, pass, stream);
                rc = mg_allgather_rhs(P);
            }
            if (rc) return rc;
            launches += 3;
        }
        for (int l = P; l < mg_tail; ++l) {   // whole levels
            const MgLevel L = mg[l];
            launch_mg_smooth5_residual(L, L.a, L.b, f.ctl, pass, stream);
            launch_mg_restrict(L, mg[l + 1], f.ctl, pass, stream);
            launches += 2;
        }
        launch_mg_tail(mg_dev, mg_tail, lc, mg[mg_tail].a, mg[mg_tail].b, mg[0].fast, f.ctl, pass,
                       stream);
        ++launches;
        for (int l = mg_tail - 1; l >= P; --l) {
            const MgLevel L = mg[l], Cl = mg[l + 1];
            launch_mg_prolong_smooth5(Cl, l + 1 == lc ? Cl.b : Cl.a, L, L.b, L.a, f.ctl, pass, stream);
            ++launches;
        }
        for (int l = P - 1; l >= 0; --l) {
            if (l + 1 < P)
                rc = mg_exchange({{l, 1, kSmT5}, {l + 1, 0, 3}});
            else
                rc = mg_exchange({{l, 1, kSmT5}});
            if (rc) return rc;
            const MgLevel L = lvl(l, J0[l], J1[l]);
            const MgLevel Cl = l + 1 < P ? lvl(l + 1, J0[l + 1], J1[l + 1]) : mg[l + 1];
            launch_mg_prolong_smooth5(Cl, l + 1 == lc ? Cl.b : Cl.a, L, L.b, L.a, f.ctl, pass, stream);
            ++launches;
        }
    }
    // the slab's p' (and, by exchange, its deep ghosts), then the residual
    // max |A p' - rhs| over the slab's interior rows, all-reduced
    HIP_TRY(hipMemcpyAsync(f.pp[host_cur], mg[0].a + (long)J0[0] * nx, (size_t)g.nyl * nx * 4,
                           hipMemcpyDeviceToDevice, stream));
    rc = exchange_pp(host_cur, g.hg);
    if (rc) return rc;
    pp_ghosts_shallow = false;
    const MgLevel L0 = lvl(0, J0[0], J1[0]);
    launch_mg_final_residual(L0, f.pp[host_cur] - (long)J0[0] * nx, f.err_slots, f.ctl, pass, stream);
    launch_fold_slots(f.ctl->err, f.err_slots, 1, stream);
    rc = allreduce_max_u32(f.ctl->err, 1);
    if (rc) return rc;
    end_solve_timing(e0, 1, (uint64_t)launches + 1);
    launch_finalize_solve(g, f, pass, 1, pass >= 1 ? 1 : 0, 0, stream, 1);
    HIP_TRY(hipGetLastError());
    if (residual_out) {
        float r = 0.f;
        HIP_TRY(hipMemcpyAsync(&r, &f.ctl->last_p, 4, hipMemcpyDeviceToHost, stream));
        rc = wait_done(nullptr);
        if (rc) return rc;
        *residual_out = r;
    }
    return 0;
}

int cfd_model::enqueue_mg(int pass, float *residual_out) {
    int rc = mg_build();
    if (rc) return rc;
    hipEvent_t e0;
    begin_solve_timing(pass, &e0);
    if (sharded() && mg_P > 0) return enqueue_mg_partitioned(pass, residual_out, e0);
    if (sharded()) {
        rc = gather_rhs();
        if (rc) return rc;
    }
    const int lc = (int)mg.size() - 1;
    auto lvl = [&](int l) {
        MgLevel L = mg[l];
        if (l == 0 && !sharded()) {
            L.a = f.pp[host_cur];
            L.b = f.pp[host_cur ^ 1];
        }
        return L;
    };
    const MgLevel L0 = lvl(0);
    launch_fill_zero(L0.a, (size_t)g.nx * g.ny, f.ctl, pass, stream);
    // 5 smooths x -> y: one temporally blocked launch, or 5 single sweeps
    // ping-ponging x/y (CFD_MG_TB=0; the result lands in y either way)
    const bool tb = env_flag("CFD_MG_TB", true);
    int launches = 1;
    auto smooth5 = [&](const MgLevel &L, float *x, float *y) {
        if (tb) {
            launch_mg_smooth5(L, x, y, f.ctl, pass, stream);
            launches += 1;
        } else {
            for (int t = 0; t < 5; ++t)
                launch_mg_smooth(L, t & 1 ? y : x, t & 1 ? x : y, f.ctl, pass, stream);
            launches += 5;
        }
    };
    for (int cycle = 0; cycle < 3; ++cycle) {
        for (int l = 0; l < mg_tail; ++l) {   // down: 5 smooths a->b, residual, restrict
            const MgLevel L = lvl(l);
            if (tb && mg_smooth_wave_form()) {
                // the residual is formed by the smoothing launch itself
                launch_mg_smooth5_residual(L, L.a, L.b, f.ctl, pass, stream);
                launches += 1;
            } else {
                smooth5(L, L.a, L.b);
                launch_mg_residual(L, L.b, f.ctl, pass, stream);
                launches += 1;
            }
            launch_mg_restrict(L, lvl(l + 1), f.ctl, pass, stream);
            launches += 1;
        }
        launch_mg_tail(mg_dev, mg_tail, lc, L0.a, L0.b, L0.fast, f.ctl, pass, stream);
        ++launches;
        for (int l = mg_tail - 1; l >= 0; --l) {   // up: prolong-add into b, 5 smooths b->a
            const MgLevel L = lvl(l), Cl = lvl(l + 1);
            const float *e = l + 1 == lc ? Cl.b : Cl.a;
            if (tb && mg_smooth_wave_form()) {
                // the prolong-add happens as the smoothing loads its window
                launch_mg_prolong_smooth5(Cl, e, L, L.b, L.a, f.ctl, pass, stream);
                launches += 1;
                continue;
            }
            launch_mg_prolong_add(Cl, e, L, L.b, f.ctl, pass, stream);
            smooth5(L, L.b, L.a);
            launches += 1;
        }
    }
    unsigned long long *const r64 = res64_on();
    launch_mg_final_residual(L0, L0.a, f.err_slots, f.ctl, pass, stream, r64);
    if (sharded()) {
        // the slab's rows and its hg ghost rows (inside the grid) of the
        // whole-grid solution: the deep ghosts are exact afterwards
        const int lo = std::max(-g.hg, -(int)j0), hi = std::min(g.nyl + g.hg, g.ny - (int)j0);
        HIP_TRY(hipMemcpyAsync(f.pp[host_cur] + (long)lo * g.nx, L0.a + ((long)j0 + lo) * g.nx,
                               (size_t)(hi - lo) * g.nx * 4, hipMemcpyDeviceToDevice, stream));
        pp_ghosts_shallow = false;
    }
    end_solve_timing(e0, 1, (uint64_t)launches + 1);
    launch_finalize_solve(g, f, pass, 1, pass >= 1 ? 1 : 0, 0, stream, 1);
    if (r64) launch_publish_f64(f, r64, pass, 1, 0, 0, stream);
    HIP_TRY(hipGetLastError());
    if (residual_out) {
        float r = 0.f;
        HIP_TRY(hipMemcpyAsync(&r, &f.ctl->last_p, 4, hipMemcpyDeviceToHost, stream));
        rc = wait_done(nullptr);
        if (rc) return rc;
        *residual_out = r;
    }
    return 0;
}

// the double residual's slot sets are zero between solves; a solve that timed
// out may have left some behind
int cfd_model::clear_res64() {
    if (res64) HIP_TRY(hipMemset(res64, 0, kRes64Words * 8));
    return 0;
}
