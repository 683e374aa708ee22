// cfd_model.h — the host runtime behind include/cfd.h.
//
// One cfd_model owns one slab of the grid on one GPU: its HBM fields, a HIP
// stream, the device control block (cfd::Ctl) and, for sharded models, an RCCL
// communicator with the two neighbouring ranks.  Model::update
// (the reference's src/model.rs:304-379) becomes a fixed sequence of kernel
// launches on that stream; the data-dependent control flow of the reference
// (Jacobi early exit :816, corrector-loop break :721, CFL dt :368-377) is
// decided on the device from Ctl, so a step is enqueued without any host
// round trip.
//
// The methods live in one unit per subsystem (no unit holds a kernel; every
// launch goes through the launch_* functions of cfd_internal.h):
//   cfd_model_comm.hip     halo exchanges, all-reduce, RCCL deadlines, LocalHub
//   cfd_model_jacobi.hip   the Jacobi solve: single domain, slabs, speculative
//   cfd_model_solvers.hip  SOR (red-black, script order), the script's Jacobi and multigrid
//   cfd_model_step.hip     piso_step, update, graph capture, sync, checkpoint
//   cfd_model_build.hip    options, validation, creation, destruction
//   cfd_model_extras.hip   tracer particles and the script's substep
//   cfd_model_script.hip   the script's time step (updateSimulation) around that substep
//   cfd_model_abi.hip      the remaining extern "C" surface
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <climits>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/cfd.h"
#include "cfd_internal.h"
#include "slab_plan.h"

namespace cfd {

// Sets the calling thread's cfd_last_error() message and returns `code`
// (cfd_model_abi.hip owns the one thread-local string).
int fail(int code, const std::string &msg);

// The one way the host runtime reads its environment: NAME unset gives `def`.
inline int env_int(const char *name, int def) {
    const char *e = getenv(name);
    return e ? atoi(e) : def;
}
inline long env_long(const char *name, long def) {
    const char *e = getenv(name);
    return e ? atol(e) : def;
}
inline bool env_flag(const char *name, bool def) {
    const char *e = getenv(name);
    return e ? atoi(e) != 0 : def;
}
inline double env_double(const char *name, double def) {
    const char *e = getenv(name);
    return e ? atof(e) : def;
}
constexpr int kEnvUnset = INT_MIN;   // default of the options that have no value of their own

// Spacings that are exact powers of two: division == reciprocal multiply.
inline bool exact_pow2(double c) {
    int e;
    return c > 0.0 && std::isfinite(c) && std::frexp(c, &e) == 0.5 && std::isnormal(1.0 / c);
}

inline size_t round4(size_t n) { return (n + 3) & ~size_t(3); }

}  // namespace cfd

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t e_ = (expr);                                                            \
        if (e_ != hipSuccess)                                                              \
            return cfd::fail(CFD_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

#define RCCL_TRY(expr)                                                                     \
    do {                                                                                   \
        ncclResult_t r_ = (expr);                                                          \
        if (r_ != ncclSuccess)                                                             \
            return cfd::fail(CFD_ERCCL, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
    } while (0)

// An operation on the model's communicator.  Should a call return
// ncclInProgress (a non-blocking communicator), settle() waits, under the
// RCCL deadline, until the communicator's state leaves ncclInProgress.
#define RCCL_OP(expr)                                                                      \
    do {                                                                                   \
        int rc_ = settle((expr), #expr);                                                   \
        if (rc_) return rc_;                                                               \
    } while (0)

// In-process stand-in for the RCCL communicator (testing only): n slabs in
// one process, each driven by its own host thread, possibly all on one GPU.
// Halo exchanges become device-to-device copies between the members' buffers
// and the max all-reduce a host fold, each fenced by host barriers.  Every
// kernel and every row range the sharded path launches is unchanged, so a
// 1-GPU box can check the whole decomposition against the single-domain
// oracle (tests/test_gpu_sharded.py).
struct LocalHub {
    int n = 0;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    std::vector<cfd_model *> members;
    void barrier() {
        std::unique_lock<std::mutex> lk(mu);
        const uint64_t my = gen;
        if (++arrived == n) {
            arrived = 0;
            ++gen;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != my; });
        }
    }
};

// Fields that travel between slabs.
enum FieldId { FLD_U = 0, FLD_V, FLD_PP0, FLD_PP1, FLD_RHS };

// One per device: the last persistent or resident Jacobi launch of this
// process on it (cfd_model::gate_wait).
struct PersistGate {
    std::mutex mu;
    hipEvent_t ev = nullptr;
    hipStream_t last = nullptr;   // the stream of the device's last such launch
};

// Every CFD_* switch that is fixed for a model's life, parsed once per model
// by read_options() when the model is created (never a process-wide static:
// one process creates models under different environments).  Read later, each
// at its own point, and so not here: CFD_FASTDIV in level_consts,
// CFD_MG_TB / CFD_MG_TAIL (mg_build, enqueue_mg), CFD_HALO_DEPTH
// (create_model), CFD_TRACER_WGS (cfd_tracers_enable) and CFD_JACOBI_SUMS
// (set_sums_track); INTEGRATION.md lists them all.
struct cfd_options {
    bool sor_fused = true;         // CFD_SOR_FUSED (1): one k_sor_march launch per red-black iteration; 0: two color passes
    bool mg_partition = true;      // CFD_MG_PARTITION (1): slabs partition the fine multigrid levels
    bool spec = true;              // CFD_SPEC (1): speculative temporal blocks in the tolerance mode; 0: a launch per sweep
    bool spec_lag = true;          // CFD_SPEC_LAG (1): each speculative launch checks the one before; 0: a k_spec_check launch each
    bool spec_slabs = true;        // CFD_SPEC_SLABS (1): the speculative blocks on slabs; 0: the host-driven per-sweep loop
    int persist = -1;              // CFD_PERSIST (unset -1): 0 never persistent, > 0 also on a single domain
    bool persist_sharded = false;  // CFD_PERSIST_SHARDED (0): slabs run the blocks between two exchanges as one persistent launch
    bool persist_gate = false;     // CFD_PERSIST_GATE (0): serialize persistent launches of different models on one device
    int resident = -1;             // CFD_RESIDENT (unset -1: up to kResidentAutoCells cells): 1 on any grid, 0 never
    bool copy_div = true;          // CFD_COPY_DIV (1): a pass head's copy and divergence as one launch; 0: two
    bool pred_vec = true;          // CFD_PRED_VEC (1): the separate first-order predictors' four-column form; 0: one face per thread
    bool corr_vec = true;          // CFD_CORR_VEC (1): the corrector's four-cell form; 0: one float per thread
    bool corr_head = true;         // CFD_CORR_HEAD (1): a pass's corrector and the next pass's head as one launch; 0: separate
    bool graph = false;            // CFD_GRAPH (0): cfd_update_n replays a captured hipGraph of graph_steps steps
    bool ckpt = true;              // CFD_CKPT (1): self-recovery checkpoint; 0: a solve timeout invalidates the state
    int fastdiv = cfd::kEnvUnset;       // CFD_FASTDIV (unset: cheapest proven form): 0 IEEE division, 2 prefer the FMA-corrected form
    int uv_fused = cfd::kEnvUnset;      // CFD_UV_FUSED (unset: first order on a grid that fills the chip): the fixed-count step on one domain keeps u*, v* out of memory (uv_fused_ok); 1 wherever it applies, 0 never
    int resident_div = cfd::kEnvUnset;  // CFD_RESIDENT_DIV (unset): 3 lets the resident solve take the guarded FMA form
    int pred_div = cfd::kEnvUnset;      // CFD_PRED_DIV (unset: 2): 0 IEEE division in the predictors
    int tb_kind = cfd::kEnvUnset;       // CFD_TB_KIND (unset: 5 with the exact reciprocal, else 4): 1, 4 or 5
    int temporal = cfd::kEnvUnset;      // CFD_TEMPORAL (unset: 8 for kind 5, else 4 or 8): sweeps per blocked launch
    int tb_rows = cfd::kEnvUnset;       // CFD_TB_ROWS (unset: 24, kind 5: 0 = sized to the resident waves): rows per wave segment
    int tb_bpc = cfd::kEnvUnset;        // CFD_TB_BPC (unset: 3): balanced segmentation, blocks per CU
    int xcd_remap = cfd::kEnvUnset;     // CFD_XCD_REMAP (unset: 1): 0 keeps the hardware's workgroup-to-XCD order
    double rccl_timeout_s = 300.0; // CFD_RCCL_TIMEOUT_S (300, at least 1): deadline of every RCCL wait
};

struct cfd_model {
    // ------------------------------------------------------------ identity
    int device = 0;
    cfd_grid grid{};
    cfd_params params{};
    cfd_options opt{};
    cfd::Geom g{};
    cfd::Fields f{};

    // ------------------------------------------------- streams and events
    hipStream_t stream = nullptr;
    // sharded fixed-count solves: the boundary bands and their p' exchange run
    // on cstream while the interior runs on stream (SURVEY.md §8(e) overlap)
    hipStream_t cstream = nullptr;
    hipEvent_t ev_ov0 = nullptr, ev_ov1 = nullptr, ev_rhs = nullptr, ev_uv = nullptr;
    static constexpr bool overlap = true;

    // -------------------------------------------------------- allocations
    float *u_all = nullptr, *v_all = nullptr, *uo_all = nullptr, *vo_all = nullptr;
    float *us_all = nullptr, *vs_all = nullptr;
    float *p = nullptr, *rhs = nullptr, *pp_all[2] = {nullptr, nullptr};
    uint8_t *mask_u = nullptr, *mask_v = nullptr;
    int32_t *obs = nullptr;
    cfd::Ctl *ctl = nullptr;
    uint32_t *slots = nullptr;   // spread residual maxima (cfd_internal.h kResSlots)
    float *vis_buf = nullptr;    // render output (nx*nyl words), allocated on first use
    uint32_t *h_nonfinite = nullptr;   // pinned host word the device sets (Fields::host_nonfinite)
    std::vector<uint8_t> h_mask_u, h_mask_v;
    std::vector<uint8_t> dmask_u, dmask_v;   // staging for the async mask upload

    // ---------------------------------------- sharding (cfd_model_comm.hip)
    int n_ranks = 1, rank = 0;
    uint64_t j0 = 0, j1 = 0;
    ncclComm_t comm = nullptr;
    LocalHub *hub = nullptr;   // testing stand-in for comm
    bool comm_aborted = false;
    uint64_t comm_calls = 0;   // halo groups + all-reduces enqueued (cfd_get_comm_calls)
    // p' ghost rows deeper than 1 are stale (a host-driven tolerance solve or
    // cfd_profile_sweeps refreshed only one row per sweep): the next deep-halo
    // fixed-count solve re-exchanges hg rows before its first sweep
    bool pp_ghosts_shallow = false;

    // ----------------------------- the Jacobi solve (cfd_model_jacobi.hip)
    int host_cur = 0;   // mirror of ctl->cur, valid when the tolerance is off
    int t_max = cfd::kMaxTemporal;   // sweeps per temporally blocked launch (CFD_TEMPORAL)
    // sharded tolerance mode: per-sweep residuals copied to pinned host words,
    // each with its completion event (kLag ring, see enqueue_solve_host_driven)
    static constexpr int kResRing = 8;
    uint32_t *h_res = nullptr;
    hipEvent_t ev_res[kResRing] = {};
    // the speculative slab solve's residual blocks (enqueue_spec_slabs)
    static constexpr int kSpecRing = 4;
    uint32_t *h_spec = nullptr;               // kSpecRing x kMaxTemporal pinned words
    hipEvent_t ev_spec[kSpecRing] = {};
    bool spec_converged = false;              // the last speculative slab solve ended early
    // persistent launches (k_jacobi_persist): allowed until a timeout clears
    // persist_on; each launch gets a new flag epoch from the host (flags start at 0)
    bool persist_on = true;
    uint32_t persist_epoch = 0;
    int last_persist_blocks = 0;   // cfd_get_persist_blocks
    bool capturing = false;   // inside update_graph's capture: no persistent launch
    // the resident solve (k_jacobi_resident): off after a timeout
    static constexpr long kResidentAutoCells = 1l << 21;
    bool resident_off = false;
    uint64_t resident_solves = 0;   // resident launches enqueued (cfd_get_resident_solves)
    bool last_abort_resident = false;
    // fixed-count steps on slabs: the solve residual rides the step all-reduce
    bool merge_res_allreduce = false;

    // --------------------- the other solvers (cfd_model_solvers.hip)
    uint32_t *lex_pol = nullptr, *lex_exit = nullptr;   // script-order SOR's tickets
    size_t lex_words = 0;
    // cfd_script_options: solves 2, 4 and 5 also publish the script's double
    // residual (Ctl::last_p64) through res64, the slot sets their second
    // instantiations raise (cfd_internal.h kRes64Words; allocated while the
    // option is set).  p64_valid: the last solve enqueued published one.
    cfd_script_options sopt{};
    unsigned long long *res64 = nullptr;
    bool p64_valid = false;
    // multigrid hierarchy (cfd_solvers.hip), built on the first multigrid solve
    std::vector<cfd::MgLevel> mg;     // level table; level 0's a/b are the p' buffers of the solve
    cfd::MgLevel *mg_dev = nullptr;   // device copy for k_mg_tail
    float *mg_pool = nullptr;
    int mg_tail = 0;             // first level handled inside the single-workgroup tail
    int mg_P = 0;                // partitioned levels (enqueue_mg_partitioned)
    static constexpr int kMgGhost = 8;   // >= 7: 5 sweeps + residual + the restriction's row
    static constexpr int kSmT5 = 5;      // the smoothing window's halo (5 sweeps)
    struct MgX {
        int l, which, depth;
    };

    // ------------------------------------------ the step (cfd_model_step.hip)
    bool step_begin_folded = false;   // this step's (enqueue_update)
    bool uv_async = false;   // this step's u/v exchange runs on cstream (enqueue_update)
    bool stepped = false;    // ev_step0 / ev_step1 hold a step
    hipGraphExec_t step_graph = nullptr;
    int graph_cur_delta = 0;   // host_cur advance of one replay
    // the uv-fused step (cfd_options::uv_fused): its finish stores the new
    // u, v into the u_old / v_old arrays and the host swaps the pairs in
    // Fields, so f.u / f.v are always the current fields and f.u_old / f.v_old
    // the step's old ones.  uv_flip: the pairs are swapped against the
    // allocation order; star_lazy: the last step stored no u*, v* (need_star
    // materialises them from the old pair before anything reads them)
    int uv_flip = 0, graph_uv_flip = 0, graph_uv_delta = 0, ck_uv_flip = 0;
    bool star_lazy = false, ck_star_lazy = false;
    int graph_steps = 4;
    // self-recovery checkpoint (ck_begin)
    struct CkSeg {
        void *ptr;
        size_t bytes;
    };
    std::vector<CkSeg> ck_segs;   // u, v, u_old, v_old, u*, v*, p, rhs, p' x2, Ctl
    char *ck_pool = nullptr;
    size_t ck_bytes = 0;
    bool ck_open = false;
    int ck_host_cur = 0;
    bool ck_shallow = false;
    std::vector<std::function<int()>> ck_replay;
    uint64_t recoveries = 0;   // cfd_get_recoveries

    // ------------------------------------------------------------- timing
    hipEvent_t ev_step0 = nullptr, ev_step1 = nullptr, ev_prof0 = nullptr, ev_prof1 = nullptr;
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    size_t ev_next = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> solve_events;
    std::vector<hipEvent_t> step_events;
    uint64_t timed_sweeps = 0, timed_steps = 0, timed_launches = 0;
    double timed_step_ms = 0.0;
    // per-phase events (cfd_timing_phases): [0] predictors + first
    // divergence, [1] the corrector / finish, [2] the RCCL halo exchanges and
    // all-reduces (each on the stream it runs on, waiting for the peer
    // included), summed at cfd_timing_end
    bool timing_phases = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> phase_events[3];
    double phase_ms[3] = {0.0, 0.0, 0.0};
    uint64_t phase_count[3] = {0, 0, 0};

    // ------------- tracers and the script's substep (cfd_model_extras.hip)
    // One allocation: TrcCtl and the tile words, then x, y, initialY of both
    // buffers.  While enabled it is one more segment of the self-recovery
    // checkpoint (a replayed step moves the tracers again), and steps are not
    // replayed from a captured graph (graph_ok).
    cfd::Tracers trc{};
    char *trc_pool = nullptr;
    size_t trc_bytes = 0;
    int trc_grid = 0;            // workgroups per launch: from the capacity, at most 8 per CU
    uint32_t *trc_dens = nullptr;   // cfd_tracers_density's nx * ny counts
    // One allocation, built at first use (the grid never changes after
    // creation): the obstacle face intervals of u (2 ny ints) and v
    // (2 (ny + 1) ints), then the ny inlet values, re-uploaded when a call's
    // (inlet_velocity, profile) differs from the last upload's.
    char *scr_pool = nullptr;
    cfd::ScriptStep scr{};
    std::vector<float> scr_inlet_h;
    double scr_inlet_v = 0.0;
    int scr_inlet_profile = -1;   // -1: nothing uploaded yet

    // ------------------ the script's time step (cfd_model_script.hip)
    // One allocation at the first cfd_script_begin: uPrev, vPrev, uOld, vOld,
    // then the step's reduction block (cfd_internal.h kScrRedWords); su_h is
    // its pinned host copy.  The host scalars are the script's globals.
    char *su_pool = nullptr;
    float *su_uprev = nullptr, *su_vprev = nullptr, *su_uold = nullptr, *su_vold = nullptr;
    unsigned long long *su_red = nullptr, *su_h = nullptr;
    bool su_begun = false, su_bad = false;
    bool su_failed = false;       // an update failed after its begin pass: u, v are mid-step
    bool su_dt_set = false;       // false: the first update takes dt_user (`let dt` is the input's value)
    double su_dt = 0.0;           // let dt
    int32_t su_substeps = 5;      // let substepCount
    uint64_t su_steps = 0;        // simulationStepCount
    double su_inlet = 0.0;        // currentInletVelocity
    double su_pmax64 = 0.0;       // maxPressureResidual of the last update whose solves published doubles

    // ============================================================ methods
    bool sharded() const { return n_ranks > 1; }
    size_t u_rows_alloc() const { return (size_t)g.nyl + 2 * cfd::kGhostUV; }
    size_t v_rows_alloc() const { return (size_t)g.nyl + 1 + 2 * cfd::kGhostUV; }

    // ---- cfd_model_comm.hip
    struct HaloX {
        int id, kind, depth;
    };
    float *field_ptr(int id);
    size_t field_pitch(int id) const { return id == FLD_U ? (size_t)g.nx + 1 : (size_t)g.nx; }
    int exchange_group(std::initializer_list<HaloX> items, hipStream_t st);
    int exchange_ops(int id, int kind, int depth, hipStream_t st);
    int exchange_local(int id, int kind, int depth, hipStream_t st);
    // Ghost-row exchange of one field with both neighbours
    int exchange(int id, int kind, int depth, hipStream_t st = nullptr) {
        return exchange_group({{id, kind, depth}}, st);
    }
    // u/v ghost rows before the predictors: both fields in
    // ONE RCCL group (one launch latency over xGMI instead of two).
    int exchange_uv(hipStream_t st = nullptr) {
        return exchange_group({{FLD_U, cfd::HALO_U, 2}, {FLD_V, cfd::HALO_V, 2}}, st);
    }
    // p' halo: `rows` owned boundary rows of buffer `buf` each way.
    int exchange_pp(int buf, int rows, hipStream_t st = nullptr) {
        return exchange(buf ? FLD_PP1 : FLD_PP0, cfd::HALO_PP, rows, st);
    }
    // rhs ghosts `rhs_rows` deep and p' buffer `buf`'s `pp_rows` deep in ONE
    // RCCL group (one collective call: the speculative slab solve's first block)
    int exchange_rhs_pp(int rhs_rows, int buf, int pp_rows) {
        return exchange_group({{FLD_RHS, cfd::HALO_PP, rhs_rows},
                               {buf ? FLD_PP1 : FLD_PP0, cfd::HALO_PP, pp_rows}}, nullptr);
    }
    int allreduce_max_u32(uint32_t *dev, size_t n);
    int settle(ncclResult_t r, const char *what);
    int wait_done(hipEvent_t ev);

    // ---- cfd_model_jacobi.hip
    bool spec_mode() const;
    bool resident_mode() const;
    bool spec_slab_ok() const;
    bool host_driven() const;
    int gate_wait(PersistGate &gate, bool always);
    int launch_persist(int pass, int par0, int nblk, int lo, int hi, int res_it, bool *done);
    int enqueue_solve(int pass);
    int enqueue_jacobi_single(int pass);
    int enqueue_jacobi_slabs(int pass);
    int enqueue_spec_slabs(int pass);
    int enqueue_solve_host_driven(float *residual_out);

    // ---- cfd_model_solvers.hip
    static void level_consts(double dx, double dy, double *dx2, double *dy2, double *denom,
                             double *r, int32_t *fast);
    cfd::SorConst sor_consts() const;
    int enqueue_sor(int pass);
    int enqueue_sor_sharded(const cfd::SorConst &k, int pass, float *residual_out, hipEvent_t e0);
    int enqueue_sor_sharded_deep(const cfd::SorConst &k, int pass, hipEvent_t e0);
    int enqueue_sor_lex(int pass);
    int enqueue_jacobi_script(int pass);
    // the double residual's slot sets when this model's solves publish it, else null
    unsigned long long *res64_on() const { return sopt.residual_f64 && !sharded() ? res64 : nullptr; }
    int clear_res64();
    void mg_rows(int l, int r, int *j0o, int *j1o) const;
    int mg_partition_levels(const std::vector<std::pair<int, int>> &dims, int tail) const;
    int mg_build();
    int gather_rhs();
    int mg_exchange(std::initializer_list<MgX> items);
    int mg_allgather_rhs(int l);
    int enqueue_mg_partitioned(int pass, float *residual_out, hipEvent_t e0);
    int enqueue_mg(int pass, float *residual_out = nullptr);

    // ---- cfd_model_step.hip
    hipEvent_t take_event();
    hipEvent_t phase_mark(int ph, bool end, hipStream_t st = nullptr);
    void begin_solve_timing(int pass, hipEvent_t *e0);
    void end_solve_timing(hipEvent_t e0, uint64_t sweeps, uint64_t launches);
    void pass_head(int pass, float dt_override);
    int enqueue_piso(float dt_override, bool finish = false);
    int enqueue_update(bool rec_step = true);
    bool uv_fused_ok() const;
    void swap_uv();
    int need_star();
    bool graph_ok() const;
    void drop_graph();
    int update_graph(int n);
    int abort_allreduce();
    int sync();
    int read_ctl(cfd::Ctl *out);
    int persist_timeout_check(bool at_sync);
    bool ckpt_needed() const;
    int ck_begin();
    void ck_record(std::function<int()> fn);
    void ck_commit();
    int ck_drop_pool();
    int recover();
    int invalidate_sums();
    int clear_abort_words();

    // ---- cfd_model_extras.hip
    int trc_release();
    bool scr_in_obstacle(double x, double y) const;
    int script_build();
    int script_prepare(const cfd_script_step *s, cfd::ScriptStep *out);
    int script_substep(const cfd_script_step *s);

    // ---- cfd_model_script.hip
    int su_alloc();
    int su_update(const cfd_script_config *c, cfd_script_report *out);

    // ---- cfd_model_build.hip
    void destroy();
};

namespace cfd {
// ---- cfd_model_build.hip
cfd_options read_options();
int validate(const cfd_grid *grid, const cfd_params *p);
int validate_sharded(const cfd_model *m, const cfd_params *p);
void apply_params(cfd_model *m, const cfd_params *p);
void set_sums_track(cfd_model *m);
int create_model(const cfd_grid *grid, const cfd_params *params, int device, int n_ranks, int rank,
                 const void *uid, LocalHub *hub, cfd_model **out);
// ---- cfd_model_extras.hip: the argument and model checks of cfd_script_piso_step
int script_check(cfd_model *m, const cfd_script_step *s);
// ---- cfd_model_comm.hip
int comm_init(cfd_model *m, const ncclUniqueId &id, int n_ranks, int rank);
// ---- cfd_model_jacobi.hip
PersistGate &persist_gate(int device);
}  // namespace cfd
