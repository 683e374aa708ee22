/*
 * cfd.h — C ABI of the MI355X-native pressure-projection hot path of
 * TSultanov/cfd-demo (src/model.rs).  Plain C types only: an opaque handle,
 * POD structs, float/uint8 pointers and sizes.  No torch or HIP types cross
 * this boundary.
 *
 * Each entry point replaces one method of the reference's `Model`
 * (/root/reference/src/model.rs); the citation is given per function.  The
 * reference has no FFI of its own; INTEGRATION.md shows the Rust `extern "C"`
 * block and wrapper a maintainer would add to keep src/app.rs unchanged.
 *
 * Conventions
 *   - return 0 on success, a negative cfd_status on failure; cfd_last_error()
 *     returns a thread-local message for the last failure on this thread.
 *   - a handle is thread-affine (the reference moves Model into one worker
 *     thread, model.rs:1287); calls on one handle must not race.
 *   - host buffers are caller-owned; sizes follow the reference's flat
 *     row-major layout (model.rs:161-214):
 *        u: (nx+1)*ny   v: nx*(ny+1)   p, rhs, p_prime: nx*ny
 *     For a sharded model (cfd_create_sharded) every host buffer covers the
 *     rank's slab only: pressure rows [j0, j1) (cfd_get_slab), u rows
 *     [j0, j1), v rows [j0, j1] (the shared face row j1 is held by both
 *     neighbouring ranks).
 *   - the precondition nx % 8 == 0 of the reference's 8-lane loops
 *     (model.rs:541, 402-403) is enforced: other shapes return CFD_EINVAL.
 *   - cfd_update / cfd_update_n are asynchronous: they enqueue the step on the
 *     model's HIP stream and return.  Reading calls (snapshot, state,
 *     residuals) synchronise.
 */
#ifndef CFD_H
#define CFD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CFD_ABI_VERSION 1

typedef enum {
    CFD_OK = 0,
    CFD_EINVAL = -1,   /* bad argument or unsupported shape (nx % 8 != 0, ...) */
    CFD_EHIP = -2,     /* HIP runtime error (no device, out of memory, launch) */
    CFD_ERCCL = -3,    /* RCCL error (sharded models only) */
    CFD_ESTATE = -4,   /* call not valid in the model's current state */
    CFD_ENONFINITE = -5, /* a finished step left NaN/Inf in u or v (failure detection;
                            the reference has none): cfd_update refuses to step on
                            and cfd_get_residuals reports it (filling *out all the
                            same) until cfd_set_state injects a new state */
    CFD_ETIMEOUT = -6, /* a persistent Jacobi solve (k_jacobi_persist: CFD_PERSIST=1,
                          or slabs with CFD_PERSIST_SHARDED=1) or the resident
                          tolerance-mode solve (k_jacobi_resident: small single-domain
                          grids by default) waited past its deadline
                          (CFD_PERSIST_DEADLINE_US, default 10 s).  For the persistent
                          solve that is a fault (it completes with any number of its
                          workgroups resident); the resident solve needs all its
                          workgroups co-resident, so co-tenant kernels that hold CUs for
                          seconds can cause it.  Self-recovering since r5: the model
                          checkpoints its state (device copies) before the first
                          cfd_update_n / cfd_pressure_solve / cfd_piso_step after a
                          synchronisation whenever such a solve may run; the call that
                          detects the timeout (a synchronising call, or the next
                          cfd_update_n on a single domain) restores that checkpoint,
                          re-runs every call since with one launch per block, and
                          returns CFD_ETIMEOUT with the state VALID (that detecting
                          cfd_update_n itself enqueued nothing).  Slabs tell each
                          other through the step all-reduce and recover at the same
                          synchronisation.  Solves run per launch from then on;
                          cfd_get_recoveries counts these.  CFD_CKPT=0 disables the
                          checkpoint: the state is then invalid until cfd_set_state */
} cfd_status;

typedef struct cfd_model cfd_model;

/* Grid + optional Cylinder (model.rs:119-139).  dx = lx/nx and dy = ly/ny
 * are derived exactly as src/app.rs:37-38 does. */
typedef struct {
    uint64_t nx, ny;
    float lx, ly;
    int32_t has_cylinder;
    float cylinder_x, cylinder_y, cylinder_radius;
} cfd_grid;

/* SimulationParams (model.rs:13-21) + this build's knobs.  Reference
 * behaviour is jacobi_iters 50, corrector_passes 20, tol_enabled 1,
 * p_tol 1e-4, bc_kind CFD_BC_CHANNEL. */
enum { CFD_SCHEME_FIRST_ORDER = 0, CFD_SCHEME_SECOND_ORDER = 1 };
enum { CFD_INLET_UNIFORM = 0, CFD_INLET_PARABOLIC = 1 };
/* Pressure solver of each solve piso_step runs (model.rs:684, :710).
 * JACOBI is the reference's (model.rs:734-824).  SOR and MULTIGRID are the
 * solvers of the reference's JavaScript variant (index.html:741-774 and
 * :775-795 + :1344-1470): p' restarts from 0 each solve, arithmetic in double
 * with f32 storage as in the script; SOR is swept red-black (omega 1.7,
 * jacobi_iters iterations, early exit at p_tol); MULTIGRID runs 3 V-cycles and
 * reports max |A p' - rhs|.  Both run on sharded models too (>= 16 interior
 * rows and halo depth >= 2 per slab), bit-identical to the unsharded solve.
 * SOR, fixed count (tol_enabled 0): deep ghosts -- an hg-row p' exchange
 * every hg/2 iterations, the iterations between recomputing shrinking ghost
 * bands; with the tolerance on, a 2-row exchange and an all-reduced residual
 * per iteration (checked one iteration behind).  MULTIGRID: the fine levels
 * whose every slab boundary divides by 2^(l+1) (>= 16 rows per slab there)
 * are partitioned -- each rank smooths, forms residuals and restricts only
 * its rows, with 8-row ghost exchanges per level -- and the coarser levels
 * are gathered and solved whole on every rank.
 * SOR_LEX (value 4; 3 is unassigned and stays rejected with CFD_EINVAL, as
 * before this solver existed) is the script's SOR in the script's own order
 * (index.html:741-774):
 * p' restarts from 0 and is updated in place, row by row, left to right,
 * omega 1.7, in double with f32 stores, then rows 0 / ny-1 and columns 0 /
 * nx-1 are copied as :761-770 does; the iterates are the script's bit for bit
 * (tests/golden/js_sor_*.npz hold the script's own results under node).  It
 * runs jacobi_iters iterations with the early exit at p_tol when tol_enabled,
 * reports (float)maxError of the last iteration run, and jacobi_sweeps_total
 * grows by the iterations run -- the conventions of CFD_SOLVER_SOR.  The one
 * place its arithmetic can differ from the script: the script compares the
 * double maxError with the double 1e-4, this library (float)maxError with the
 * float p_tol, as CFD_SOLVER_SOR does; the two disagree only when maxError
 * falls in the sliver just below 1e-4 that rounds to or above f32(1e-4).
 * One domain only: cfd_create_sharded* and a cfd_set_params on a sharded
 * model return CFD_EINVAL for it.  On the GPU it is a pipelined wavefront of
 * (iteration, 64-row band) tasks in one launch (cfd_sor_lex.hip);
 * CFD_SOR_LEX_WGS=N caps its workgroups (any N >= 1 gives the same bits).  Its
 * waits are bounded like the persistent Jacobi solve's
 * (CFD_PERSIST_DEADLINE_US): past the deadline the next synchronising call
 * returns CFD_ETIMEOUT and p' is invalid until cfd_set_state (no checkpoint
 * is kept for this solver).
 * JACOBI_SCRIPT (value 5) is the script's default solver, its Jacobi branch
 * (index.html:796-838): p' restarts from 0; per iteration, over the interior,
 *   new = 0.7 * ((E + W)/(dx*dx) + (N + S)/(dy*dy) - rhs) / denom + (1 - 0.7) * old
 * with denom = 2/dx2 + 2/dy2 as :181-183 builds it, every operation in double
 * in the script's order ((1 - 0.7) is the double 0.30000000000000004) and one
 * rounding to f32 on the store; maxError = max |new - old| over the interior,
 * on the stored values widened, NaN ignored; then the interior is copied back,
 * rows 0 / ny-1 take rows 1 / ny-2 over all columns, column 0 takes column 1
 * and column nx-1 is 0 over all rows, in that order (:828-835).  The iterates
 * are the script's bit for bit (tests/golden/js_jac_*.npz).  Conventions as
 * SOR_LEX: jacobi_iters iterations (the script's 50) with the early exit at
 * p_tol when tol_enabled (the script's 1e-6), (float)maxError of the last
 * iteration run reported, jacobi_sweeps_total grows by the iterations run, and
 * the same sliver: the script tests the double against the double 1e-6, this
 * library the float against the float p_tol.  One domain only, as SOR_LEX.  On
 * the GPU one iteration is one launch (cfd_jacobi_script.hip: update, maximum
 * and boundary copies; p' ping-pongs), the exit is decided on the device and no
 * workgroup waits for another, so it has no deadline and cannot time out.
 * With jacobi_iters 0 (the script's count is a constant 50) p' is 0 and the
 * reported residual is 0, as for SOR_LEX, where the script's branch would leave
 * lastPResidual = Infinity (:801, :838). */
enum { CFD_SOLVER_JACOBI = 0, CFD_SOLVER_SOR = 1, CFD_SOLVER_MULTIGRID = 2, CFD_SOLVER_SOR_LEX = 4,
       CFD_SOLVER_JACOBI_SCRIPT = 5 };
enum { CFD_BC_CHANNEL = 0, CFD_BC_CAVITY = 1 };
typedef struct {
    float dt;
    float viscosity;
    float target_inlet_velocity;   /* channel: inlet U; cavity: lid U */
    int32_t velocity_scheme;
    int32_t inlet_profile;
    int32_t pressure_solver;
    int32_t jacobi_iters;          /* sweeps per pressure solve (model.rs:737) */
    int32_t corrector_passes;      /* extra correction passes (model.rs:696) */
    int32_t tol_enabled;           /* early exits at p_tol (model.rs:816, 721) */
    float p_tol;
    int32_t bc_kind;
} cfd_params;

/* Residuals (model.rs:23-32). step_time_s is device time of the last step
 * measured with HIP events. */
typedef struct {
    uint64_t simulation_step;
    float simulation_time;
    float dt;
    float p, u, v;
    double step_time_s;
    uint32_t piso_substeps;
    uint64_t jacobi_sweeps_total;
} cfd_residuals;

/* Full persistent state: enough to resume bit-exactly.
 * Any pointer may be NULL to skip that field. */
typedef struct {
    float *u, *v, *p, *u_star, *v_star, *p_prime, *rhs;
    float dt;
    float simulation_time;
    uint64_t simulation_step;
    float last_p_residual, last_u_residual, last_v_residual;
    uint64_t jacobi_sweeps_total;
} cfd_state;

/* SimulationParams::default() (model.rs:44-55) + reference knob values. */
void cfd_default_params(cfd_params *out);
/* default_grid() (src/app.rs:32-53): 800 x 264, 30 x 10, cylinder r 0.75. */
void cfd_default_grid(cfd_grid *out);

/* Model::new (model.rs:219-299) on HIP device `device_ordinal`. */
int cfd_create(const cfd_grid *grid, const cfd_params *params, int device_ordinal,
               cfd_model **out);

/* 1D row-slab decomposition over n_ranks processes (one per GPU).  Rank 0
 * calls cfd_rccl_unique_id and distributes the 128 bytes out of band
 * (bench.py uses torch.distributed).  Results are bitwise identical to the
 * single-GPU model: the path has no sums across ranks, only halo copies and
 * exact maxima. */
int cfd_rccl_unique_id(void *out_128_bytes);
int cfd_create_sharded(const cfd_grid *grid, const cfd_params *params, int device_ordinal,
                       int n_ranks, int rank, const void *rccl_unique_id, cfd_model **out);
/* Testing stand-in for the RCCL communicator: n_ranks slabs inside ONE
 * process (one host thread per slab, any devices, several may share a GPU);
 * halo exchanges become device-to-device copies between the members and the
 * max all-reduce a host fold.  Kernels and row plans are those of the RCCL
 * path; only the transport differs.  Destroy the hub after its members. */
void *cfd_local_hub_create(int n_ranks);
void cfd_local_hub_destroy(void *hub);
int cfd_create_sharded_local(const cfd_grid *grid, const cfd_params *params, int device_ordinal,
                             int n_ranks, int rank, void *hub, cfd_model **out);
/* HIP devices visible to this process (bench.py's launched ranks check that
 * there is one per rank before creating anything). */
int cfd_device_count(int *n_out);
/* Ranks the model's transport reports: ncclCommCount of the RCCL
 * communicator, the LocalHub's size, or 1 for an unsharded model. */
int cfd_get_comm_size(const cfd_model *m, int *n_out);
/* Global pressure rows [j0, j1) held by this model (0, ny for cfd_create). */
int cfd_get_slab(const cfd_model *m, uint64_t *j0, uint64_t *j1);

/* Model::update (model.rs:304-379): one time step, asynchronous. */
int cfd_update(cfd_model *m);
/* n consecutive Model::update calls, enqueued without host round trips. */
int cfd_update_n(cfd_model *m, int n);
/* piso_step (model.rs:529-730) with an explicit dt_sub; no u_old copy, no
 * residual/CFL bookkeeping. */
int cfd_piso_step(cfd_model *m, float dt_sub);
/* jacobi_pressure (model.rs:734-824) on the current rhs and p_prime.
 * Synchronous; writes the returned max |dp'| to *residual_out (may be NULL). */
int cfd_pressure_solve(cfd_model *m, float *residual_out);

/* Single phases of piso_step, for known-answer tests. */
enum {
    CFD_PHASE_U_PREDICTOR = 0,   /* model.rs:538-580   */
    CFD_PHASE_V_PREDICTOR = 1,   /* model.rs:586-670   */
    CFD_PHASE_DIVERGENCE = 2,    /* model.rs:1406-1440 */
    CFD_PHASE_CORRECTOR = 3,     /* model.rs:1334-1404 */
    CFD_PHASE_BOUNDARY = 4,      /* model.rs:826-875   */
};
int cfd_run_phase(cfd_model *m, int phase, float dt_sub);

/* set_parameters (model.rs:1250-1257). */
int cfd_set_params(cfd_model *m, const cfd_params *params);
/* get_snapshot (model.rs:1259-1267): copies u, v, p (NULL skips) and dt. */
int cfd_get_snapshot(cfd_model *m, float *u, float *v, float *p, float *dt_out);
/* get_residuals (model.rs:1269-1280). */
int cfd_get_residuals(cfd_model *m, cfd_residuals *out);
/* Whole state, for fixtures and checkpoint/resume. */
int cfd_get_state(cfd_model *m, cfd_state *st);
int cfd_set_state(cfd_model *m, const cfd_state *st);
/* Obstacle masks as built by Model::new (u8, u and v layouts). */
int cfd_get_masks(cfd_model *m, uint8_t *mask_u, uint8_t *mask_v);

/* Wait for all work enqueued on the model's stream. */
int cfd_synchronize(cfd_model *m);
/* Last Jacobi kernel duration in ms averaged over the sweeps of the most
 * recent cfd_profile_sweeps() call; measured with HIP events on the
 * model's stream. */
int cfd_profile_sweeps(cfd_model *m, int n_sweeps, double *avg_ms_out);

/* Event timing of the pressure solves and whole steps inside cfd_update:
 * cfd_timing_begin starts recording, cfd_timing_end synchronises and returns
 * the summed solve time, sweeps timed, summed step time and steps timed. */
int cfd_timing_begin(cfd_model *m);
int cfd_timing_end(cfd_model *m, double *solve_ms, uint64_t *sweeps, double *step_ms,
                   uint64_t *steps);
/* Per-phase timing inside the timing window (off by default: every event
 * record costs the step a few microseconds): with on != 0, the following
 * cfd_timing_begin/end windows also time each step's predictor + first
 * divergence phase (model.rs:538-676) and its corrector / fused finish
 * (model.rs:693, 728, 333-377); cfd_timing_phase_ms returns the sums of the
 * last window (0 when a phase was not timed). */
int cfd_timing_phases(cfd_model *m, int on);
int cfd_timing_phase_ms(const cfd_model *m, double *predict_ms, double *finish_ms);
/* Sharded models over RCCL, same windows: the summed duration of every halo
 * exchange group and all-reduce on the stream it runs on (waiting for the
 * peer included), and how many there were.  (new; per-rank exchange time) */
int cfd_timing_exchange_ms(const cfd_model *m, double *exchange_ms, uint64_t *exchanges);
/* p' halo depth (rows exchanged per RCCL round) of a sharded model. */
int cfd_get_halo_depth(const cfd_model *m);
/* Jacobi kernel configuration chosen at creation: division form proven exact
 * for this grid's divisors (0 IEEE, 1 reciprocal multiply, 2 FMA-corrected)
 * and sweeps per launch (1 when the tolerance is on). */
int cfd_get_kernel_config(const cfd_model *m, int *fastdiv, int *temporal);
/* The Jacobi kernel a solve launches: kind 0 single sweep (k_jacobi), 1
 * register-march temporal blocking (k_jacobi_tb), 4 the prefetch-pipelined
 * register march, 2 columns per lane (k_jacobi_pipe), 5 the
 * LDS row march (k_jacobi_lds; with the tolerance on its speculative form), 6
 * the tolerance-mode solve of a small grid as one resident launch
 * (k_jacobi_resident, default up to 2^21 cells; CFD_RESIDENT=0/1 forces), and
 * its instantiated name as rocprofv3 reports it (NUL-terminated, truncated to
 * name_len). */
int cfd_get_jacobi_kernel(const cfd_model *m, int *kind, char *name, size_t name_len);

/* Blocks of 8 sweeps the model's last fixed-count solve ran inside ONE
 * persistent launch (k_jacobi_persist; 0: none, every block its own launch).
 * Blocks after them (shorter ones of an uneven split) are k_jacobi_lds
 * launches of their own. */
int cfd_get_persist_blocks(const cfd_model *m, int *blocks);
/* Blocks of persistent solves that a workgroup ran for a neighbour tile whose
 * owner had not claimed them (k_jacobi_persist stealing; 0 when every owner
 * was resident), summed over the model's life.  Synchronises.  (new) */
int cfd_get_persist_steals(cfd_model *m, uint64_t *steals);
/* 8-sweep blocks run in the SUMS form -- (h + v) / dx^2 for h / dx^2 +
 * v / dy^2, one instruction per column pair and sweep fewer, taken only where
 * a guard proves it bitwise: persistent-solve blocks per tile
 * (k_jacobi_persist's per-task guard), summed over the model's life.
 * Synchronises.  (new; diagnostics) */
int cfd_get_persist_sums(cfd_model *m, uint64_t *blocks);
/* Per-launch marches (k_jacobi_lds, fixed-count solves of one domain) that ran
 * the fma form -- fma(h + v, 1/dx^2, -rhs), two instructions per column pair
 * and sweep fewer -- under the whole-solve guard whose maxima the corrector
 * finish and the predictor march publish, summed over the model's life.
 * CFD_JACOBI_SUMS=0 keeps it at 0.  Synchronises.  (new; diagnostics) */
int cfd_get_sums_launches(cfd_model *m, uint64_t *launches);
/* The words that guard reads, as they stand now: state (0 nothing valid, 1 the
 * corrector finish bounded the p' the next solve starts from, 2 the predictor
 * march bounded its rhs as well), and the bounds of max |p'| and max |rhs| as
 * f32 bits with the sign cleared (NaN and Inf compare above every finite
 * value).  Each bound is at least its threshold (2^122 dx^2, 2^112) once
 * published.  All zero for a model that never keeps them (sharded, another
 * solver, the tolerance on, a grid without the form, CFD_JACOBI_SUMS=0).
 * Read-only; synchronises.  (new; diagnostics) */
int cfd_get_sums_bounds(cfd_model *m, uint32_t *state, uint32_t *m0_bits, uint32_t *rm_bits);
/* Collective calls this (sharded) model has enqueued: halo-exchange groups
 * and all-reduces, summed over its life (0 unsharded).  (new; diagnostics) */
int cfd_get_comm_calls(const cfd_model *m, uint64_t *n);
/* Solve timeouts this model recovered from by itself (CFD_ETIMEOUT). */
int cfd_get_recoveries(const cfd_model *m, uint64_t *n);
/* Tolerance-mode solves this model enqueued as one resident launch
 * (k_jacobi_resident, see cfd_get_jacobi_kernel kind 6); diagnostics. */
int cfd_get_resident_solves(const cfd_model *m, uint64_t *solves);
/* The tile plan of that resident launch as the model's next tolerance-mode
 * solve would take it: rows and columns of a tile's output cells, tiles in the
 * grid and workgroups launched.  CFD_ESTATE when the model would not take the
 * resident solve (kind != 6).  Read-only; diagnostics. */
int cfd_get_resident_geometry(const cfd_model *m, int *br, int *bc, int *tiles, int *wgs);
/* The tile geometry of the model's 8-sweep kind-5 Jacobi launch over its
 * first block's rows (persist != 0: the persistent form's): the dynamic LDS
 * pad in bytes (24 KiB caps a CU at 3 four-wave workgroups on cache-resident
 * slabs), the workgroups per CU the round is sized for, the wave columns and
 * the wave segments per column.  (new; diagnostics) */
int cfd_get_jacobi_geometry(const cfd_model *m, int persist, int *lds_pad, int *wgs_per_cu,
                            int *wave_cols, int *segments);

/* Host-only slab plan used by cfd_create_sharded (no device needed; the
 * multi-rank CPU tests drive the same plan):
 *   cfd_plan_slab  — global pressure rows [j0, j1) of `rank`;
 *   cfd_plan_sweep — local rows [lo, hi) that sweep `it` of an `iters`-sweep
 *                    solve recomputes with halo depth d, and whether d rows
 *                    of p' are exchanged after it;
 *   cfd_plan_halo  — ghost geometry of a field (kind 0 u, 1 v, 2 p'):
 *                    out6 = {send, recv, rows} with rank-1, then with rank+1,
 *                    in local rows. */
int cfd_plan_slab(uint64_t ny, int n_ranks, int rank, uint64_t *j0, uint64_t *j1);
int cfd_plan_sweep(int j0, int nyl, int ny, int halo_depth, int it, int iters, int *lo, int *hi,
                   int *exchange);
int cfd_plan_halo(int kind, int nyl, int depth, int rank, int n_ranks, int *out6);
/* The overlapped exchange block: out6 = the two bands the
 * p' exchange sends ({lo, hi} to rank-1, then to rank+1; empty without a
 * neighbour) and the interior {lo, hi} computed while it travels; returns 1
 * when the block splits, 0 when the slab is too thin (run it whole). */
int cfd_plan_overlap(int nyl, int halo_depth, int rank, int n_ranks, int lo, int hi, int *out6);
/* Temporally blocked form of cfd_plan_sweep: the launch starting at sweep
 * `it` runs *T <= t_max sweeps and stores its last sweep on local rows
 * [out_lo, out_hi); halo_depth <= 0 means unsharded. */
int cfd_plan_block(int j0, int nyl, int ny, int halo_depth, int it, int t_max, int iters, int *T,
                   int *out_lo, int *out_hi, int *exchange);

/* Visualisation modes of App (src/app.rs:505-509 VisualizationMode). */
typedef enum { CFD_VIS_PRESSURE = 0, CFD_VIS_VELOCITY = 1, CFD_VIS_VORTICITY = 2 } cfd_vis_mode;

/* Device-side equivalent of the image App::update_simulation_view builds
 * from a snapshot (src/app.rs:235-403): derive the mode's scalar field
 * (p; cell-centred |velocity|; interior vorticity, 0 elsewhere), its min/max
 * (NaN ignored) and the RGBA8 image (r = (norm*255) as u8, g = 0,
 * b = ((1-norm)*255) as u8, a = 255; cells whose centre is within the
 * cylinder radius, `<=`, grey 128), all on the device; only nx*ny*4 bytes
 * are copied into rgba (row-major, x fastest; NULL skips the image).
 * min_max_out (2 floats, may be NULL) gets the field's min and max before
 * the reference's 1e-6 range widening.  Sharded: the rank's slab rows, with
 * min/max reduced over all ranks (collective: every rank must call). */
int cfd_render(cfd_model *m, int mode, uint8_t *rgba, float *min_max_out);
/* The mode's derived scalar field itself (nx*ny f32; slab rows when sharded). */
int cfd_derive_field(cfd_model *m, int mode, float *out, float *min_max_out);

/* ---- tracer particles (index.html:1472-1543), the script's fourth
 * visualisation mode, as a device-side pass over the solver state ----
 * A tracer is {x, y, initialY}; the list is ordered and the order is kept.
 * All arithmetic is the script's, in double, on the model's f32 u, v, dx, dy,
 * lx, ly and dt widened to double; the lists are the script's bit for bit
 * (tests/golden/js_tracers_*.npz hold the script's own results under node).
 * While enabled, every step of cfd_update / cfd_update_n ends as
 * simulationLoop does (:1231-1238): updateTracers(dt) with the dt the step has
 * just computed, then injectTracers() iff simulation_step % interval == 0 (the
 * count after the step's increment) -- two launches, nothing read back, so a
 * batch of n steps gives the same tracers as n single calls.  Disabled, a step
 * enqueues nothing for them.  Tracers leaving [0, lx] x [0, ly] (or turning
 * NaN) are dropped by a stable compaction; -0 and exactly lx stay.
 * An injection that does not fit the capacity appends nothing and sets a
 * sticky overflow word: cfd_tracers_count / _get / _density then return
 * CFD_ESTATE until cfd_tracers_enable or cfd_tracers_set.
 * One domain only: a tracer reads u and v rows of other slabs, so
 * cfd_tracers_enable returns CFD_EINVAL on a sharded model (like
 * CFD_SOLVER_SOR_LEX).  cfd_get_state / cfd_set_state do not touch tracers;
 * cfd_tracers_get / cfd_tracers_set are their checkpoint.  The model's
 * CFD_ETIMEOUT self-recovery covers them: the tracer buffers are part of its
 * checkpoint, and the explicit calls below synchronise first, so the next
 * checkpoint is taken after them.  Steps are not replayed from a captured
 * graph (CFD_GRAPH=1) while tracers are enabled. */
/* initTracers (:1475-1483): ny tracers at x = 0, y = (j + 0.5) dy.  capacity in
 * [ny, 2^30]; inject_interval <= 0 means tracerInjectionInterval, 100 (:1534).
 * Enabling again starts over. */
int cfd_tracers_enable(cfd_model *m, uint64_t capacity, int inject_interval);
/* tracers = [] (:1311); frees the buffers. */
int cfd_tracers_disable(cfd_model *m);
/* tracers.length.  Synchronises. */
int cfd_tracers_count(cfd_model *m, uint64_t *n);
/* The first min(count, max) tracers in list order (NULL skips an array);
 * *n_out = tracers copied.  Synchronises. */
int cfd_tracers_get(cfd_model *m, double *x, double *y, double *initial_y, uint64_t max,
                    uint64_t *n_out);
/* Replace the list.  CFD_EINVAL for n > capacity and for a non-finite value
 * (the script would read u[NaN]); finite positions outside the domain are
 * accepted: they take getVelocityAt's clamps (:1504-1507) and the next
 * advance drops them.  Clears the overflow word. */
int cfd_tracers_set(cfd_model *m, const double *x, const double *y, const double *initial_y,
                    uint64_t n);
/* One updateTracers(dt) (:1485-1497, getVelocityAt :1499-1525) on the current
 * u, v; no injection.  Asynchronous. */
int cfd_tracers_advance(cfd_model *m, double dt);
/* One injectTracers() (:1537-1543).  Asynchronous. */
int cfd_tracers_inject(cfd_model *m);
/* Build-defined, in the spirit of cfd_render: tracers per pressure cell
 * (nx*ny u32, row-major, x fastest), cell = floor(x/dx), floor(y/dy) clipped to
 * the grid, so a large population need not cross PCIe to be drawn.  Integer
 * atomics: exact and independent of order.  Synchronises. */
int cfd_tracers_density(cfd_model *m, uint32_t *counts_nx_ny);

/* ---- the script's own substep (index.html:366-867 pisoStep with
 * :870-930 applyBoundaryConditions) ----
 * What SURVEY Appendix B lists as the JavaScript variant's differences from
 * model.rs, on the device: the u flux through an averaged v, the obstacle
 * tested at each face's own position (isPointInObstacle, `<=` included) rather
 * than through the cell masks of cfd_get_masks, no re-correction loop, double
 * arithmetic over f32 arrays, and the third advection scheme, QUICK.  All
 * arithmetic is the script's, in double, on the model's f32 u, v, p, p', dx, dy,
 * lx, ly and viscosity widened (the convention of cfd_tracers_*); each value
 * stored into a field is rounded to f32 once, as a Float32Array store is.  The
 * fields are the script's bit for bit (tests/golden/js_step_*.npz hold the
 * script's own results under node).  Nothing of the script is "fixed": faces
 * its loops do not visit keep u / v; the second-order and QUICK y-Laplacian of
 * v is (v[idx+2] - 2 v[idx] + v[idx]) / dy^2; every index guard is as written;
 * rhs = (du/dx + dv/dy) / dt_sub over all cells; p += p' over all cells; the
 * boundary pass runs in the script's order (inlet, outlet copy, rows 0 and
 * ny-1 of u, rows 0 and ny of v, obstacle faces).
 * The solve between the two passes is the model's own, unchanged, and must be
 * one of the three pinned to the script: pressure_solver CFD_SOLVER_MULTIGRID,
 * CFD_SOLVER_SOR_LEX or CFD_SOLVER_JACOBI_SCRIPT (all restart p' from 0); any
 * other returns CFD_EINVAL (the red-black SOR and the Rust Jacobi are not the
 * script's).  Its settings come from cfd_params (the script's own: jacobi_iters
 * 50, tol_enabled 1, p_tol 1e-4, or 1e-6 for its Jacobi); its residual lands
 * in cfd_get_state().last_p_residual and jacobi_sweeps_total grows as the solve
 * makes it grow.  simulation_step, dt and the u / v residuals are not touched:
 * like cfd_piso_step this is the substep, not updateSimulation (the caller
 * owns the inlet ramp of :277-281, dt / substepCount and the extrapolation).
 * CFD_EINVAL also for a sharded model (one domain only, as CFD_SOLVER_SOR_LEX
 * and tracers), bc_kind CFD_BC_CAVITY (the script has the channel only), an
 * unknown scheme or profile, a non-finite or non-positive dt_sub and a
 * non-finite inlet_velocity.  velocity_scheme in cfd_params still takes 0 or 1
 * only, and cfd_update never takes this path.  The obstacle faces (per row of
 * faces one column interval; has_cylinder == 0: none) and the inlet column are
 * evaluated on the host in double (sqrt, the parabola) and uploaded. */
enum { CFD_SCRIPT_FIRST = 0, CFD_SCRIPT_SECOND = 1, CFD_SCRIPT_QUICK = 2 };
typedef struct {
    int32_t scheme;          /* currentVelocityScheme: "first" / "second" / "quick" */
    int32_t inlet_profile;   /* CFD_INLET_UNIFORM / CFD_INLET_PARABOLIC (inletProfileSelect) */
    double  inlet_velocity;  /* currentInletVelocity (the caller owns the script's ramp, :277-281) */
    double  dt_sub;          /* dt / substepCount (:282) */
} cfd_script_step;
/* pisoStep(dt_sub) + applyBoundaryConditions(), asynchronous like cfd_piso_step:
 * two launches (k_script_predict, k_script_correct) around the solve's. */
int cfd_script_piso_step(cfd_model *m, const cfd_script_step *s);
/* Its two passes alone, synchronous, for known-answer tests. */
enum { CFD_SCRIPT_PHASE_PREDICT = 0,   /* :368-739  u*, v*, rhs             */
       CFD_SCRIPT_PHASE_CORRECT = 1 }; /* :842-866  u, v, p += p', then BCs */
int cfd_script_phase(cfd_model *m, int phase, const cfd_script_step *s);

/* ---- the script's time step (index.html:261-363 updateSimulation with
 * :1322-1342 computeAutomaticTimeStep, then simulationLoop's tracer tail
 * :1233-1238) ----
 * One cfd_script_update is one updateSimulation(), in the script's order:
 *   extrapolate  (step_count > 0) u = 2u - uPrev, v = 2v - vPrev, each stored as
 *                (float)(2.0 * (double)u - (double)uPrev);
 *   save         uOld = u, vOld = v;
 *   ramp         currentInletVelocity = step_count < 1000
 *                ? (step_count / 1000) * target : target (:277-281);
 *   substeps     substep_count runs of cfd_script_piso_step's path with
 *                dt_sub = dt / substep_count, enqueued back to back, the running
 *                maximum of their pressure residuals kept on the device;
 *   residuals    max |u - uOld|, max |v - vOld| and maxVel = max(|u|, |v|), in
 *                double, NaN ignored as the script's `>` ignores it;
 *   save         uPrev = u, vPrev = v.
 * That is two fused passes of new device work around the substeps' launches
 * (k_script_begin, k_script_end) and one word folded after each solve
 * (k_script_pmax); no field crosses PCIe.  Then ONE synchronisation and one
 * small read-back per step (dt_sub and the substep count are kernel arguments
 * and host loop bounds of the substep), after which the host applies the
 * script's rules in C double, JavaScript's number: step_count++, the substep
 * rule of :310-317 (ceil, floor, the cap 20, the floor 1),
 * computeAutomaticTimeStep (its maxVel === 0 return of dt_user included) and
 * the 1.1 x previous dt limit.  While tracers are enabled each update ends as
 * simulationLoop does: cfd_tracers_advance(dt_next) -- the script passes the
 * dt it has just computed -- then cfd_tracers_inject() iff step_count %
 * interval == 0 after the increment.
 * The pressure residual is the library's, (double)(float)maxError, where the
 * script holds the double.  Rounding is monotone, so the maximum over the
 * substeps commutes with it, and the substep and dt decisions can differ from
 * the script's only when that rounding moves errorNorm across 1e-3, across
 * 1e-4, or across an integer boundary of substepCount * errorNorm / 1e-3 (the
 * sliver note of CFD_SOLVER_SOR_LEX above, one level up); no committed fixture
 * (tests/golden/js_update_*.npz, the script's own numbers under node) is in
 * it.  cfd_script_set_options (below) lifts that caveat: with residual_f64 the
 * solves publish the script's own double, errorNorm, the substep rule,
 * residual_p and the dt rule are taken from it, and the update's decisions are
 * the script's with no such sliver.  residual_scaling adds the page's
 * residualScalingEnabled branch (:338-348) on that double.
 * State: uPrev, vPrev, uOld, vOld on the device and the script's dt,
 * substepCount, simulationStepCount and currentInletVelocity on the host, all
 * allocated by the first cfd_script_begin.  simulation_step, dt and the u / v
 * residuals of the Rust-path state (cfd_get_state) are not touched, cfd_update
 * never takes this path, and steps that use it are not replayed from a
 * captured graph.
 * CFD_EINVAL as cfd_script_piso_step gives it (a sharded model, the cavity, a
 * pressure_solver that is not 2, 4 or 5, a bad scheme or profile), and for a
 * non-finite or non-positive dt_user, a non-finite target and n < 1;
 * CFD_ESTATE before cfd_script_begin; CFD_ENONFINITE, with the report filled,
 * when a residual or dt_next comes out non-finite or dt_next <= 0 (the script
 * would go on dividing by it): further updates then return CFD_ENONFINITE
 * until cfd_script_begin or cfd_script_set_state.  An update that fails for
 * another reason after its first pass was enqueued (a solve's CFD_ETIMEOUT, a
 * HIP error) leaves u and v extrapolated or part-way through the substeps and
 * the script's scalars unchanged; a retry would extrapolate twice, so further
 * updates return CFD_ESTATE until the caller has restored the fields
 * (cfd_set_state) and called cfd_script_begin or cfd_script_set_state. */
typedef struct {            /* what the page's controls hold when the step starts */
    int32_t scheme;         /* CFD_SCRIPT_FIRST / SECOND / QUICK */
    int32_t inlet_profile;  /* CFD_INLET_UNIFORM / CFD_INLET_PARABOLIC */
    double  target_inlet_velocity;  /* inletVelocitySlider */
    double  dt_user;                /* parseFloat(timeStepInput.value) */
} cfd_script_config;
typedef struct {            /* the script's step state; also its checkpoint (with cfd_get_state) */
    double   dt;            /* let dt; 0: unset, the next update takes dt_user */
    int32_t  substep_count; /* let substepCount (5 at page load), in [1, 20] */
    uint64_t step_count;    /* simulationStepCount */
    float   *u_prev, *v_prev;       /* (nx+1)*ny and nx*(ny+1) floats; NULL skips */
} cfd_script_state;
typedef struct {            /* one log line of :320-324 plus the new dt */
    uint64_t step_count;    /* after the increment */
    int32_t  substeps_run, substep_count_next;
    double   residual_u, residual_v, residual_p, dt_next, inlet_velocity;
} cfd_script_report;
/* st NULL: initSimulation (:218-228) -- dt unset, substep_count 5, step 0,
 * uPrev / vPrev = the model's current u, v.  Else as cfd_script_set_state, with
 * uPrev / vPrev = the model's current u, v where a pointer is NULL.
 * Synchronises; clears CFD_ENONFINITE of this path. */
int cfd_script_begin(cfd_model *m, const cfd_script_state *st);
/* Scalars, and uPrev / vPrev into the caller's arrays.  Synchronises. */
int cfd_script_get_state(cfd_model *m, cfd_script_state *st);
/* CFD_EINVAL for a negative or non-finite dt and substep_count outside [1, 20]. */
int cfd_script_set_state(cfd_model *m, const cfd_script_state *st);
int cfd_script_update(cfd_model *m, const cfd_script_config *c, cfd_script_report *out);
/* n updates (the loop, so that a binding crosses the ABI once); out_n: n
 * records or NULL.  Stops at the first failing update. */
int cfd_script_update_n(cfd_model *m, const cfd_script_config *c, int n, cfd_script_report *out_n);

/* ---- the script's double pressure residual and residualScalingEnabled ----
 * residual_f64: solves 2, 4 and 5 (CFD_SOLVER_MULTIGRID, CFD_SOLVER_SOR_LEX,
 * CFD_SOLVER_JACOBI_SCRIPT) run a second instantiation of their residual kernel
 * that folds the maximum as the script's double -- max |new - old| of :757 and
 * :817, max |A p' - rhs| of :784-794, NaN ignored as `>` ignores it -- and
 * publish the double of the last iteration run next to last_p_residual, whose
 * value is its f32 rounding.  The exit test stays (float)maxError < p_tol with
 * the float tolerance (rounding is monotone: the f32 of the double maximum is
 * the maximum of the f32s), so p', last_p_residual, the iterations run and
 * jacobi_sweeps_total are the same bits with the option on or off; the
 * solve-level sliver of CFD_SOLVER_SOR_LEX above (the script compares the
 * double with the double 1e-4 or 1e-6) stays.  cfd_pressure_solve,
 * cfd_piso_step, cfd_script_piso_step and cfd_update publish through the same
 * solve.  With jacobi_iters 0 the double is 0.0; solvers 0 and 1 publish none.
 * cfd_script_update then keeps the running maximum of the substeps' doubles on
 * the device (k_script_pmax64, in k_script_pmax's place; the step's one
 * read-back carries it) and takes errorNorm, the substep rule, residual_p of
 * the report and the dt rule from it: the script's own numbers, with no
 * update-level caveat.
 * residual_scaling (implies residual_f64; setting it reads back residual_f64 1):
 * the host adds :338-348 in C double -- dt_pressure = dt_cfl; if maxP > 1e-3,
 * dt_pressure = dt_cfl * (1e-3 / (maxP + 1e-10)); newDt = min(dt_cfl,
 * dt_pressure) -- before the unchanged 1.1 limit.  An infinite residual gives
 * dt_next 0, which the dt_next <= 0 rule above reports as CFD_ENONFINITE.
 * Both are 0 at creation and persist across cfd_script_begin (initSimulation
 * does not touch the checkbox).  cfd_script_set_options synchronises and drops
 * a captured step graph; CFD_EINVAL on a sharded model and for values other
 * than 0 or 1.  cfd_set_state clears the published double, and the
 * CFD_ETIMEOUT checkpoint covers it. */
typedef struct {
    int32_t residual_f64;      /* solves 2/4/5 publish the script's double; script updates decide from it */
    int32_t residual_scaling;  /* residualScalingEnabled (index.html:338-348); implies residual_f64 */
} cfd_script_options;
int cfd_script_set_options(cfd_model *m, const cfd_script_options *o);
int cfd_script_get_options(const cfd_model *m, cfd_script_options *o);
/* last: the last solve's double residual; step_max: the maximum over the substeps of the last
 * cfd_script_update (NULL skips either; 0.0 before the first such update).  Synchronises.
 * CFD_ESTATE while residual_f64 is off, before a solve has published since the option was set or
 * the state was replaced, and when the last solve was solver 0 or 1. */
int cfd_get_p_residual_f64(cfd_model *m, double *last, double *step_max);

/* The grid and parameters the model runs with (NULL skips either). */
int cfd_get_config(const cfd_model *m, cfd_grid *grid, cfd_params *params);

/* ---- Model::run (model.rs:1282-1332): the asynchronous host runtime ----
 * cfd_run_start hands the model to a worker thread that loops exactly as the
 * reference's (model.rs:1287-1325): drain the queued commands in order
 * (Stop, SetParams, GetSnapshot — at most one snapshot per drain —, Pause,
 * Resume; model.rs:57-63), then either run one cfd_update and queue its
 * residuals, or wait 16 ms while paused.  Until cfd_run_stop returns, only
 * cfd_run_* calls may touch the model.  Any thread may call cfd_run_*.
 * Difference: Stop ends the worker (the reference's Stop only leaves the
 * command loop, model.rs:1296); cfd_run_stop joins it, frees the runner and
 * leaves the model to the caller. */
typedef struct cfd_runner cfd_runner;
int cfd_run_start(cfd_model *m, cfd_runner **out);             /* Model::run        :1282 */
int cfd_run_stop(cfd_runner *r);                               /* handle.stop()     :72   */
int cfd_run_pause(cfd_runner *r);                              /* handle.pause()    :110  */
int cfd_run_resume(cfd_runner *r);                             /* handle.resume()   :114  */
int cfd_run_set_params(cfd_runner *r, const cfd_params *p);    /* handle.set_params :104  */
int cfd_run_request_snapshot(cfd_runner *r);                   /* request_snapshot  :100  */
/* get_last_available_snapshot (:76-86): the newest snapshot published since
 * the previous call (slab sizes as cfd_get_snapshot; NULL skips a field);
 * *available = 0 when there is none. */
int cfd_run_last_snapshot(cfd_runner *r, float *u, float *v, float *p, float *dt_out,
                          int *paused_out, int *available);
/* get_new_log_messages (:88-98): up to `max` queued residual records, oldest
 * first; *n_out = records copied. */
int cfd_run_new_residuals(cfd_runner *r, cfd_residuals *out, int max, int *n_out);
/* Command (drained in order with the others): cfd_tracers_enable(capacity,
 * inject_interval) on the worker's model, or cfd_tracers_disable for capacity
 * 0 (the script's checkbox, index.html:1306-1312).  While enabled, every
 * snapshot the worker publishes carries the tracer list of the same step. */
int cfd_run_set_tracers(cfd_runner *r, uint64_t capacity, int inject_interval);
/* The tracers of the newest snapshot published since the previous call: the
 * first min(count, max) in list order (NULL skips an array), *n_out = tracers
 * copied; *available = 0 when there is none. */
int cfd_run_last_tracers(cfd_runner *r, double *x, double *y, double *initial_y, uint64_t max,
                         uint64_t *n_out, int *available);
/* 0 while the worker is healthy, else the first failing status of a call it
 * made (it then stops stepping and waits for Stop); msg gets the message. */
int cfd_run_status(cfd_runner *r, char *msg, size_t msg_len);
/* Steps the worker has completed. */
uint64_t cfd_run_steps(cfd_runner *r);

/* ---- the adaptive quadtree mesher (src/quad_mesh, src/utils/intersection.rs) ----
 * f64 throughout, as the reference.  Polygon construction, the geometry
 * predicates and the tesselation are host code; Mesh::from_quad_tree
 * (mesh.rs:51-227: leaf filtering, the O(n^2) face-neighbour search, the
 * cell/edge intersections) runs on the GPU.  Geometry calls return 0 / a
 * negative cfd_status like every entry point; the reference's PolygonError
 * comes back through *poly_error. */
typedef struct { double x, y; } cfd_point;                    /* point.rs */
typedef struct { cfd_point center; double half_width, half_height; } cfd_aabb;   /* aabb.rs */
enum { CFD_POLY_OK = 0, CFD_POLY_NOT_ENOUGH_VERTICES = 1, CFD_POLY_SELF_INTERSECTING = 2,
       CFD_POLY_INVALID_HOLE = 3 };                          /* PolygonError polygon.rs:12-16 */
typedef struct cfd_polygon cfd_polygon;
typedef struct cfd_quadtree cfd_quadtree;
typedef struct cfd_mesh cfd_mesh;

/* Polygon::new (polygon.rs:19-40): *out is NULL when *poly_error != 0. */
int cfd_polygon_new(const cfd_point *vertex_buffer, size_t n_points, const uint64_t *vertices,
                    size_t n_vertices, cfd_polygon **out, int *poly_error);
int cfd_polygon_new_rect(double x, double y, double w, double h, cfd_polygon **out); /* :42-53 */
int cfd_polygon_new_regular(cfd_point center, double radius, size_t n, double start_angle,
                            cfd_polygon **out);                                  /* new_polygon :55-67 */
/* add_hole (:69-79): on success the polygon takes ownership of `hole`. */
int cfd_polygon_add_hole(cfd_polygon *p, cfd_polygon *hole, int *poly_error);
/* contains_point (:81-103), intersects_aabb (:105-117), edges_intersect_aabb
 * (:119-133): *result 0 / 1. */
int cfd_polygon_contains_point(const cfd_polygon *p, cfd_point pt, int *result);
int cfd_polygon_intersects_aabb(const cfd_polygon *p, const cfd_aabb *box, int *result);
int cfd_polygon_edges_intersect_aabb(const cfd_polygon *p, const cfd_aabb *box, int *result);
int cfd_polygon_bounding_box(const cfd_polygon *p, cfd_aabb *out);               /* :150-178 */
int cfd_polygon_bounding_square(const cfd_polygon *p, cfd_aabb *out);            /* :180-184 */
/* edges (:186-196), reference quirk kept: edge k joins vertex_buffer[v_k] and
 * vertex_buffer[(v_k + 1) % n_vertices]; out gets 2 points per edge. */
int cfd_polygon_edges(const cfd_polygon *p, cfd_point *out, size_t max_edges, size_t *n_edges);
void cfd_polygon_destroy(cfd_polygon *p);

/* utils/intersection.rs: do_intersect (:20-38), line_segment_intersection
 * (:41-63; *found 0 for None), intersect_quad_edge (:68-129) for
 * quad = Quad::new_rect(center, hw, hh) (quad.rs:24-35; up to 8 points). */
int cfd_geom_do_intersect(cfd_point p, cfd_point q, cfd_point a, cfd_point b, int *result);
int cfd_geom_segment_intersection(cfd_point p, cfd_point q, cfd_point a, cfd_point b,
                                  cfd_point *out, int *found);
int cfd_geom_intersect_quad_edge(cfd_point center, double hw, double hh, cfd_point p1,
                                 cfd_point p2, cfd_point *out8, int *n);

/* tesselate (quad_tree.rs:17-100).  Nodes in depth-first pre-order; children
 * (4 per node, quadrant order of :43-91) as node indices, -1 for a leaf. */
int cfd_tesselate(const cfd_polygon *p, double feature_size, double max_cell_size,
                  cfd_quadtree **out);
int cfd_quadtree_size(const cfd_quadtree *t, uint64_t *n_nodes, uint64_t *n_leaves);
int cfd_quadtree_nodes(const cfd_quadtree *t, cfd_aabb *boxes, int64_t *children4);
void cfd_quadtree_destroy(cfd_quadtree *t);

/* Mesh::from_quad_tree (mesh.rs:51-227) on HIP device `device`.  Arrays as the
 * reference's SoA Mesh; neighbour lists of each cell in ascending cell order. */
enum { CFD_FACE_EAST = 0, CFD_FACE_WEST = 1, CFD_FACE_NORTH = 2, CFD_FACE_SOUTH = 3 };
int cfd_mesh_from_quadtree(const cfd_quadtree *t, const cfd_polygon *p, int device,
                           cfd_mesh **out);
/* sizes[0] cells, [1..4] neighbour index counts (east, west, north, south),
 * [5] intersection points. */
int cfd_mesh_sizes(const cfd_mesh *m, uint64_t *sizes6);
int cfd_mesh_cells(const cfd_mesh *m, double *cx, double *cy, double *hw, double *hh);
/* ranges: 2 x u64 (start, end) per cell. */
int cfd_mesh_neighbors(const cfd_mesh *m, int face, uint64_t *ranges, uint64_t *indexes);
int cfd_mesh_intersections(const cfd_mesh *m, uint64_t *ranges, cfd_point *points);
int cfd_mesh_full_bounding_box(const cfd_mesh *m, cfd_aabb *out);               /* :294-338 */
/* device time of the last cfd_mesh_from_quadtree's kernels (HIP events) */
int cfd_mesh_build_ms(const cfd_mesh *m, double *ms);
void cfd_mesh_destroy(cfd_mesh *m);

/* ---- the Mesh tab's images (src/utils/polygon_rasterizer.rs,
 * quad_tree_rasterizer.rs, mesh_rasterizer.rs, drawing.rs) ----
 * Drawn on HIP device `device`; only the w*h*4 bytes of the image leave it.
 * Part of the ABI:
 *   - RGBA8, 4 bytes per pixel, row-major, x fastest; row 0 is the reference's
 *     y = 0 (the reference does not flip, neither does this).
 *   - The colours are egui's Color32 constants as bytes:
 *       TRANSPARENT (0, 0, 0, 0)        BLACK  (0, 0, 0, 255)
 *       LIGHT_BLUE  (173, 216, 230, 255)   from_rgb(0xAD, 0xD8, 0xE6)
 *       ORANGE      (255, 165, 0, 255)     from_rgb(255, 165, 0)
 *   - The arithmetic is the reference's f64: scale = min((w - 1) / bbox.width(),
 *     (h - 1) / bbox.height()), pixel = floor((x - top_left.x) * scale) cast as
 *     each rasteriser casts it (`as usize` then `as isize` for the polygon and
 *     the quadtree: negatives and NaN give 0; straight `as isize` for the mesh:
 *     negatives stay and are clipped per pixel), draw_line and draw_diamond
 *     pixel for pixel, and the reference's drawing order (fill, polygon edges,
 *     cells in ascending index, each cell's outline before its diamonds).
 * Build-defined limits, checked on the host before any launch (the reference
 * has none: it would walk a far-off line for as long as it takes): w and h in
 * [2, 16384]; a finite bbox of positive width and height; every segment end
 * and diamond centre within [-32768, 32768] pixels; polygon holes without
 * holes of their own (as cfd_mesh_from_quadtree).  CFD_EINVAL for these and
 * for NULL handles or outputs, with nothing written.  device_ms may be NULL;
 * otherwise it receives the device time of the call's kernels (HIP events).
 * `background` and `rgba` are w*h*4 bytes and may be the same buffer. */
/* PolygonRasterizer::rasterize (polygon_rasterizer.rs:44-103) on the polygon's
 * own bounding box. */
int cfd_raster_polygon(const cfd_polygon *p, int device, size_t w, size_t h, uint8_t *rgba,
                       double *device_ms);
/* rasterize_quad_tree / rasterize_quad_tree_no_background
 * (quad_tree_rasterizer.rs:6-59).  NULL bbox: the tree's boundary; NULL
 * background: transparent. */
int cfd_raster_quadtree(const cfd_quadtree *t, const cfd_aabb *bbox, int device, size_t w, size_t h,
                        const uint8_t *background, uint8_t *rgba, double *device_ms);
/* rasterize_mesh / rasterize_mesh_no_background (mesh_rasterizer.rs:8-57).
 * bbox is required; NULL background: transparent.  A mesh of 0 cells gives
 * the background. */
int cfd_raster_mesh(const cfd_mesh *m, const cfd_aabb *bbox, int device, size_t w, size_t h,
                    const uint8_t *background, uint8_t *rgba, double *device_ms);
/* The first image of MeshView::draw_sketch (views/mesh_view.rs:86-94): the
 * polygon raster with the mesh (if any) over it, on the polygon's bounding
 * box, in one device pass. */
int cfd_raster_mesh_view(const cfd_polygon *p, const cfd_mesh *mesh_or_null, int device, size_t w,
                         size_t h, uint8_t *rgba, double *device_ms);
/* The image-size rule of views/mesh_view.rs:75-88: the available aspect is an
 * f32 division widened to f64, the sizes are truncated `as usize`.  Host only. */
int cfd_mesh_view_size(const cfd_aabb *bbox, float avail_w, float avail_h, size_t *w, size_t *h);

const char *cfd_last_error(void);
int cfd_abi_version(void);
void cfd_destroy(cfd_model *m);

#ifdef __cplusplus
}
#endif
#endif /* CFD_H */
