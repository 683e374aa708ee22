// cfd_internal.h — device-side data layout and kernel launch interface of the
// MI355X pressure-projection path.  Shared by the kernel units (cfd_device.h
// and every csrc/*.hip that holds kernels) and by cfd_model.h /
// cfd_model_*.hip (host runtime behind include/cfd.h).
//
// Layout in HBM (one slab per GPU; a single-GPU model is the 1-slab case):
//   every field is row-major with x fastest and the reference's pitches
//   (u: nx+1, v: nx, p/rhs/p': nx — model.rs:161-214), so the reference's
//   flat wrap-around reads (U(nx+1,j) == U(0,j+1)) are plain loads here.
//   "local row" lj = global row j - j0.  Base pointers point at local row 0;
//   ghost rows sit at negative lj and at lj >= nyl:
//     u, u_old, u_star : rows [-G, nyl+G)        (G = 2)
//     v, v_old, v_star : rows [-G, nyl+1+G)      (v row nyl is the face shared
//                                                 with the rank above)
//     p                : rows [0, nyl)
//     rhs, p' (x2)     : rows [-HG, nyl+HG)      (HG = halo depth >= 1; deep-halo
//                                                 sweeps recompute ghost rows)
//   mask_u rows [0,nyl), mask_v rows [0,nyl] (u8, same pitches).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/cfd.h"

namespace cfd {

// Calls f with the division mode (Geom::fastdiv: 1, 2, anything else 0) as a
// std::integral_constant, so a generic lambda can name the kernel
// instantiation (k<T, F()>); returns what f returns.
template <class Fn>
auto with_fastdiv(int fastdiv, Fn &&f) {
    if (fastdiv == 1) return f(std::integral_constant<int, 1>{});
    if (fastdiv == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 0>{});
}

constexpr int kGhostUV = 2;
// thresholds of the fma form's bounds (Ctl::sums_m0 / sums_rm): R max|p'| <=
// 2^122 and 0.1875 kMaxSweeps max|rhs| <= 768 * 2^112 < 2^122 keep the guard's
// sum below its 2^123
constexpr float kSumsPLim = 0x1p122f, kSumsRLim = 0x1p112f;
constexpr int kMaxSweeps = 4096;   // per pressure solve
constexpr int kMaxPasses = 64;     // corrector passes + 1

// Residual maxima are published with atomicMax on f32 bits.  Device-scope
// atomics on ONE address serialise at the memory side (~10 ns each, measured:
// 6,000 per launch cost 54 us), so every maximum is spread over kResSlots
// addresses kResStride words apart and folded by its reader (fold_res /
// read_res).  Sweep k of a solve owns slots err_slots[(k*kResSlots + s)*kResStride];
// the 4 step maxima own red_slots likewise.  Slots are zero between uses.
constexpr int kResSlots = 32;
constexpr int kResStride = 16;
// persistent-solve words (k_jacobi_persist), one 64-B line each: line 0 [1]
// the abort flag, [2] the blocks stolen so far, [3] the blocks run in the
// SUMS form so far; then one line per tile: [0] its done flag, [1] its claim
// counter, [2..5] / [6..9] its waves' max |p'| stored in its last even / odd
// block
constexpr int kPersistFlagStride = 16;
// head lines: 0 = the persistent solve's words ([1] abort, [2] steals, [3]
// SUMS blocks); 2 = the resident solve's top barrier counter, 4 = its exit
// ticket, 5-12 its group counters, 13-20 its group generations
// (cfd_jacobi_resident.hip)
constexpr int kPersistHeadLines = 21;
// flag = epoch << kPersistBlockBits | blocks done: room for every block of the
// longest solve (kMaxSweeps / 8 = 512), epochs below 2^(32 - bits)
constexpr int kPersistBlockBits = 10;
static_assert((1 << kPersistBlockBits) > kMaxSweeps / 8, "persistent flag layout");
constexpr int kPersistMaxGroups = 16384;   // tiles (wave columns x row groups)
constexpr size_t kPersistWords = (size_t)(kPersistMaxGroups + kPersistHeadLines) * kPersistFlagStride;
// slot sets: kMaxSweeps per-sweep residual sets, then red (4), vis (2), 10
// spare; then the persistent solve's words
constexpr size_t kSlotWords = (size_t)(kMaxSweeps + 16) * kResSlots * kResStride + kPersistWords;

// Device-resident control block: every data-dependent decision of
// Model::update lives here so a whole step can be enqueued (or replayed as a
// hipGraph) with no host round trip.
struct Ctl {
    float dt;               // Model::dt (model.rs:170)
    float time;             // simulation_time
    uint32_t step;          // simulation_step
    float inlet;            // current_inlet_velocity (set at step start)
    int32_t cur;            // which p' buffer holds the current p'
    uint32_t n_exec_last;   // sweeps executed by the last solve
    float last_p;           // last_pressure_residual
    float res_u, res_v;     // last_u_residual / last_v_residual
    uint32_t red[7];        // step maxima as f32 bits: |du|, |dv|, |u|, |v|; red[6]: a
                            // persistent solve of some slab timed out (r5, all-reduced so
                            // every rank recovers); red[5]: the last
                            // solve's residual (all-reduced with the maxima on slabs); red[4]:
                            // non-finite flag (1: some new u/v value is NaN or +-Inf)
    uint32_t nonfinite_step;   // sticky: simulation_step after the first step whose
                               // velocities were not all finite (0 = never)
    uint32_t vis[2];        // render: max key, max ~key of the derived field (cfd_render.hip)
    // The fma form of the per-launch march (LdsMarch SUMS == 2) and its
    // whole-solve guard.  sums_m0 / sums_rm are upper bounds of max |p'| /
    // max |rhs| (bits & 0x7fffffff): the publishing kernel raises the word to
    // a fixed threshold (kSumsPLim / R, kSumsRLim: together they pass the
    // guard) and only a lane that holds a larger value raises it further, so
    // the usual launch issues ONE atomic.  sums_state: 0 the bounds describe
    // nothing a solve may rely on; 1 the corrector finish bounded the p' the
    // next step's solve starts from in sums_m0 and zeroed sums_rm; 2 the
    // predictor march then bounded the rhs it formed in sums_rm.  Only
    // a solve that finds 2 may take the form; every k_finalize_solve (and the
    // resident solve's own) returns to 0 and zeroes sums_m0, and every host
    // call that can change p' or rhs outside a step returns to 0.
    uint32_t sums_state;
    uint64_t sweeps_total;
    // speculative temporal blocking with the tolerance on (k_spec_check):
    // spec_stop: a launch of this solve converged (later launches skip);
    // spec_launch / spec_redo: that launch and the stages its re-run keeps
    // (0: none, it converged on its last stage); spec_launches: launches run
    // (the finalize's buffer flips).  All 0 between solves.
    int32_t spec_stop, spec_redo, spec_launch, spec_launches;
    uint32_t sums_launches; // per-launch marches that ran the fma form (diagnostics)
    uint32_t sums_m0, sums_rm;   // max |p'| / max |rhs| as bits & 0x7fffffff (NaN, Inf: above every finite)
    int32_t go[kMaxPasses + 1];      // go[p]: pass p of the corrector loop runs
    uint32_t err[kMaxSweeps];        // per-sweep max |p'new - p'| as f32 bits
    // the script's double of last_p (cfd_script_options.residual_f64; solvers
    // 2, 4 and 5): the residual of the last iteration run, whose f32 rounding
    // is last_p.  Written by k_publish_f64 behind the solve's finalize.
    double last_p64;
    // dt of the last uv-fused step (k_predict_march MODE 2), for the launch
    // that materialises its u*, v* on demand (cfd_model::need_star)
    float star_dt;
};

// The double residual's spread maxima (cfd_script_options.residual_f64): a
// non-negative double orders as its 64 bits, so iteration k of a solve owns
// kResSlots 64-bit words res64[(k * kResSlots + s) * kRes64Stride], one 64-byte
// line each, raised with 64-bit atomicMax.  Zero between solves; allocated
// when the option is switched on, released when it is switched off.
constexpr int kRes64Stride = 8;
constexpr size_t kRes64Words = (size_t)kMaxSweeps * kResSlots * kRes64Stride;

// Scalars every kernel needs; passed by value as a kernel argument.
struct Geom {
    int32_t nx, ny;       // global pressure cells
    int32_t j0, nyl;      // global row of local row 0; owned rows
    int32_t hg;           // p' halo depth
    float dx, dy, nu, ly;
    float target_inlet;
    int32_t scheme, profile, bc_kind;
    int32_t tol_enabled;
    float p_tol;
    int32_t jacobi_iters;
    // Jacobi divisors exactly as model.rs:740-746 forms them, their rounded
    // reciprocals, and the division mode proven exact for all three
    // (0: IEEE `/`, 1: x * (1/c), 2: x * (1/c) + one FMA correction step);
    // see choose_division() in cfd_model_build.hip.
    float dx_sq, dy_sq, denom;
    float r_dx_sq, r_dy_sq, r_denom;
    int32_t fastdiv;
    int32_t tb_rows;      // fixed output rows per wave segment (0: balanced by tb_bpc)
    int32_t tb_bpc;       // target k_jacobi_tb blocks per CU (balanced segmentation)
    int32_t n_cu;         // compute units of the device
    int32_t tb_kind;      // 1: k_jacobi_tb (T <= 4); 4: the prefetch pipeline (T <= 8,
                          // 2 columns per lane, k_jacobi_pipe); 5: the same march
                          // with its rhs window in LDS (k_jacobi_lds)
    int32_t xcd_remap;    // renumber blocks so each XCD gets contiguous tiles (xcd_block)
    // reciprocals of dx, dy, dx*dx, dy*dy; sp_pow2 = 1 when all four spacings
    // are exact powers of two (then sdiv multiplies, bit-identically)
    float r_dx, r_dy, r_dxx, r_dyy;
    int32_t sp_pow2;
    int32_t pred_div;     // predictors + divergence: 2: one row march (k_predict_march, both
                          // schemes) where it applies, 0: separate launches
    int32_t res_div;      // r4: the resident solve's division mode: fastdiv, or 3 (FMA-corrected
                          // above 2^-96, IEEE below; proven like the others) where fastdiv is 0
};

struct Fields {
    float *u, *v, *u_old, *v_old, *u_star, *v_star;   // at local row 0
    float *p, *rhs;
    float *pp[2];                                      // p' ping-pong
    const uint8_t *mask_u, *mask_v;
    const int32_t *obs;       // (i, j_global) pairs, cells touching this slab
    uint32_t *err_slots;      // spread per-sweep residual maxima (kResSlots per sweep)
    uint32_t *red_slots;      // spread step maxima (4 x kResSlots)
    uint32_t *vis_slots;      // spread render min/max keys (2 x kResSlots)
    int32_t n_obs;
    int32_t any_pmask;   // some predictor mask bit (bit 0) is set in this slab's masks
    size_t u_alloc, v_alloc;  // floats in the u/v allocations (incl. ghosts)
    float *u_alloc_base, *v_alloc_base, *u_old_base, *v_old_base, *u_star_base, *v_star_base;
    Ctl *ctl;
    // host-mapped word (pinned, zero-copy) mirroring Ctl::nonfinite_step, so the
    // host can see a blown-up run without synchronising the stream
    uint32_t *host_nonfinite;
    // host-mapped word the step finalize sets to Ctl::step (sharded models):
    // the RCCL watchdog's evidence of forward progress
    uint32_t *host_progress;
    uint32_t *persist;   // kPersistWords words after the slot sets (see kPersistFlagStride)
    // the fma form of the per-launch march can run for this model at all (one
    // domain, Jacobi with a fixed count, a grid that allows the form, knob
    // on): only then do the corrector finish and the predictor march keep
    // Ctl::sums_state and its bounds; 0: they skip that bookkeeping entirely,
    // sums_state stays 0 and every launch runs the reference's body
    int32_t sums_track;
};

// The float4 rows of the vector kernels: 16-byte aligned.  An invariant of
// build_model (every field base is a hipMalloc base plus whole rows of nx
// floats, nx % 8 == 0), which refuses a model that breaks it.
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// ---- step kernels (cfd_kernels.hip; the predictor march cfd_predict_march.hip,
// the blocked Jacobi marches cfd_jacobi_*.hip) ----
// pass < 0 means "not inside the corrector loop" (always runs).
void launch_step_begin(const Geom &g, const Fields &f, int copy, hipStream_t s);
void launch_copy_star(const Geom &g, const Fields &f, int pass, hipStream_t s);
// k_copy_star + k_divergence of a corrector pass in one launch (same values).
void launch_copy_star_div(const Geom &g, const Fields &f, int pass, float dt_override,
                          hipStream_t s);
void launch_u_predictor(const Geom &g, const Fields &f, float dt_override, hipStream_t s);
void launch_v_predictor(const Geom &g, const Fields &f, float dt_override, hipStream_t s);
// u and v predictors in one pass (same results as the two launches above);
// vec (cfd_options::pred_vec): the first-order scheme's four-column form.
void launch_predict(const Geom &g, const Fields &f, float dt_override, bool vec, hipStream_t s);
// both schemes' predictors + divergence in one row march (cfd_predict_march.hip),
// when predict_march_ok(): replaces launch_predict + the step's first divergence
bool predict_march_ok(const Geom &g, const Fields &f);
int predict_march_workgroups(const Geom &g);
// set_inlet: also set Ctl::inlet from Ctl::step (k_step_begin's ramp,
// model.rs:311-316) — the step's k_step_begin is then not launched
// [row_lo, row_hi): the divergence rows the launch forms (>= 4 rows; default
// all owned rows) — a sharded step runs rows [2, nyl-2), which read no u/v
// ghost row, while the ghost exchange is in flight
// mode (the uv-fused fixed-count step, cfd_options::uv_fused; one domain,
// all owned rows): 1 stores rhs only; 2 is the corrector finish on the same
// march after the solve -- it forms u*, v* again from f.u / f.v and stores the
// new u, v into f.u_old / f.v_old (the caller then swaps the pairs), p += p',
// the step maxima, Ctl::star_dt.  star (mode 0): f.u / f.v are that step's old
// pair; store the u*, v* it never stored (dt = Ctl::star_dt), rhs stays.
void launch_predict_march(const Geom &g, const Fields &f, float dt_override, hipStream_t s,
                          bool set_inlet = false, int row_lo = 0, int row_hi = -1, int mode = 0,
                          bool star = false);
void launch_divergence(const Geom &g, const Fields &f, int pass, float dt_override,
                       hipStream_t s);
// One Jacobi sweep over local rows [row_lo, row_hi) (may reach into ghosts).
// res: publish this sweep's residual (always with the tolerance on; only the
// last sweep of a fixed-count solve needs it).
void launch_jacobi_sweep(const Geom &g, const Fields &f, int pass, int it, int row_lo,
                         int row_hi, int res, hipStream_t s);
// T consecutive Jacobi sweeps in one launch (temporal blocking, tolerance
// off): the final sweep's rows [out_lo, out_hi) are stored; sweep `it` of the
// block is the first.  T <= kMaxTemporal.
// `par` = launches of this solve before this one (selects the source buffer:
// buffers flip once per launch).
void launch_jacobi_block(const Geom &g, const Fields &f, int pass, int it, int par, int T,
                         int out_lo, int out_hi, int res, hipStream_t s);
// nblk consecutive 8-sweep kind-5 blocks (no residual) in ONE persistent
// launch whose workgroups hand rows to their neighbours through flags
// (k_jacobi_persist); res_it >= 0: the last block is the solve's last and
// publishes sweep res_it's residual; returns false (nothing launched) where
// the one-round geometry does not apply
bool launch_jacobi_persist(const Geom &g, const Fields &f, int pass, int par0, int nblk,
                           int out_lo, int out_hi, uint32_t epoch, int res_it, hipStream_t s);
// The tile geometry of the T = 8 kind-5 launch over rows [out_lo, out_hi)
// (persist: the persistent form's): dynamic LDS pad, workgroups per CU the
// round is sized for, wave columns, wave segments per column
// (cfd_jacobi_lds8.hip, from the launches' own lds_tiles, cfd_jacobi_lds.hip).
void lds_geometry8(const Geom &g, int out_lo, int out_hi, bool persist, int *pad, int *occ, int *nwc,
                   int *nseg);
// The block kernels behind it: k_jacobi_tb (kind 1, T <= 4, cfd_jacobi_tb1.hip)
// and the prefetch-pipelined march, 2 columns per lane (kind 4, T <= 8,
// cfd_jacobi_pipe.hip).
// res_slots: the slot set the last sweep's residual goes to, or null.
void launch_tb1(const Geom &g, const Fields &f, int T, int pass, int it, int par, int out_lo,
                int out_hi, uint32_t *res_slots, hipStream_t s);
void launch_pipe(const Geom &g, const Fields &f, int T, int pass, int it, int par, int out_lo,
                 int out_hi, uint32_t *res_slots, hipStream_t s);
// kind 5: the same march with its rhs window in LDS: its persistent form
// (cfd_jacobi_lds_persist.hip, T = 8) and its per-launch form
// (cfd_jacobi_lds.hip, T <= 8); mode 2 / 3: the speculative launch / its re-run
// (launch_jacobi_spec)
bool launch_lds_persist8(const Geom &g, const Fields &f, int pass, int par0, int nblk, int out_lo,
                         int out_hi, uint32_t epoch, uint32_t *rs, hipStream_t s);
// lag (r5, speculative solves on one domain): mode 2 -- the previous launch's
// sweep count, whose early-exit check this launch makes (0: none); mode 3 --
// the solve's last launch's, checked by the re-run (see k_jacobi_lds)
void launch_lds(const Geom &g, const Fields &f, int T, int pass, int it, int par, int out_lo,
                int out_hi, uint32_t *res_slots, hipStream_t s, int mode = 0, int lag = 0);
// Speculative temporal blocking for the tolerance mode (model.rs:748-819):
// the launch starting at sweep `it` runs T sweeps (kind 5) and publishes
// every sweep's residual; k_spec_check folds them, finds the first sweep
// below p_tol and, when it is not the launch's last, schedules the re-run
// (launch_jacobi_redo) of that launch with exactly that many sweeps from its
// untouched source buffer.  Later launches of the solve return at once.
// lag > 0 (one domain, the default since r6; CFD_SPEC_LAG=0 turns it off): no k_spec_check launches -- each launch checks the
// previous one (lag = its sweep count) and the re-run checks the last one
// (launch_jacobi_redo's last_*); see spec_lag_first.
void launch_jacobi_spec(const Geom &g, const Fields &f, int pass, int it, int par, int T,
                        int out_lo, int out_hi, hipStream_t s, int lag = 0);
void launch_spec_check(const Geom &g, const Fields &f, int pass, int it, int T, int par,
                       hipStream_t s);
// The whole tolerance-mode solve of a single-domain grid in one launch
// (cfd_jacobi_resident.hip); false: no tile plan fits (nothing launched).
// fin: its last workgroup also runs k_finalize_solve's body (exact_flips 2).
bool launch_jacobi_resident(const Geom &g, const Fields &f, int pass, int iters, int fin,
                            int check_break, hipStream_t s);
bool jacobi_resident_geometry(const Geom &g, int *br, int *bc, int *tiles, int *wgs);
// slabs (r5): after the re-run, the converged launch's result moved to the
// buffer the host counts n launches ahead (k_spec_align; nyl * nx % 4 == 0)
void launch_spec_align(const Geom &g, const Fields &f, int pass, int n, hipStream_t s);
void launch_jacobi_redo(const Geom &g, const Fields &f, int pass, int out_lo, int out_hi,
                        hipStream_t s, int last_it = 0, int last_par = 0, int last_T = 0);
// dst[q] = max(dst[q], slots of q) for q < n, then zero those slots (before
// an all-reduce of dst reads it).
void launch_fold_slots(uint32_t *dst, uint32_t *slots, int n, hipStream_t s);
// Visualisation (cfd_render.hip, src/app.rs:235-403): derived field of `mode`
// into `out` (may be null) with its min/max keys into 2 spread sets; then the
// RGBA8 image from the folded keys (field null: re-derive on the fly).
void launch_vis_field(const Geom &g, const Fields &f, int mode, float *out, uint32_t *slots,
                      hipStream_t s);
void launch_vis_color(const Geom &g, const Fields &f, int mode, const float *field, uint32_t *px,
                      const uint32_t *keys, int has_cyl, float cx, float cy, float radius,
                      hipStream_t s);
// Exhaustive check over all 2^32 f32 inputs x of x/c against the two fast
// forms; writes mismatch counts {mode1, mode2} to dev_counts (2 x u64).
void launch_verify_division(float c, float r, unsigned long long *dev_counts, hipStream_t s);
// flips = launches of a fixed-count solve (ignored with the tolerance on,
// where each executed sweep is one launch).  exact_flips: flip the current
// p' buffer exactly `flips` times regardless of the tolerance (solvers that
// work in place: SOR, multigrid); 2: Ctl::spec_launches times (speculative
// solve), and reset the speculative state.
void launch_finalize_solve(const Geom &g, const Fields &f, int pass, int iters, int check_break,
                           int flips, hipStream_t s, int exact_flips = 0);

// ---- alternative pressure solvers (cfd_solvers.hip; index.html) ----
// Double-precision constants of one grid level: dx2 = dx*dx, dy2 = dy*dy,
// denom = 2/dx2 + 2/dy2 exactly as the script forms them, their reciprocals,
// and fast = 1 when all three divisors are powers of two (x / c == x * (1/c)
// bit for bit for every double x).
struct SorConst {
    double dx2, dy2, denom;
    double r_dx2, r_dy2, r_denom;
    int32_t fast;
};
// One multigrid level: solution ping-pong buffers a/b (level 0: the model's
// current / other p' buffer), right-hand side, residual scratch, size and the
// level's constants (spacing 2^l times the model's, index.html:1458).
struct MgLevel {
    // biased to global row 0: element (i, j) of the level is a[j * nx + i]
    // for every stored row j in [ys, ye)
    float *a, *b, *rhs, *r;
    int32_t nx, ny;        // the level's global size
    double dx2, dy2, denom;
    double r_dx2, r_dy2, r_denom;
    int32_t fast;
    int32_t ys, ye;        // stored rows (a slab's rows + ghost rows; 0, ny unsharded)
    int32_t lo, hi;        // rows a launch outputs (set per launch; 0, ny unsharded)
};
constexpr int kMgMaxLevels = 40;
void launch_sor_color(float *pp, const float *rhs, int nx, int ny, const SorConst &k, int color,
                      Ctl *ctl, uint32_t *err_slots, int pass, int it, int tol, float p_tol, int res,
                      hipStream_t s);
// One whole red-black iteration per launch (k_sor_march) over the local
// interior rows [row_lo, row_hi) of a slab starting at global row j0 (p' and
// rhs rows readable in [lo_clamp, hi_clamp]), ping-pong between pa / pb from
// ctl->cur (iteration `it` reads buffer (cur + it) & 1; it = 0 reads nothing:
// p' starts at 0), when sor_fused_ok(nx, row_hi - row_lo).
bool sor_fused_ok(int nx, int nrows);
void launch_sor_fused(float *pa, float *pb, const float *rhs, int nx, int ny, const SorConst &k,
                      Ctl *ctl, uint32_t *err_slots, int pass, int it, int tol, float p_tol, int res,
                      int row_lo, int row_hi, int j0, int lo_clamp, int hi_clamp, hipStream_t s);
void launch_fill_zero(float *p, size_t n, const Ctl *ctl, int pass, hipStream_t s);
// SOR in the script's own order (cfd_sor_lex.hip, pressure_solver 4): the
// whole solve as one launch of (iteration, 64-row band) tasks handed out by a
// ticket counter, plus, with the tolerance on, a replay launch that returns
// at once unless iterations had run past the early exit.  Iteration k reads
// buffer (ctl->cur + k) & 1 and writes the other (k = 0 reads nothing), and
// folds its max |new - old| into ctl->err[k]: the caller's finalize flips the
// buffer once per iteration run.  pol: sor_lex_words(iters, ny) words the
// launcher zeroes before each launch; exitw: 4 words.  iters >= 1.
size_t sor_lex_words(int iters, int ny);
// res64 (both solvers below and launch_mg_final_residual): null, or the double
// residual's slot sets -- the launch then runs the kernel's second
// instantiation, which folds the maximum as a double, raises set k of res64
// with it and derives the f32 it publishes as before from that double.
hipError_t launch_sor_lex(float *pa, float *pb, const float *rhs, int nx, int ny, const SorConst &k,
                          Ctl *ctl, uint32_t *pol, uint32_t *exitw, uint32_t *host_fail, int pass,
                          int iters, int tol, float p_tol, int n_cu, int *launches, hipStream_t s,
                          unsigned long long *res64 = nullptr);
// The script's Jacobi, omega 0.7 (cfd_jacobi_script.hip, pressure_solver 5):
// one whole iteration per launch -- interior update, max |new - old| into
// err_slots' set `it`, boundary copies -- ping-pong between pa / pb from
// ctl->cur exactly as launch_sor_fused (it = 0 reads nothing); with tol the
// launch returns at once when iteration it - 1 fell below p_tol.  nx even,
// ny >= 3, whole domain.
void launch_jacobi_script(float *pa, float *pb, const float *rhs, int nx, int ny, const SorConst &k,
                          Ctl *ctl, uint32_t *err_slots, int pass, int it, int tol, float p_tol,
                          int res, hipStream_t s, unsigned long long *res64 = nullptr);
// Behind the finalize of a solve that raised res64: Ctl::last_p64 = the
// maximum of set n_exec_last - 1 (0.0 when no iteration ran), then the sets the
// solve can have raised are zeroed again: [z_lo, iters), or with to_n
// [z_lo, n_exec_last).
void launch_publish_f64(const Fields &f, unsigned long long *res64, int pass, int iters, int z_lo,
                        int to_n, hipStream_t s);
void launch_mg_smooth(const MgLevel &L, const float *src, float *dst, const Ctl *ctl, int pass,
                      hipStream_t s);
// Five smoothing sweeps src -> dst in one launch (temporal blocking: one
// wave per register window, or the LDS block form with CFD_MG_SMOOTH=1).
void launch_mg_smooth5(const MgLevel &L, const float *src, float *dst, const Ctl *ctl, int pass,
                       hipStream_t s);
// The wave-window form is selected (then the up-leg fuses its prolong-add
// into the smoothing: launch_mg_prolong_smooth5 reads src + prolongate(e)).
bool mg_smooth_wave_form();
void launch_mg_prolong_smooth5(const MgLevel &Cl, const float *e, const MgLevel &L, const float *src,
                               float *dst, const Ctl *ctl, int pass, hipStream_t s);
// ... and the down-leg forms the residual of its smoothed field in the same
// launch (launch_mg_smooth5_residual: dst and L.r).
void launch_mg_smooth5_residual(const MgLevel &L, const float *src, float *dst, const Ctl *ctl,
                                int pass, hipStream_t s);
void launch_mg_residual(const MgLevel &L, const float *p, const Ctl *ctl, int pass, hipStream_t s);
void launch_mg_restrict(const MgLevel &F, const MgLevel &Cl, const Ctl *ctl, int pass, hipStream_t s);
void launch_mg_prolong_add(const MgLevel &Cl, const float *e, const MgLevel &F, float *p,
                           const Ctl *ctl, int pass, hipStream_t s);
// fast: the hierarchy's division form (uniform: 2^l scaling keeps powers of two)
void launch_mg_tail(const MgLevel *dev_levels, int s_level, int coarsest, float *a0, float *b0,
                    int fast, const Ctl *ctl, int pass, hipStream_t s);
void launch_mg_final_residual(const MgLevel &L, const float *p, uint32_t *slots, const Ctl *ctl,
                              int pass, hipStream_t s, unsigned long long *res64 = nullptr);
// ---- velocity boundaries, step reduce and finalize (cfd_kernels.hip) ----
void launch_boundary(const Geom &g, const Fields &f, hipStream_t s);
void launch_step_reduce(const Geom &g, const Fields &f, hipStream_t s);
void launch_step_finalize(const Geom &g, const Fields &f, hipStream_t s);
// Slabs with persistent runs (r5): copy this rank's abort word (persist[1],
// a persistent solve timed out) into Ctl::red[6] before the step all-reduce
void launch_abort_to_red(const Fields &f, hipStream_t s);
// ... and, after its all-reduce outside a step, back into this rank's abort
// flag and host word (as the step finalize does)
void launch_abort_from_red(const Fields &f, hipStream_t s);

// ---- correctors (cfd_correct.hip) ----
// apply_corrector as its own launch; vec (cfd_options::corr_vec): four cells
// per thread, else the one-float-per-thread kernel.
void launch_corrector(const Geom &g, const Fields &f, int pass, float dt_override, bool vec,
                      hipStream_t s);
// The corrector finish (corrector + boundaries + step maxima): the band march
// of k_correct_finish4m.
void launch_correct_finish(const Geom &g, const Fields &f, float dt_override, hipStream_t s);
// max |p'| bound of the fma form's guard after a step with corrector passes
// (k_correct_finish4m publishes it itself); Fields::sums_track only
void launch_publish_sums_m0(const Geom &g, const Fields &f, hipStream_t s);
// The corrector of pass `pass` and, when pass+1 exists (has_next) and the
// device's go flag says it runs, pass+1's head (u* <- u, v* <- v,
// divergence) in one launch (k_correct_head4, single domain; every pass of the
// loop uses it: the passes alternate the u* / v* arrays, and u / v are
// written only when the loop ends); correct_head_ok: its alignment (the
// caller also asks cfd_options::corr_head).
bool correct_head_ok(const Geom &g, const Fields &f);
void launch_correct_head(const Geom &g, const Fields &f, int pass, float dt_override, bool has_next,
                         hipStream_t s);

// ---- tracer particles (cfd_tracers.hip; index.html:1472-1543) ----
// The script's ordered list {x, y, initialY} as three f64 arrays in two buffers
// (the compaction writes the other one), with every word that decides a
// launch on the device: a tracer step is the same two launches every step.
constexpr int kTrcBlock = 256;   // workgroup = tile of the stable compaction
struct TrcCtl {
    uint32_t count;      // tracers in buffer `cur`
    uint32_t overflow;   // sticky: an injection did not fit the capacity
    uint32_t cur;        // buffer that holds the list
    // written by the advect launch's last workgroup, read by the scatter
    // launch (which writes count / cur: no launch reads a word it writes)
    uint32_t n_prev, src, total, do_inject;
    uint32_t ticket;     // workgroups of the advect launch that have finished
};
struct Tracers {
    double *x0, *y0, *i0, *x1, *y1, *i1;   // buffers 0 and 1: x, y, initialY
    TrcCtl *tc;
    uint32_t *tile_cnt, *tile_off;   // survivors per tile of kTrcBlock, their exclusive scan
    uint32_t cap;
    uint32_t interval;    // inject when Ctl::step % interval == 0
    double dx, dy, lx, ly;   // the model's f32 values widened, as the script's doubles
};
// One updateTracers on the current u, v and the compaction (two launches of
// `grid` workgroups).  in_step: dt and the injection cadence come from Ctl
// (after the step finalize); else dt is `dt` and nothing is injected.
void launch_trc_step(const Geom &g, const Fields &f, const Tracers &t, int grid, bool in_step,
                     double dt, hipStream_t s);
// injectTracers: ny tracers appended in place (one workgroup), or the overflow word
void launch_trc_inject(const Geom &g, const Tracers &t, hipStream_t s);
// tracers per pressure cell into counts (nx*ny words, zeroed by the caller)
void launch_trc_density(const Geom &g, const Tracers &t, int grid, uint32_t *counts, hipStream_t s);

// ---- the script's substep (cfd_script_step.hip; index.html:366-930) ----
// The script's doubles as the model's f32 values widened, dx*dx and dy*dy as
// the script forms them, and their reciprocals; fast = 1 when dx, dy, dx*dx
// and dy*dy are all powers of two (x / c == x * (1/c) bit for bit).  obs_u /
// obs_v: per row of u faces (ny rows) / v faces (ny+1 rows) the half-open
// column interval [lo, hi) of isPointInObstacle at the face's own position
// (0, 0: none); inlet: the ny values the boundary pass stores into u(0, j).
struct ScriptStep {
    double dx, dy, dxx, dyy, nu, dt;
    double r_dx, r_dy, r_dxx, r_dyy;
    const int32_t *obs_u, *obs_v;
    const float *inlet;
    int32_t fast;
};
// one domain, nx % 4 == 0, ny >= 4, u / v allocations under 2 GiB (buffer loads)
bool script_step_ok(const Geom &g, const Fields &f);
// u*, v*, rhs from u, v (:368-739) in one row march; scheme: CFD_SCRIPT_*
void launch_script_predict(const Geom &g, const Fields &f, const ScriptStep &k, int scheme,
                           hipStream_t s);
// u, v from u*, v* and the current p', p += p', then the boundary pass (:842-866, :870-930)
void launch_script_correct(const Geom &g, const Fields &f, const ScriptStep &k, hipStream_t s);

// ---- one updateSimulation() around the substeps (cfd_script_update.hip;
// index.html:261-363) ----
// The step's reduction block, 64-bit words: three spread maxima of doubles as
// their bits (max |u - uOld|, max |v - vOld|, max(|u|, |v|); kResSlots slots
// each, one 64-byte line per slot), then one line whose first f32 is the
// running maximum of the substeps' pressure residuals and whose second 64-bit
// word is the running maximum of their doubles (k_script_pmax64, when the
// solves publish Ctl::last_p64).  Zeroed by the host (in stream order) when a
// step starts, read back once when it ends.
constexpr int kScrRedStride = 8;
constexpr int kScrRedPmax = 3 * kResSlots * kScrRedStride;
constexpr int kScrRedWords = kScrRedPmax + kScrRedStride;
// nu, nv: elements of u and v (one domain: contiguous from local row 0)
void launch_script_begin(const Fields &f, float *u_prev, float *u_old, float *v_prev, float *v_old,
                         long nu, long nv, int extrapolate, hipStream_t s);
void launch_script_pmax(const Fields &f, unsigned long long *red, hipStream_t s);
void launch_script_pmax64(const Fields &f, unsigned long long *red, hipStream_t s);
void launch_script_end(const Fields &f, float *u_prev, const float *u_old, float *v_prev,
                       const float *v_old, long nu, long nv, unsigned long long *red, hipStream_t s);

// Jacobi kernel geometry (exported for the roofline bookkeeping in bench).
constexpr int kJacRowsPerWave = 16;
constexpr int kMaxTemporal = 8;     // most sweeps per temporally blocked launch (kind 1: 4)
constexpr int kJacWavesPerBlock = 4;

}  // namespace cfd
