// cfd_jacobi_lds.h — kind 5: the temporally blocked Jacobi march
// (model.rs:748-815, T sweeps per launch) with its rhs window in LDS.
// Included by the translation units that instantiate it for disjoint sets
// of T (cfd_jacobi_lds.hip: T <= 4, the dispatch and the host-side tile
// geometry; cfd_jacobi_lds567.hip; cfd_jacobi_lds8.hip), so the kind's compile
// runs in parallel, and by cfd_jacobi_lds_persist.hip, whose persistent kernel
// runs the same block (lds_block) once per task.
//
// Same schedule as the prefetch-pipelined march (cfd_jacobi_pipe.hip): a wave
// owns 64 lanes x 2 columns of a row segment and marches along it; stage s
// (1..T) of slot v computes row k-s (k = k_first + v) from stage s-1's rows
// k-s-1..k-s+1, so every stage is one sweep of the reference, bit for bit.
// What changes is where each value lives between its load and its last use:
//   PQ[v % PD]  p' input row k+PD, loaded PD slots ahead       (registers)
//   RQ[v % PD]  rhs row k+PD, loaded PD slots ahead            (registers)
//   ring[v % D] rhs row k, written at slot v, read by stage s  (LDS, D >= T+1)
//               at slot v+s
//   W[s][v % 3] the newest row of stage s                      (registers)
// The march kind 4 keeps all T+PD rhs rows a slot needs in registers: ~130
// VGPRs at T = 8, 3 waves per SIMD.  Here the rhs window costs one
// ds_write_b64 and T ds_read_b64 per slot instead, and the kernel fits 8 waves
// per SIMD (~60 VGPRs, 4.5 KB of LDS per wave at T = 8).  The slot loop is
// unrolled by U = D (a multiple of 3 and of PD), so every ring index — W, PQ,
// RQ and the LDS slot, an immediate offset — is a compile-time constant.
//
// The horizontal neighbour sums are written as two scalar adds whose second
// operand is a DPP lane shift (wave_shr:1 / wave_shl:1): the backend folds
// each shift into its add (v_add_f32_dpp), one VALU instruction per sum.  The
// kind-5 units are built with -fno-slp-vectorize so the two adds are not
// packed back into a v_pk_add_f32 (VOP3P cannot take DPP); the rest of the
// update is explicit packed f32 arithmetic on column pairs.
#pragma once
#include <cmath>
#include <type_traits>

#include "cfd_device.h"

// Build-time constants of the march, each with the A/B that set it.  A variant
// build of one unit (tools/build_variants.sh) overrides them with -D.
#ifndef CFD_LDS_PD
#define CFD_LDS_PD 3        // prefetch distance (slots) of the p' and rhs rows; 4: 5.07 vs 4.95 us/sweep (r6 abvar_kvar.log)
#endif
#ifndef CFD_LDS_SPLIT
#define CFD_LDS_SPLIT 1     // stage groups per slot (LdsMarch::G); 2: 5.25 vs 4.95 us/sweep (r6 prof_r6c/abvar_kvar.log)
#endif
#ifndef CFD_LDS_PRIO
#define CFD_LDS_PRIO 1      // progress-ordered issue priority (LdsMarch::set_prio); 0: waves end 21..39 us apart (r2 timeline)
#endif
#ifndef CFD_LDS_ST_AUX
#define CFD_LDS_ST_AUX 16   // p' stores write-through (sc1): 5.07 vs 5.13 us/sweep plain, nt 5.78 (r3 ab_staux.log)
#endif
#ifndef CFD_LDS_SPEC_WPE
#define CFD_LDS_SPEC_WPE 5  // SPEC launch's waves per SIMD (4 unpinned, at 99 VGPRs): T = 8 69.7 -> 58.5 us, a few spills
#endif
#ifndef CFD_PERSIST_WPE
#define CFD_PERSIST_WPE 3   // k_jacobi_persist: the padded launch's 3 waves per SIMD, at most 168 VGPRs
#endif
#ifndef CFD_LDS_STAMP
#define CFD_LDS_STAMP 0     // diagnostic builds: the wave timeline below (tools/lds_stamps.py)
#endif

namespace cfd {

constexpr int kLdsWaves = 4;   // waves per workgroup (256 threads)

#if CFD_LDS_STAMP
// The wave timeline of a stamp build (one unit compiled with -DCFD_LDS_STAMP=1,
// by default cfd_jacobi_lds8): every wave of a RES=false launch records its
// start and end (s_memrealtime, 100 MHz), its shader-clock span (s_memtime)
// and its HW_ID / XCC_ID in g_lds_stamp (vector stores); cfd_diag_lds_stamps
// reads that unit's array back.  Off in the product build.
namespace {
constexpr int kStampWaves = 1 << 15;
__device__ unsigned long long g_lds_stamp[kStampWaves * 4];
template <bool RES>
struct StampOnExit {
    unsigned long long rt0, t0;
    unsigned long long bid;   // the XCD-renumbered block (tile: bid % nwc, row group bid / nwc)
    __device__ explicit StampOnExit(int b)
        : rt0(__builtin_amdgcn_s_memrealtime()), t0(__builtin_amdgcn_s_memtime()),
          bid((unsigned long long)b) {}
    __device__ ~StampOnExit() {
        if (RES) return;
        const unsigned long long rt1 = __builtin_amdgcn_s_memrealtime();
        const unsigned long long t1 = __builtin_amdgcn_s_memtime();
        // hwreg(id, 0, 32): HW_ID = 4, XCC_ID = 20
        const unsigned hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));
        const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));
        const int idx = (int)blockIdx.x * kLdsWaves + ((int)threadIdx.x >> 6);
        if ((threadIdx.x & 63) == 0 && idx < kStampWaves) {
            g_lds_stamp[idx * 4 + 0] = rt0;
            g_lds_stamp[idx * 4 + 1] = rt1;
            g_lds_stamp[idx * 4 + 2] = (bid << 40) | ((t1 - t0) & 0xFFFFFFFFFFull);
            g_lds_stamp[idx * 4 + 3] = ((unsigned long long)xcc << 32) | hw;
        }
    }
};
}  // namespace
extern "C" int cfd_diag_lds_stamps(unsigned long long *host, int nwaves) {
    if (nwaves > kStampWaves) nwaves = kStampWaves;
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_lds_stamp), (size_t)nwaves * 32, 0,
                               hipMemcpyDeviceToHost) == hipSuccess ? nwaves : -1;
}
#endif

// lanes of a wave whose columns are stored: 64 minus (T + 1) / 2 halo lanes
// per side (2 columns per lane)
constexpr int lds_outl(int T) { return 64 - 2 * ((T + 1) / 2); }

// The tile geometry of a kind-5 launch: dynamic LDS pad (bytes), wave columns,
// wave segments per column, and the row weights of a column's first / last
// segment (lds_block splits the rows in proportion; 16 = an interior one).
struct LdsTiles {
    int pad, nwc, nseg, wlo, whi;
};
// Fills it (cfd_jacobi_lds.hip) for T sweeps over rows [out_lo, out_hi) in
// `mode` (LdsMarch MODE).  bpc: workgroups of the caller's kernel one CU holds
// with lds_pad_bytes(g, mode) of dynamic LDS (its occupancy query).
// one_round: the persistent form's single round of resident workgroups.
LdsTiles lds_tiles(const Geom &g, int T, int out_lo, int out_hi, int mode, int bpc, bool one_round);
int lds_pad_bytes(const Geom &g, int mode);
bool lds_sums_grid(const Geom &g);

// per-translation-unit entry points (cfd_jacobi_lds*.hip)
void launch_lds_t567(const Geom &g, const Fields &f, int T, int pass, int par, int it, int out_lo,
                     int out_hi, uint32_t *rs, int mode, hipStream_t s, int lag);
void launch_lds_t8(const Geom &g, const Fields &f, int pass, int par, int it, int out_lo, int out_hi,
                   uint32_t *rs, int mode, hipStream_t s, int lag);
// workgroups of k_jacobi_persist<8, g.fastdiv> per CU (cfd_jacobi_lds_persist.hip)
int persist_blocks_per_cu8(const Geom &g, int pad);

namespace {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
constexpr int lds_gcd(int a, int b) { return b == 0 ? a : lds_gcd(b, a % b); }
// Slots of lag accumulated before stage s when the T stages form G groups,
// each group one slot behind the one before it.
constexpr int lds_off(int s, int T, int G) { return s <= 0 ? 0 : ((s - 1) * G) / T; }
// register window rows per stage: 3, or 4 when a stage reads its
// predecessor's rows one slot late
constexpr int lds_nw(int G) { return G > 1 ? 4 : 3; }
// rhs ring depth: the smallest multiple of lcm(NW, PD) holding the T + off(T)
// + 1 rows between the newest load and the last stage's read
constexpr int ring_depth(int T, int PD, int G) {
    const int nw = lds_nw(G);
    const int q = nw / lds_gcd(nw, PD) * PD;
    const int need = T + lds_off(T, T, G) + 1;
    return ((need + q - 1) / q) * q;
}

// MODE: 0 plain launch; 1 (RES) the solve's last launch, publishes the last
// stage's residual; 2 (SPEC) the speculative tolerance-mode launch: every
// stage's residual goes to its own sweep's slot set, and the launch is skipped
// once an earlier launch of the solve converged (Ctl::spec_stop); 3 (REDO)
// re-runs the converged launch from its untouched source buffer with the
// run-time stage count Ctl::spec_redo < T (stores only the segment's rows).
// SUMS (persistent launches only, FAST == 1 with dx^2 == dy^2 a power of two,
// r4): the update forms (h + v) * (1/dx^2) instead of h * (1/dx^2) +
// v * (1/dy^2) -- one packed multiply per column pair and stage fewer (10
// VALU instructions instead of 11).  Bitwise the same whenever |h|, |v| <
// 2^104: both products are then exact scalings by a power of two, and
// RN(R h + R v) = R RN(h + v) for R = 2^k (scaling commutes with rounding,
// overflow included; a subnormal h + v is exact).  k_jacobi_persist proves
// that bound per task before it picks SUMS (its guard); otherwise, and for
// every other launch, the reference's form runs.
// (r5's optimistic per-wave SUMS form for per-launch solves and r4's
// whole-solve guard, measured inside the march, lost their A/B against the
// reference's form and were removed in r6.)
// SUMS == 2 (r7, per-launch fixed-count solves of one domain): the fma form,
// fma(h + v, 1/dx^2, -rhs) -- both multiplies and the subtraction in one
// instruction, 9 VALU instead of 11.  Bitwise the same under the same bound
// ((h + v) * R is exact, so the fma rounds once, where the reference's
// subtraction does).  k_jacobi_lds picks it per launch from the whole-solve
// guard whose maxima the corrector finish and the predictor march publish
// (Ctl::sums_state), and runs it as a second complete march.
template <int T, int FAST, int MODE, int SUMS = 0>
struct LdsMarch {
    static constexpr bool RES = MODE == 1 || MODE == 5, SPEC = MODE == 2, REDO = MODE == 3;
    // MODE 4 (PERSIST): a block of k_jacobi_persist; p' moves between
    // workgroups inside the launch, so its loads bypass L1 and its stores
    // write through (sc1 both ways, MI355X_MICROARCH.md visibility rules).
    // MODE 5: its last block, which also publishes the residual (RES)
    static constexpr bool PERSIST = MODE == 4 || MODE == 5;
    // persistent blocks in the reference's form track what the SUMS guard
    // needs: max |p'| of the rows the wave loads (imax) and of the rhs rows it
    // uses (rmax); every persistent block tracks max |p'| of the rows it
    // stores (omax), which are its neighbours' inputs in the next block
    static constexpr bool TRACK_IN = PERSIST && !SUMS;
    static constexpr bool TRACK_OUT = PERSIST;
    static_assert(!SUMS || FAST == 1, "SUMS: reciprocal multiply");
    static constexpr int PLD_AUX = PERSIST ? 16 : 0;
    static constexpr int PST_AUX = PERSIST ? 16 : CFD_LDS_ST_AUX;
    // Stage s of slot v computes row k - s - off(s).  With G = 1 (off = 0)
    // this is the plain pipeline: stage s reads stage s-1's row of the SAME
    // slot, one serial chain of T dependent updates per slot.  With G > 1 the
    // stages form G groups and each group runs one slot behind the previous
    // one: a group's first stage reads rows its predecessor finished in an
    // EARLIER slot, so a slot holds G independent chains of T/G updates (ILP
    // that hides the packed-f32 result latency), for one more window row per
    // stage (NW = 4) and off(T) more warm-up and ring rows.  The set of
    // (stage, row) updates is the same, and so is every value.
    // (G = 2 lost its A/B, but off(s) stays in the source: with it folded to
    // 0 by hand the optimiser sees the stage loop differently before it
    // unrolls, and 31 k_jacobi_lds instantiations come out with other
    // instruction streams -- profiles/r10/isa_compare.md.)
    static constexpr int G = CFD_LDS_SPLIT;
    static constexpr int NW = lds_nw(G);            // register window rows per stage
    static constexpr int PD = CFD_LDS_PD;           // prefetch distance (slots) of p' and rhs
    static constexpr int OFFT = lds_off(T, T, G);
    static constexpr int D = ring_depth(T, PD, G);  // rhs ring depth; PD and NW divide it
    static constexpr int U = D;                     // slot unroll: every ring index compile-time
    static constexpr int WARM = 2 * T + OFFT;       // stage s starts at slot 2s + off(s)
    static constexpr int H = (T + 1) / 2;           // halo lanes per side (2 columns per lane)
    static constexpr int OUTL = lds_outl(T);        // lanes whose columns are stored
    static constexpr int off(int s) { return lds_off(s, T, G); }
    static constexpr int start(int s) { return 2 * s + off(s); }
    static_assert(D % PD == 0 && D % NW == 0 && D >= T + OFFT + 1, "ring geometry");
    static_assert(G >= 1 && G <= T, "stage groups");

    f2 W[T][NW];
    f2 PQ[PD];
    f2 RQ[PD];
    // this wave's D x 64 slots (LDS).  Typed as the packed pair itself: a
    // float2-struct ring made the compiler split every read into a b32 and a
    // b64 load plus a v_mov per stage
    f2 *ring;
    int lane;
    int k_first, S, lo_clamp, hi_clamp, nch, g_first, g_last, g_top, g_zero, row_bytes;
    int wbase;   // first row of the wave's buffer window (descriptors start there)
    int ch, vo_ld, vo_st, abase, dir;
    bool e0, e1;         // residual columns (kCol slots)
    // the Jacobi divisors and their reciprocals (uniform values, not a pointer
    // to the kernel argument: a pointer escaping into the block function made
    // the compiler copy the argument to scratch)
    float dx_sq, r_dx_sq, dy_sq, r_dy_sq, denom, r_denom;
    __amdgpu_buffer_rsrc_t rs_p, rs_r, rs_d;
    float m;
    float omax, imax, rmax;   // PERSIST: the guard's maxima (above)
    float mm[SPEC ? T : 1];   // SPEC: stage s's residual (segment rows only)
    int r0v, r1v;             // the segment's output rows (march order)
    int nst;                  // REDO: stages to run (< T)
    int nyl_;

    LdsMarch() = default;

    __device__ __forceinline__ int act(int vrow) const { return abase + dir * vrow; }

    // Row `vrow` (virtual, march order) of p' or rhs.  Rows outside the
    // allocation lie beyond the global boundary and rows past the segment's
    // last input row are never needed: both are clamped to a row that exists
    // (their values only reach halo rows that the boundary patch overwrites).
    template <int AUX = 0>
    __device__ __forceinline__ f2 ld(__amdgpu_buffer_rsrc_t rs, int vrow) const {
        vrow = vrow < k_first + S ? vrow : k_first + S - 1;
        int row = act(vrow);
        row = row < lo_clamp ? lo_clamp : (row > hi_clamp ? hi_clamp : row);
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, vo_ld, (row - wbase) * row_bytes, AUX);
        return (f2){__uint_as_float(v.x), __uint_as_float(v.y)};
    }
    __device__ __forceinline__ void st(const f2 &x, int row) const {
        const u32x2 v = {__float_as_uint(x.x), __float_as_uint(x.y)};
        __builtin_amdgcn_raw_buffer_store_b64(v, rs_d, vo_st, (row - wbase) * row_bytes, PST_AUX);
    }

    // One reference update (model.rs:775-793) of the lane's column pair.
    __device__ __forceinline__ f2 update(const f2 &B, const f2 &C, const f2 &Tp, const f2 &Rh) const {
        // horizontal: P(i+1) + P(i-1); the neighbour columns come from the
        // adjacent lanes (left lane's second column, right lane's first)
        const float hx = C.y + from_left(C.y);
        const float hy = C.x + from_right(C.x);
        const f2 h = {hx, hy};
        const f2 v = Tp + B;
        f2 s;
        if constexpr (SUMS == 2) {
            // (h + v) * R - Rh in one fma: (h + v) * R is exact (a scaling by
            // a power of two below overflow) and equals the reference's hz +
            // vt, so the fma's single rounding is the reference's subtraction
            const f2 d = __builtin_elementwise_fma(h + v, (f2){r_dx_sq, r_dx_sq}, -Rh);
            const f2 pu = d * r_denom;
            return 0.75f * pu + 0.25f * C;
        } else if constexpr (SUMS == 1) {
            s = (h + v) * r_dx_sq;   // == h * r_dx_sq + v * r_dy_sq under the guard
        } else {
            const f2 hz = fdiv2<FAST>(h, dx_sq, r_dx_sq);
            const f2 vt = fdiv2<FAST>(v, dy_sq, r_dy_sq);
            s = hz + vt;
        }
        const f2 pu = fdiv2<FAST>(s - Rh, denom, r_denom);
        const float omega = 0.75f;
        const float om1 = 1.0f - omega;
        return omega * pu + om1 * C;
    }

    // E: which boundary logic a slot carries.  kCol: the global column
    // patches and the residual's column range (waves at the left/right
    // boundary); kRow: the global row patches and boundary-row stores (waves
    // whose rows reach a global boundary row).
    static constexpr int kCol = 1, kRow = 2;

    template <int E>
    __device__ __forceinline__ f2 stage(const f2 &B, const f2 &C, const f2 &Tp, const f2 &Rh) const {
        f2 o = update(B, C, Tp, Rh);
        if (E & kCol) {
            if (ch == 0) o.x = o.y;             // P(0,j) = P(1,j)
            if (ch == nch - 1) o.y = 0.0f;      // P(nx-1,j) = 0
        }
        return o;
    }

    // Slot v (k = k_first + v), V_ == v (mod U).  GUARD 0: warm-up (V_ == v,
    // stage s runs from slot start(s) on); 1: a full group; 2: the final
    // partial group.
    template <int V_, int GUARD, int E>
    __device__ __forceinline__ void slot(int v) {
        if (GUARD == 2 && v >= S) return;
        const int k = k_first + v;
        W[0][V_ % NW] = PQ[V_ % PD];                                 // input row k
        PQ[V_ % PD] = ld<PLD_AUX>(rs_p, k + PD);
        ring[(V_ % D) * 64 + lane] = RQ[V_ % PD];                    // rhs row k
        RQ[V_ % PD] = ld(rs_r, k + PD);
#pragma unroll
        for (int s = 1; s <= T; ++s) {
            if (GUARD == 0 && V_ < start(s)) continue;               // compile-time
            const int r = k - s - off(s);
            const f2 rh = ring[((V_ - s - off(s) + 8 * D) % D) * 64 + lane];
            // stage s-1 finished row r+1 in slot v - dl (dl = 0 inside a
            // group, 1 at a group's first stage), row r one slot earlier, ...
            constexpr int kW = 4 * NW;
            const int dl = off(s) - off(s - 1);
            const f2 &B = W[s - 1][(V_ - dl - 2 + kW) % NW];         // stage s-1, row r-1
            const f2 &C = W[s - 1][(V_ - dl - 1 + kW) % NW];         //            row r
            const f2 &Tp = W[s - 1][(V_ - dl + kW) % NW];            //            row r+1
            if (REDO && s > nst) continue;                            // wave-uniform
            if constexpr (TRACK_IN) {
                // stage 1 reads every input row (as Tp, once) and every rhs row
                if (s == 1) {
                    imax = fmaxf(fmaxf(imax, fabsf(Tp.x)), fabsf(Tp.y));
                    rmax = fmaxf(fmaxf(rmax, fabsf(rh.x)), fabsf(rh.y));
                }
            }
            f2 n = stage<E>(B, C, Tp, rh);
            if constexpr (SPEC) {
                // every stage is one reference sweep: its max |new - old|.
                // Waves whose rows reach no global boundary row take every
                // row they compute, branch-free: a row outside the segment
                // [r0v, r1v) (warm-up and run-out cone) holds the exact
                // sweep value of an interior row — its inputs are all loaded
                // rows, k_first = r0v - T — which the segment owning it also
                // counts, and a max is unchanged by a repeated element.  The
                // row-edge waves count only their own rows: with k_first =
                // r0v - T, r - r0v = v - s - T (compile-time in the warm-up).
                bool in_seg;
                if constexpr (!(E & kRow))
                    in_seg = true;
                else if constexpr (GUARD == 0)
                    in_seg = V_ - s - T >= 0 && v - s - T < r1v - r0v;
                else
                    in_seg = v - s - T >= 0 && v - s - T < r1v - r0v;
                if (in_seg) {
                    const f2 d = n - C;
                    if (!(E & kCol)) {
                        mm[s - 1] = fmaxf(fmaxf(mm[s - 1], fabsf(d.x)), fabsf(d.y));
                    } else {
                        if (e0) mm[s - 1] = fmaxf(mm[s - 1], fabsf(d.x));
                        if (e1) mm[s - 1] = fmaxf(mm[s - 1], fabsf(d.y));
                    }
                }
            }
            if (REDO && s == nst) {
                // the stored stage: only rows of this segment (the march
                // computes the T-stage window, wider than nst stages need)
                if (r >= r0v && r < r1v) {
                    const int ra = act(r);
                    st(n, ra);
                    if ((E & kRow) && r == g_first) st(n, g_zero);
                    if ((E & kRow) && r == g_last) st(n, g_top);
                }
            } else if (s < T) {
                // stage s's row r-1 is its previous slot's row
                if ((E & kRow) && r == g_top) n = W[s][(V_ - 1 + kW) % NW]; // P(i,ny-1) = P(i,ny-2)
                W[s][V_ % NW] = n;
                if ((E & kRow) && r == g_first) W[s][(V_ - 1 + kW) % NW] = n; // P(i,0) = P(i,1)
            } else {
                const int ra = act(r);
                if (RES && ra >= 0 && ra < nyl_) {
                    const f2 d = n - C;
                    if (!(E & kCol)) {
                        m = fmaxf(fmaxf(m, fabsf(d.x)), fabsf(d.y));
                    } else {
                        if (e0) m = fmaxf(m, fabsf(d.x));
                        if (e1) m = fmaxf(m, fabsf(d.y));
                    }
                }
                st(n, ra);
                if ((E & kRow) && r == g_first) st(n, g_zero);
                if ((E & kRow) && r == g_last) st(n, g_top);
                if constexpr (TRACK_OUT) omax = fmaxf(fmaxf(omax, fabsf(n.x)), fabsf(n.y));
            }
        }
    }

    template <int V_, int E>
    __device__ __forceinline__ void warmup() {
        if constexpr (V_ < WARM) {
            slot<V_, 0, E>(V_);
            warmup<V_ + 1, E>();
        }
    }

    // U slots from `base`; WARM == base (mod U)
    template <int J, int GUARD, int E>
    __device__ __forceinline__ void group(int base) {
        if constexpr (J < U) {
            slot<WARM + J, GUARD, E>(base + J);
            group<J + 1, GUARD, E>(base);
        }
    }

    // Issue priority from progress.  The SIMD arbiter issues from the oldest
    // ready wave, so of the ~4 equal marches sharing a SIMD the first-launched
    // finishes first and the last one runs its final third nearly alone, at
    // the latency of its own dependent chain (r2 wave timeline: ends at 21 /
    // 25 / 32 / 39 us for one 40-row launch).  A wave lowers its priority as
    // it passes each quarter of its march, so the waves behind catch up and
    // the SIMD keeps four waves to issue from until close to the end.
    __device__ __forceinline__ void set_prio(int done) const {
        if (!CFD_LDS_PRIO) return;
        const int rows = S - WARM, d4 = 4 * done;   // wave-uniform
        if (d4 >= 3 * rows)
            __builtin_amdgcn_s_setprio(0);
        else if (d4 >= 2 * rows)
            __builtin_amdgcn_s_setprio(1);
        else if (d4 >= rows)
            __builtin_amdgcn_s_setprio(2);
        else
            __builtin_amdgcn_s_setprio(3);
    }

    // E: 0 (interior waves), kCol (waves at the left/right boundary), or
    // kCol|kRow (waves whose rows reach a global boundary row; the column
    // patches are no-ops on interior columns).  Chosen once per wave: a
    // per-group switch between paths costs ~15 VGPRs of phi copies.
    template <int E>
    __device__ __forceinline__ void run() {
        set_prio(0);
        warmup<0, E>();
        int base = WARM;
        const int full_end = WARM + ((S - WARM) / U) * U;
        for (; base < full_end; base += U) {
            set_prio(base - WARM);
            group<0, 1, E>(base);
        }
        set_prio(base - WARM);
        if (base < S) group<0, 2, E>(base);
    }
};

// One T-sweep block of one workgroup's four wave tiles (the body of
// k_jacobi_lds; k_jacobi_persist runs it once per block).  `bid`: the
// workgroup's (XCD-renumbered) index.  Returns without touching memory for
// waves with no rows.
// trk (persistent blocks): per wave, trk[3 w .. 3 w + 2] = max |p'| of the
// rows it stored, of the p' rows it loaded and of the rhs rows it used (the
// last two only in the reference's form; 0 where not tracked or no rows).
template <int T, int FAST, int MODE, int SUMS = 0>
__device__ __forceinline__ void lds_block(const Geom &g, float *__restrict__ pa,
                                          float *__restrict__ pb, const float *__restrict__ rhs,
                                          Ctl *ctl, uint32_t *res_slots, int par, int out_lo,
                                          int out_hi, int nwc, int nseg, int wlo, int whi, f2 *lds,
                                          int nst, int bid, float *trk = nullptr) {
    using M = LdsMarch<T, FAST, MODE, SUMS>;
    constexpr bool RES = M::RES;
    M w;
    w.nst = nst;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = (int)threadIdx.x & 63;
    if (M::PERSIST && trk && lane == 0) trk[3 * wave] = trk[3 * wave + 1] = trk[3 * wave + 2] = 0.0f;
    const int wc = bid % nwc;
    const int seg = (bid / nwc) * kLdsWaves + wave;
    const int nrows = out_hi - out_lo;
    if (seg >= nseg) return;
    // rows split in proportion to weights: 16 per segment, wlo / whi for the
    // first / last one (lighter where that segment runs the boundary-row path)
    const long total = nseg == 1 ? 16 : wlo + whi + 16L * (nseg - 2);
    auto cum = [&](int i) -> long { return i <= 0 ? 0 : (i >= nseg ? total : wlo + 16L * (i - 1)); };
    const int r0 = out_lo + (int)(cum(seg) * nrows / total);
    const int r1 = out_lo + (int)(cum(seg + 1) * nrows / total);
    if (r0 >= r1) return;
    const int nx = g.nx;
    w.ring = lds + wave * M::D * 64;
    w.lane = lane;
    w.nch = nx / 2;
    w.nyl_ = g.nyl;
    w.lo_clamp = -g.hg;
    w.hi_clamp = g.nyl + g.hg - 1;
    w.ch = wc * M::OUTL - M::H + lane;
    const bool in_dom = w.ch >= 0 && w.ch < w.nch;
    const bool out_lane = in_dom && lane >= M::H && lane < 64 - M::H;
    const int col = 2 * w.ch;
    w.row_bytes = nx * 4;
    constexpr int kFar = 0x7FFF0000;   // voffset of a lane that must not touch memory
    w.vo_ld = in_dom ? col * 4 : kFar;
    w.vo_st = out_lane ? col * 4 : kFar;
    // buffers ping-pong once per LAUNCH: par = launches since the solve began
    const int si = (ctl->cur + par) & 1;
    float *src_alloc = si ? pb : pa;
    float *dst_alloc = si ? pa : pb;
    // buffer descriptors over the rows this wave can touch, [r0 - T, r1 + T)
    // clamped to the allocation, with a row of margin: offsets stay small at
    // any field size, so a parked lane's voffset (kFar) plus the row offset
    // never wraps 2^32 and always lands past the window (fields of any size,
    // not just up to 1 GiB)
    const int wb = max(w.lo_clamp, r0 - T - 1), wt = min(w.hi_clamp, r1 + T);
    w.wbase = wb;
    const long woff = (long)(wb - w.lo_clamp) * nx;
    const int wbytes = (wt - wb + 1) * nx * 4;
    w.rs_p = __builtin_amdgcn_make_buffer_rsrc(src_alloc + woff, 0, wbytes, 0x00020000);
    w.rs_d = __builtin_amdgcn_make_buffer_rsrc(dst_alloc + woff, 0, wbytes, 0x00020000);
    w.rs_r = __builtin_amdgcn_make_buffer_rsrc((void *)(rhs - (long)g.hg * nx + woff), 0, wbytes,
                                               0x00020000);
    w.dx_sq = g.dx_sq;
    w.r_dx_sq = g.r_dx_sq;
    w.dy_sq = g.dy_sq;
    w.r_dy_sq = g.r_dy_sq;
    w.denom = g.denom;
    w.r_denom = g.r_denom;
    // residual columns 1..=nx-8 (the reference's full 8-lane chunks, Q6)
    w.e0 = out_lane && col >= 1 && col <= nx - 8;
    w.e1 = out_lane && col + 1 >= 1 && col + 1 <= nx - 8;
    w.g_first = 1 - g.j0;
    w.g_last = g.ny - 2 - g.j0;
    w.g_top = g.ny - 1 - g.j0;
    w.g_zero = -g.j0;
    w.m = 0.0f;
    w.omax = w.imax = w.rmax = 0.0f;
#pragma unroll
    for (int s = 0; s < (M::SPEC ? T : 1); ++s) w.mm[s] = 0.0f;
    w.r0v = r0;
    w.r1v = r1;
    w.k_first = r0 - T;
    w.S = (r1 - r0) + M::WARM;
    w.abase = 0;
    w.dir = 1;
    const f2 z = {0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < T; ++s)
#pragma unroll
        for (int q = 0; q < M::NW; ++q) w.W[s][q] = z;
    // edge waves: a lane stores column 0 or a column outside the residual
    // range, or a stage touches a global boundary row; interior waves skip
    // all boundary logic
    const int ch_lo = wc * M::OUTL - M::H, ch_hi = ch_lo + 63;
    const bool col_edge = ch_lo <= 0 || 2 * (ch_hi + 1) > nx - 8;
    const int lo_row = w.k_first - 2, hi_row = r1 + T + M::OFFT + 2;   // every row a stage computes
    auto hits = [&](int r) { return r >= lo_row && r <= hi_row; };
    const bool row_edge = hits(w.g_zero) || hits(w.g_first) || hits(w.g_last) || hits(w.g_top);
    const bool edge = col_edge || row_edge;
    // odd interior segments march downward through the mirrored rows (the
    // stencil is symmetric and f32 addition commutative: same bits), so
    // neighbouring segments read their shared rows at the same time
    if (!edge && (seg & 1)) {
        w.abase = r0 + r1 - 1;
        w.dir = -1;
    }
#pragma unroll
    for (int q = 0; q < M::PD; ++q) {
        w.PQ[q] = w.template ld<M::PLD_AUX>(w.rs_p, w.k_first + q);
        w.RQ[q] = w.ld(w.rs_r, w.k_first + q);
    }
    // the march and what the launch publishes
    if (row_edge)
        w.template run<M::kCol | M::kRow>();
    else if (col_edge)
        w.template run<M::kCol>();
    else
        w.template run<0>();
    if (M::PERSIST && trk) {
        const float o = wave_max(out_lane ? w.omax : 0.0f);
        const float im = M::TRACK_IN ? wave_max(w.imax) : 0.0f;
        const float rm = M::TRACK_IN ? wave_max(w.rmax) : 0.0f;
        if (lane == 0) {
            trk[3 * wave] = o;
            trk[3 * wave + 1] = im;
            trk[3 * wave + 2] = rm;
        }
    }
    if (M::SPEC) {
#pragma unroll
        for (int s = 0; s < T; ++s) {
            const float ms = wave_max(out_lane ? w.mm[s] : 0.0f);
            if (lane == 0 && ms > 0.0f)
                atomicMax(res_slots + (size_t)s * kResSlots * kResStride +
                              ((bid * kLdsWaves + wave) & (kResSlots - 1)) * kResStride,
                          __float_as_uint(ms));
        }
    }
    if (!RES) return;
    const float m = wave_max(out_lane ? w.m : 0.0f);
    if (lane == 0) publish_max(res_slots, bid * kLdsWaves + wave, m);
}

// Minimum waves per SIMD the register allocation must allow (the SPEC
// launch holds T residual maxima on top of the plain march: 99 VGPRs, 4
// waves; pinned to 5 it spills).
constexpr int lds_min_waves(int mode) { return mode == 2 ? CFD_LDS_SPEC_WPE : 1; }
// The lagged early-exit check (r5, single-domain speculative solves; replaces
// the one-workgroup k_spec_check launch after every speculative launch): each
// workgroup of the NEXT launch folds the T residual slot sets of launch lpar
// itself (sweeps [it0, it0 + T), published a launch boundary earlier, never
// reset during the solve -- the finalize folds and clears them) and finds the
// first sweep below p_tol (model.rs:816).  Every workgroup computes the same
// value; workgroup 0 publishes it (the launches that ran and, with `stop`, the
// stop / re-run fields k_spec_check would set).  Returns that sweep's index,
// T when none converged.  Called by every thread of the workgroup.
__device__ __forceinline__ int spec_lag_first(const Geom &g, Ctl *ctl, const uint32_t *set0, int it0,
                                              int T, int lpar, bool stop = true) {
    __shared__ float e_s[kMaxTemporal];
    const int wv = (int)threadIdx.x >> 6;
    for (int s = wv; s < T; s += kLdsWaves) {
        const float v = read_max(set0 + (size_t)s * kResSlots * kResStride, ctl->err[it0 + s]);
        if ((threadIdx.x & 63) == 0) e_s[s] = v;
    }
    __syncthreads();
    int j = 0;
    while (j < T && !(e_s[j] < g.p_tol)) ++j;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ctl->spec_launches = lpar + 1;
        if (stop && j < T) {
            ctl->spec_stop = 1;
            ctl->spec_launch = lpar;
            ctl->spec_redo = j + 1 < T ? j + 1 : 0;
        }
    }
    return j;
}

template <int T, int FAST, int MODE>
__global__ __launch_bounds__(kLdsWaves * 64, lds_min_waves(MODE)) void k_jacobi_lds(
    Geom g, float *__restrict__ pa, float *__restrict__ pb, const float *__restrict__ rhs,
    Ctl *ctl, uint32_t *res_slots, int pass, int par, int out_lo, int out_hi, int nwc, int nseg,
    int wlo, int whi, int it, int lag, float sums_c) {
    using M = LdsMarch<T, FAST, MODE>;
    __shared__ f2 lds[kLdsWaves * M::D * 64];
#if CFD_LDS_STAMP
    StampOnExit<M::RES> stamp_guard(xcd_block(g));
#endif
    if (pass_off(ctl, pass)) return;
    int nst = 0;
    if constexpr (M::SPEC) {
        if (lag > 0) {
            // the previous launch's check (k_spec_check's, a launch boundary
            // after its residuals were published).  spec_stop is read once
            // per workgroup: workgroup 0 of THIS launch may set it meanwhile,
            // and the workgroup's waves must take one path (barriers below)
            __shared__ int stop_s;
            if (threadIdx.x == 0) stop_s = ctl->spec_stop;
            __syncthreads();
            if (stop_s) return;
            if (spec_lag_first(g, ctl, res_slots - (size_t)lag * kResSlots * kResStride, it - lag, lag,
                               par - 1) < lag)
                return;   // it converged: this launch and every later one skip
        } else if (ctl->spec_stop) {
            return;   // an earlier launch of the solve converged
        }
    }
    if constexpr (M::REDO) {
        if (lag > 0 && !ctl->spec_stop) {
            // the solve's last launch (par, sweeps [it, it + lag)) is checked
            // here; only the count of launches that ran is published (the
            // other workgroups read spec_stop / spec_redo / spec_launch)
            const int j = spec_lag_first(g, ctl, res_slots, it, lag, par, false);
            nst = j + 1 < lag ? j + 1 : 0;
        } else {
            nst = ctl->spec_redo;
            par = ctl->spec_launch;   // re-run that launch: same source, same destination
        }
        if (nst <= 0) return;
    }
    // The fma form (LdsMarch SUMS == 2), fixed-count launches of one domain:
    // sums_c = 0.1875 * kMaxSweeps (the most sweeps any solve has: the bound
    // holds for every launch of every solve, whatever its count) where the
    // grid allows the form (launch_lds_t), else 0.  A sweep moves max |p'| by at most 0.1875 Rm / R
    // (Rm = max |rhs|, R = 1/dx^2) and the boundary copies never raise it, so
    // every |p'| of the solve stays below M0 + sums_c Rm / R; the form runs
    // when that is below 2^123 / R (then R |h|, R |v| < 2^127).  M0 and Rm
    // are the finish's and the predictor march's maxima (Ctl::sums_state);
    // NaN / Inf bits make the sum NaN or Inf and fail the test.  One branch,
    // wave-uniform, between two complete marches that share only arguments.
    if constexpr (FAST == 1 && MODE <= 1) {
        if (sums_c > 0.0f && ctl->sums_state == 2u) {
            const float bound = __uint_as_float(ctl->sums_m0) * g.r_dx_sq + sums_c * __uint_as_float(ctl->sums_rm);
            if (bound < 0x1p123f) {
                if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&ctl->sums_launches, 1u);
                lds_block<T, FAST, MODE, 2>(g, pa, pb, rhs, ctl, res_slots, par, out_lo, out_hi, nwc, nseg,
                                            wlo, whi, lds, nst, xcd_block(g));
                return;
            }
        }
    }
    lds_block<T, FAST, MODE>(g, pa, pb, rhs, ctl, res_slots, par, out_lo, out_hi, nwc, nseg, wlo,
                             whi, lds, nst, xcd_block(g));
}

// Workgroups of k_jacobi_lds<T, FAST, MODE> one CU holds at once with `pad`
// bytes of dynamic LDS (occupancy API, cached per instantiation).
template <int T, int FAST, int MODE>
int lds_blocks_per_cu(int pad) {
    static int cache[2] = {0, 0};   // unpadded, padded (one pad value per process)
    int &nb = cache[pad > 0 ? 1 : 0];
    if (nb == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &n, reinterpret_cast<const void *>(&k_jacobi_lds<T, FAST, MODE>), kLdsWaves * 64, pad) !=
                hipSuccess ||
            n < 1)
            n = 1;
        nb = n;
    }
    return nb;
}

template <int T, int MODE>
void launch_lds_t(const Geom &g, const Fields &f, int pass, int par, int it, int out_lo, int out_hi,
                  uint32_t *rs, hipStream_t s, int lag = 0) {
    const int bpc = with_fastdiv(g.fastdiv, [&](auto F) {
        return lds_blocks_per_cu<T, F(), MODE>(lds_pad_bytes(g, MODE));
    });
    const LdsTiles t = lds_tiles(g, T, out_lo, out_hi, MODE, bpc, false);
    const dim3 grid(t.nwc * cdiv(t.nseg, kLdsWaves)), block(kLdsWaves * 64);
    float *pa = f.pp[0] - (long)g.hg * g.nx, *pb = f.pp[1] - (long)g.hg * g.nx;
    // the fma form's guard constant (k_jacobi_lds): fixed-count launches of
    // one domain (a slab's bound would need its neighbours' maxima) on a grid
    // that allows the form; the sweeps of a solve are at most kMaxSweeps
    const float sums_c =
        MODE <= 1 && g.j0 == 0 && g.nyl == g.ny && lds_sums_grid(g) ? 0.1875f * kMaxSweeps : 0.0f;
    with_fastdiv(g.fastdiv, [&](auto F) {
        hipLaunchKernelGGL((k_jacobi_lds<T, F(), MODE>), grid, block, t.pad, s, g, pa, pb, f.rhs, f.ctl,
                           rs, pass, par, out_lo, out_hi, t.nwc, t.nseg, t.wlo, t.whi, it, lag, sums_c);
    });
}

// T sweeps per launch: mode 0 / 1 (plain / last-stage residual, chosen by
// rs != nullptr), 2 (SPEC, rs = the first stage's slot set), 3 (REDO, T = 8).
template <int T>
void launch_lds_T(const Geom &g, const Fields &f, int pass, int par, int it, int out_lo, int out_hi,
                  uint32_t *rs, int mode, hipStream_t s, int lag = 0) {
    if (mode == 2) {
        launch_lds_t<T, 2>(g, f, pass, par, it, out_lo, out_hi, rs, s, lag);
        return;
    }
    if constexpr (T == 8) {
        if (mode == 3) {
            launch_lds_t<8, 3>(g, f, pass, par, it, out_lo, out_hi, rs, s, lag);
            return;
        }
    }
    if (rs)
        launch_lds_t<T, 1>(g, f, pass, par, it, out_lo, out_hi, rs, s);
    else
        launch_lds_t<T, 0>(g, f, pass, par, it, out_lo, out_hi, rs, s);
}

}  // namespace
}  // namespace cfd
