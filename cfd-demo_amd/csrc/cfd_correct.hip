// cfd_correct.hip — the corrector kernels of Model::update (K5, K5'):
// apply_corrector (model.rs:1334-1404) as its own launch, fused with the next
// pass's head (k_correct_head4), and fused with the boundaries and the step
// maxima (k_correct_finish4m).  The arithmetic is cfd_correct.h's, so every
// form stores the same bits; built like cfd_kernels.hip (-ffp-contract=off,
// correctly rounded division).
//
// Citations are /root/reference/src/model.rs line numbers.
#include "cfd_correct.h"

namespace cfd {
namespace {

// ------------------------------------------------------------- corrector (K5)

// apply_corrector (model.rs:1334-1404).  u: all owned rows, faces 1..nx-1
// (u_corr: the Q9 tail).  v: global rows 1..=ny-1 held by this slab (incl. the
// shared face row).  p += p'.
template <int SP>
__global__ __launch_bounds__(kBlock) void k_corrector(Geom g, Fields f, int pass,
                                                      float dt_override, int nbx) {
    Ctl *c = f.ctl;
    if (pass_off(c, pass)) return;
    const int bid = xcd_block(g);
    const int i = (bid % nbx) * kBlock + (int)threadIdx.x;   // 0..nx
    const int lj = bid / nbx;                                // 0..nyl
    const int nx = g.nx, W = nx + 1;
    if (i > nx) return;
    const float dt = dt_of(c, dt_override);
    const float *__restrict__ pp = c->cur ? f.pp[1] : f.pp[0];
    const int j = g.j0 + lj;
    if (lj < g.nyl && i >= 1 && i <= nx - 1) {
        const float p_right = pp[(long)lj * nx + i];
        const float p_left = pp[(long)lj * nx + i - 1];
        const long k = (long)lj * W + i;
        f.u[k] = u_corr<SP>(g, f.u_star[k], p_right, p_left, dt, i);
    }
    if (i < nx && j >= 1 && j <= g.ny - 1) {
        const float p_top = pp[(long)lj * nx + i];
        const float p_bottom = pp[(long)(lj - 1) * nx + i];
        const long k = (long)lj * nx + i;
        f.v[k] = v_corr<SP>(g, f.v_star[k], p_top, p_bottom, dt);
    }
    if (i < nx && lj < g.nyl) {
        const long k = (long)lj * nx + i;
        f.p[k] = f.p[k] + pp[k];
    }
}

// k_corrector with a thread per 4 consecutive cells of a row: the p', v, v*
// and p rows (pitch nx, 16-byte aligned) move as float4, the u / u* row
// (pitch nx+1) as scalars; the left neighbour p'(i0-1) of the first u face is
// one more scalar load.  The same expressions per face and cell as
// k_corrector (Q9 tail included), so the same bits; one float per thread held
// the corrector at ~4 TB/s.
template <int SP>
__global__ __launch_bounds__(kBlock) void k_corrector4(Geom g, Fields f, int pass,
                                                       float dt_override, int nbx) {
    Ctl *c = f.ctl;
    if (pass_off(c, pass)) return;
    const int bid = xcd_block(g);
    const int i0 = 4 * ((bid % nbx) * kBlock + (int)threadIdx.x);   // cells i0..i0+3
    const int lj = bid / nbx;                                       // 0..nyl
    const int nx = g.nx, W = nx + 1;
    if (i0 >= nx) return;
    const float dt = dt_of(c, dt_override);
    const float *__restrict__ pp = c->cur ? f.pp[1] : f.pp[0];
    const int j = g.j0 + lj;
    const long kc = (long)lj * nx + i0;
    float4 pc = {0.f, 0.f, 0.f, 0.f};
    if (lj < g.nyl) {
        pc = *reinterpret_cast<const float4 *>(pp + kc);
        const float pl = i0 > 0 ? pp[kc - 1] : 0.0f;
        const float pr[4] = {pc.x, pc.y, pc.z, pc.w};
        const float pw[4] = {pl, pc.x, pc.y, pc.z};
        const long ku = (long)lj * W + i0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q;
            if (i < 1 || i > nx - 1) continue;
            f.u[ku + q] = u_corr<SP>(g, f.u_star[ku + q], pr[q], pw[q], dt, i);
        }
    }
    if (j >= 1 && j <= g.ny - 1) {
        const float4 pt = lj < g.nyl ? pc : *reinterpret_cast<const float4 *>(pp + kc);
        const float4 pb = *reinterpret_cast<const float4 *>(pp + kc - nx);
        const float4 vs = *reinterpret_cast<const float4 *>(f.v_star + kc);
        float4 o;
        v_corr4<SP>(g, vs, pt, pb, dt, o);
        *reinterpret_cast<float4 *>(f.v + kc) = o;
    }
    if (lj < g.nyl)
        *reinterpret_cast<float4 *>(f.p + kc) = add4(*reinterpret_cast<const float4 *>(f.p + kc), pc);
}

// The corrector of pass k fused with the head of pass k+1 (model.rs:693 +
// 698-704: apply_corrector, then u* <- u, v* <- v and rhs = div(u*, v*)/dt)
// when the device says pass k+1 runs (Ctl::go[pass+1], set by the solve's
// finalize before this launch); otherwise the plain corrector.  Single domain,
// one thread per 4 cells of an allocation row.
//
// The corrected velocities go straight into the next pass's u* / v*, and
// u / v get their final values only from the loop's last corrector: every
// pass's corrector overwrites every corrected face of u and v and leaves the
// others (u faces 0 and nx, v rows 0 and ny, ghost rows) as they are, which is
// also what the copies give u* / v* there.  The divergence of a row needs the
// corrected east face u(i0+4) of the next thread and v of the next row: both
// are recomputed here from the corrector's inputs with its own expressions
// (the same bits), so those inputs must not be overwritten by this launch --
// the passes alternate arrays.  Pass k reads its u* / v* from u_star / v_star
// when k is even and from u / v when k is odd, and writes the corrected values
// to the other pair:
//   head, k even: u_star -> u (u already holds u at the uncorrected places);
//   head, k odd:  u -> u_star (plus u* <- u at the uncorrected places, ghost
//                 rows included, as k_copy_star_div does);
//   last, k even: k_corrector4 (u <- u_star - corr);
//   last, k odd:  u_star <- u everywhere (the reference's u* of the last
//                 pass), then u <- u - corr in place (elementwise).
// p += p' in every pass.  32 B per cell (read u*, v*, p', p; write the other
// pair, p, rhs) against 48 for k_corrector4 + k_copy_star_div, and one launch
// per pass fewer.
//
// ROWS allocation rows per thread (r6: a band march of kCfRows rows, as
// k_correct_finish4m): row lr's p' row, its v correction and the p' row below
// it come from row lr-1's iteration -- the v_row of row lr+1 that the
// divergence needs is the next row's vlo, the p' row lr+1 it loads the next
// row's pc -- instead of every row re-reading three p' rows and two v* rows
// and computing two v rows.  The same expressions on the same inputs: bitwise
// the one-row form (ROWS = 1).
template <int SP, int ROWS>
__global__ __launch_bounds__(kBlock) void k_correct_head4(Geom g, Fields f, int pass,
                                                          float dt_override, int nbx, int has_next) {
    Ctl *c = f.ctl;
    if (pass_off(c, pass)) return;
    // pass+1 exists (host) and runs (device: the early exit, model.rs:721)
    const bool head = has_next && c->go[pass + 1] != 0;
    const bool odd = pass & 1;
    const float *__restrict__ in_u = odd ? f.u : f.u_star;   // this pass's u*
    const float *__restrict__ in_v = odd ? f.v : f.v_star;
    float *__restrict__ out_u = odd ? f.u_star : f.u;        // the next pass's u*
    float *__restrict__ out_v = odd ? f.v_star : f.v;
    const int bid = xcd_block(g);
    const int i0 = 4 * ((bid % nbx) * kBlock + (int)threadIdx.x);
    const int nx = g.nx, W = nx + 1, nyl = g.nyl;
    if (i0 >= nx) return;
    const float dt = dt_of(c, dt_override);
    const float *__restrict__ pp = c->cur ? f.pp[1] : f.pp[0];
    auto v_row = [&](int r, const float4 &pt, bool *hit) -> float4 {
        const int jr = g.j0 + r;
        const long k = (long)r * nx + i0;
        *hit = jr >= 1 && jr <= g.ny - 1;   // model.rs:1366: rows 1..ny-1
        if (!*hit) return *reinterpret_cast<const float4 *>(f.v + k);
        const float4 pb = *reinterpret_cast<const float4 *>(pp + k - nx);
        const float4 vs = *reinterpret_cast<const float4 *>(in_v + k);
        float4 o;
        v_corr4<SP>(g, vs, pt, pb, dt, o);
        return o;
    };
    // allocation rows: v rows -G..nyl+G, u rows -G..nyl+G-1
    const int lr0 = (bid / nbx) * ROWS - kGhostUV, lr1 = min(lr0 + ROWS, nyl + 1 + kGhostUV);
    bool carry = false;          // p' row lr and v row lr from row lr-1's iteration
    float4 p_next = {0.f, 0.f, 0.f, 0.f}, v_next = {0.f, 0.f, 0.f, 0.f};
    // an owned head row's loads: p' row r, its west / east neighbours (clamped
    // in-row addresses, the edge lanes' values selected by the caller), u* row
    // r, p' row r+1, v* row r+1 (v where row r+1 is not corrected), p row r
    struct HRow {
        float4 pld, pt, vsn, pv;
        f4u iu;
        float iu4, plv, p4v;
    };
    HRow cur, nxt;
    bool have = false;   // cur holds row lr's loads
    auto load_hrow = [&](int r, HRow &h) {
        const long kc = (long)r * nx + i0, ku = (long)r * W + i0;
        h.pld = *reinterpret_cast<const float4 *>(pp + kc);
        h.plv = pp[kc - (i0 > 0 ? 1 : 0)];
        h.p4v = pp[kc + (i0 + 4 < nx ? 4 : 3)];
        h.iu = *reinterpret_cast<const f4u *>(in_u + ku);   // dword-aligned (pitch nx + 1)
        h.iu4 = in_u[ku + 4];
        h.pt = *reinterpret_cast<const float4 *>(pp + kc + nx);
        const int jr = g.j0 + r + 1;   // model.rs:1366: v rows 1..ny-1 are corrected
        h.vsn = *reinterpret_cast<const float4 *>((jr >= 1 && jr <= g.ny - 1 ? in_v : f.v) + kc + nx);
        h.pv = *reinterpret_cast<const float4 *>(f.p + kc);
    };
    for (int lr = lr0; lr < lr1; ++lr) {
        const long kc = (long)lr * nx + i0, ku = (long)lr * W + i0;
        const bool owned = lr >= 0 && lr < nyl;
        // u* <- u and v* <- v of the whole row (the next pass's u* at places no
        // corrector writes, or the last odd pass's u*): only when u* is out of date
        if (odd && (!head || !owned)) {
            *reinterpret_cast<float4 *>(f.v_star + kc) = *reinterpret_cast<const float4 *>(f.v + kc);
            if (lr < nyl + kGhostUV) {   // not v's extra face row
                const float *__restrict__ ur = f.u + ku;
                float *__restrict__ us = f.u_star + ku;
                *reinterpret_cast<f4u *>(us) = *reinterpret_cast<const f4u *>(ur);
                if (i0 + 4 == nx) us[4] = ur[4];   // face nx
            }
        }
        if (!owned && (head || lr != nyl)) {
            carry = false;
            have = false;
            continue;
        }
        if (!head) {
            // the loop's last corrector: u, v, p final (rows 0..nyl; v's row nyl)
            float4 pc = {0.f, 0.f, 0.f, 0.f};
            if (owned) {
                pc = *reinterpret_cast<const float4 *>(pp + kc);
                const float pl = i0 > 0 ? pp[kc - 1] : 0.0f;
                const float pr[4] = {pc.x, pc.y, pc.z, pc.w};
                const float pw[4] = {pl, pc.x, pc.y, pc.z};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int i = i0 + q;
                    if (i < 1 || i > nx - 1) continue;
                    f.u[ku + q] = u_corr<SP>(g, in_u[ku + q], pr[q], pw[q], dt, i);
                }
            }
            bool hit;
            const float4 o = v_row(lr, owned ? pc : *reinterpret_cast<const float4 *>(pp + kc), &hit);
            if (hit) *reinterpret_cast<float4 *>(f.v + kc) = o;
            if (owned)
                *reinterpret_cast<float4 *>(f.p + kc) = add4(*reinterpret_cast<const float4 *>(f.p + kc), pc);
            carry = false;
            have = false;
            continue;
        }
        // ---- an owned row: corrector k, then pass k+1's copy and divergence
        // Row lr's loads were issued during row lr-1 (cur) unless this is the
        // band's first owned row; row lr+1's go out now, before row lr's
        // stores (no array this row stores is one the next row loads at the
        // same place), so each row's loads overlap the previous row's work.
        if (!have) load_hrow(lr, cur);
        const bool pf = ROWS > 1 && lr + 1 < lr1 && lr + 1 < nyl;   // the next row is owned too
        if (pf) load_hrow(lr + 1, nxt);
        // p' row lr: loaded every row and the carried copy selected, so no
        // branch guards the load; the edge lanes' values selected likewise
        const float4 pc = carry ? p_next : cur.pld;
        const float pl = i0 > 0 ? cur.plv : 0.0f;
        const float p4 = i0 + 4 < nx ? cur.p4v : 0.0f;   // for the east face i0+4
        const float pr[5] = {pc.x, pc.y, pc.z, pc.w, p4};
        const float pw[5] = {pl, pc.x, pc.y, pc.z, pc.w};
        float un[5];
        const float iuq[5] = {cur.iu.x, cur.iu.y, cur.iu.z, cur.iu.w, cur.iu4};
#pragma unroll
        for (int q = 0; q < 5; ++q) un[q] = u_corr<SP>(g, iuq[q], pr[q], pw[q], dt, i0 + q);
        // faces 0 and nx keep u (the only lanes whose i0 + q leaves 1..nx-1)
        if (i0 == 0) un[0] = f.u[ku];
        if (i0 + 4 == nx) un[4] = f.u[ku + 4];
        *reinterpret_cast<f4u *>(out_u + ku) = (f4u){un[0], un[1], un[2], un[3]};
        if (i0 + 4 == nx) out_u[ku + 4] = un[4];
        bool hit;
        const float4 vlo = carry ? v_next : v_row(lr, pc, &hit);
        const float4 pt = cur.pt;
        // v row lr+1 (v_row's expression; its p' row below is pc)
        float4 vhi = cur.vsn;
        {
            const int jr = g.j0 + lr + 1;
            if (jr >= 1 && jr <= g.ny - 1) v_corr4<SP>(g, cur.vsn, pt, pc, dt, vhi);
        }
        *reinterpret_cast<float4 *>(out_v + kc) = vlo;
        *reinterpret_cast<float4 *>(f.p + kc) = add4(cur.pv, pc);
        // the divergence of the new u*, v*
        *reinterpret_cast<float4 *>(f.rhs + kc) = div4<SP>(g, un[0], un[1], un[2], un[3], un[4], vlo, vhi, dt);
        if (pf) cur = nxt;
        have = pf;
        carry = ROWS > 1;
        p_next = pt;
        v_next = vhi;
    }
}

// ------------------------------- fused corrector + boundaries + reductions (K5')

// One row of k_correct_finish4m's work for the 4 columns i0..i0+3 of local
// row lj: pc = p' row lj, pb = p' row lj-1 (loaded by the caller), the step
// maxima and the non-finite flag accumulate into du..bad.
template <int SP>
__device__ __forceinline__ void cf4_row(const Geom &g, const Fields &f, const float *__restrict__ pp,
                                        float inlet, float dt, int i0, int lj, const float4 &pc,
                                        const float4 &pb, float &du, float &dv, float &mu,
                                        float &mv, bool &bad) {
    const int nx = g.nx, W = nx + 1;
    const int j = g.j0 + lj;
    const long rp = (long)lj * nx + i0;
    const bool vrow = (j != 0 && j != g.ny);
    if (lj < g.nyl) {
        const long k = (long)lj * W + i0;
        const float pl = (i0 > 0) ? pp[rp - 1] : 0.0f;
        // u rows have pitch nx + 1: their 4-column groups are dword-aligned
        // only, and move as one 16-byte access each (f4u)
        const f4u su = *reinterpret_cast<const f4u *>(f.u_star + k);
        const float s0 = su.x, s1 = su.y, s2 = su.z, s3 = su.w;
        float n0 = cf_u_face<SP>(g, inlet, dt, i0, j, s0, pc.x, pl);
        float n1 = cf_u_face<SP>(g, inlet, dt, i0 + 1, j, s1, pc.y, pc.x);
        float n2 = cf_u_face<SP>(g, inlet, dt, i0 + 2, j, s2, pc.z, pc.y);
        float n3 = cf_u_face<SP>(g, inlet, dt, i0 + 3, j, s3, pc.w, pc.z);
        if (f.n_obs > 0) {
            if (f.mask_u[k] & 2) n0 = 0.0f;
            if (f.mask_u[k + 1] & 2) n1 = 0.0f;
            if (f.mask_u[k + 2] & 2) n2 = 0.0f;
            if (f.mask_u[k + 3] & 2) n3 = 0.0f;
        }
        const f4u uo = *reinterpret_cast<const f4u *>(f.u + k);
        const float o0 = uo.x, o1 = uo.y, o2 = uo.z, o3 = uo.w;
        *reinterpret_cast<f4u *>(f.u + k) = (f4u){n0, n1, n2, n3};
        du = fmaxf(fmaxf(fmaxf(du, fabsf(n0 - o0)), fmaxf(fabsf(n1 - o1), fabsf(n2 - o2))),
                   fabsf(n3 - o3));
        mu = fmaxf(fmaxf(fmaxf(mu, fabsf(n0)), fmaxf(fabsf(n1), fabsf(n2))), fabsf(n3));
        bad |= nonfinite(n0) || nonfinite(n1) || nonfinite(n2) || nonfinite(n3);
        if (i0 + 4 == nx) {   // outflow face nx copies the corrected face nx-1 (Q9)
            float n4 = cf_u_face<SP>(g, inlet, dt, nx, j, s3, pc.w, pc.z);
            if (f.n_obs > 0 && (f.mask_u[k + 4] & 2)) n4 = 0.0f;
            const float o4 = f.u[k + 4];
            f.u[k + 4] = n4;
            du = fmaxf(du, fabsf(n4 - o4));
            mu = fmaxf(mu, fabsf(n4));
            bad |= nonfinite(n4);
        }
    }
    float4 nv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vrow) v_corr4<SP>(g, *reinterpret_cast<const float4 *>(f.v_star + rp), pc, pb, dt, nv);
    if (f.n_obs > 0) {
        if (f.mask_v[rp] & 2) nv.x = 0.0f;
        if (f.mask_v[rp + 1] & 2) nv.y = 0.0f;
        if (f.mask_v[rp + 2] & 2) nv.z = 0.0f;
        if (f.mask_v[rp + 3] & 2) nv.w = 0.0f;
    }
    const float4 ov = *reinterpret_cast<const float4 *>(f.v + rp);
    *reinterpret_cast<float4 *>(f.v + rp) = nv;
    dv = fmaxf(fmaxf(fmaxf(dv, fabsf(nv.x - ov.x)), fmaxf(fabsf(nv.y - ov.y), fabsf(nv.z - ov.z))),
               fabsf(nv.w - ov.w));
    mv = fmaxf(fmaxf(fmaxf(mv, fabsf(nv.x)), fmaxf(fabsf(nv.y), fabsf(nv.z))), fabsf(nv.w));
    bad |= nonfinite(nv.x) || nonfinite(nv.y) || nonfinite(nv.z) || nonfinite(nv.w);
    if (lj < g.nyl)
        *reinterpret_cast<float4 *>(f.p + rp) = add4(*reinterpret_cast<const float4 *>(f.p + rp), pc);
}

// update() with no extra corrector passes (model.rs:707-730 with
// corrector_passes 0): the one corrector pass (apply_corrector :1334-1404),
// the velocity boundaries (apply_boundary_conditions :827-875) and the step
// residuals/CFL maxima (:333-344, :879-880) in a single pass over the fields.
// Each thread writes the FINAL value of its u faces and v faces — the value the
// reference holds after the boundary routine has run in its order (columns,
// then rows over the corners, then obstacle faces) — and, because u/v are not
// touched between step start and here, the value it overwrites IS u_old/v_old:
// |new - old| needs no copy of the old fields and no second read.  Obstacle
// faces are bit 1 of the device masks.
//
// Four columns per thread: the pitch-nx streams (p', p, v*, v) move as float4
// (16-byte aligned: build_model checks it), the pitch-(nx+1) u streams as one
// dword-aligned 16-byte access, and the thread owning columns nx-4..nx-1 also
// finishes u face nx (one float per thread held the kernel near 4.7 TB/s, like
// the divergence before it went to float4).  Each thread marches down a band
// of ROWS rows: p' row lj, loaded for row lj, is row lj+1's lower neighbour
// (the v correction's p'(j-1)), so every p' row crosses HBM once instead of
// twice.
// ROWS: the band (kCfRows, or 1 where the bands would leave the chip idle:
// cf_rows).
#ifndef CFD_CF_ROWS   // build-time (r6 A/B, profiles/r6/prof_r6ag: C3 16 / 8 / 4 rows
#define CFD_CF_ROWS 16  // 10.04 / 10.36 / 10.18 ms per step)
#endif
constexpr int kCfRows = CFD_CF_ROWS;
template <int SP, int ROWS>
__global__ __launch_bounds__(kBlock) void k_correct_finish4m(Geom g, Fields f, float dt_override,
                                                             int nbx) {
    Ctl *c = f.ctl;
    const int nx = g.nx;
    float du = 0.f, dv = 0.f, mu = 0.f, mv = 0.f;
    uint32_t pm = 0u;
    bool bad = false;
    const int bid = xcd_block(g);
    const int i0 = 4 * ((bid % nbx) * kBlock + (int)threadIdx.x);
    const int l0 = (bid / nbx) * ROWS, l1 = min(l0 + ROWS, g.nyl + 1);
    const float dt = dt_of(c, dt_override);
    const float inlet = c->inlet;
    const float *__restrict__ pp = c->cur ? f.pp[1] : f.pp[0];
    if (i0 < nx) {
        float4 pb = make_float4(0.f, 0.f, 0.f, 0.f);
        {
            const int j = g.j0 + l0;
            if (j != 0 && j != g.ny) pb = *reinterpret_cast<const float4 *>(pp + (long)(l0 - 1) * nx + i0);
        }
        for (int lj = l0; lj < l1; ++lj) {
            const int j = g.j0 + lj;
            const bool vrow = (j != 0 && j != g.ny);
            float4 pc = make_float4(0.f, 0.f, 0.f, 0.f);
            if (lj < g.nyl || vrow) pc = *reinterpret_cast<const float4 *>(pp + (long)lj * nx + i0);
            cf4_row<SP>(g, f, pp, inlet, dt, i0, lj, pc, vrow ? pb : make_float4(0.f, 0.f, 0.f, 0.f),
                        du, dv, mu, mv, bad);
            if (f.sums_track && lj < g.nyl)
                pm = max(max(pm, max(abs_bits(pc.x), abs_bits(pc.y))), max(abs_bits(pc.z), abs_bits(pc.w)));
            pb = pc;
        }
    }
    flag_nonfinite(c, bad);
    if (f.sums_track) publish_sums_m0_bound(g, c, pm);
    publish_step_maxima(f, bid, du, dv, mu, mv);
}

// The fma form's p' bound for a step that does not end in k_correct_finish4m
// -- one with corrector passes, whose last corrector is k_correct_head4: the
// same words the finish publishes, from one pass over the owned rows of the p'
// the last solve left.  Only launched where Fields::sums_track is set.
__global__ __launch_bounds__(kBlock) void k_publish_sums_m0(Geom g, Fields f) {
    Ctl *c = f.ctl;
    const float *__restrict__ pp = c->cur ? f.pp[1] : f.pp[0];
    const size_t n = (size_t)g.nx * (size_t)g.nyl;
    uint32_t pm = 0u;
    for (size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x; k < n; k += (size_t)gridDim.x * kBlock)
        pm = max(pm, abs_bits(pp[k]));
    publish_sums_m0_bound(g, c, pm);
}

// Rows per thread of the corrector bands: kCfRows where that still gives
// every CU two workgroups, else 1 (the 800 x 264 reference default: 17
// workgroups of 16-row bands ran k_correct_head4 in 34.6 us against 5.9 us for
// 270 one-row workgroups, profiles/r6/prof_r6u vs prof_r6l)
int cf_rows(const Geom &g, int nbx, int nrows) {
    return (long)nbx * cdiv(nrows, kCfRows) >= 2L * g.n_cu ? kCfRows : 1;
}

}  // namespace

// ------------------------------------------------------------------ launchers

void launch_corrector(const Geom &g, const Fields &f, int pass, float dt_override, bool vec,
                      hipStream_t s) {
    if (vec && g.nx % 4 == 0 && aligned16(f.v) && aligned16(f.v_star) && aligned16(f.p) &&
        aligned16(f.pp[0]) && aligned16(f.pp[1])) {
        const int nbx4 = cdiv(g.nx / 4, kBlock);
        if (g.sp_pow2)
            hipLaunchKernelGGL(k_corrector4<1>, dim3(nbx4 * (g.nyl + 1)), dim3(kBlock), 0, s, g, f,
                               pass, dt_override, nbx4);
        else
            hipLaunchKernelGGL(k_corrector4<0>, dim3(nbx4 * (g.nyl + 1)), dim3(kBlock), 0, s, g, f,
                               pass, dt_override, nbx4);
        return;
    }
    const int nbx = cdiv(g.nx + 1, kBlock);
    if (g.sp_pow2)
        hipLaunchKernelGGL(k_corrector<1>, dim3(nbx * (g.nyl + 1)), dim3(kBlock), 0, s, g, f, pass,
                           dt_override, nbx);
    else
        hipLaunchKernelGGL(k_corrector<0>, dim3(nbx * (g.nyl + 1)), dim3(kBlock), 0, s, g, f, pass,
                           dt_override, nbx);
}

bool correct_head_ok(const Geom &g, const Fields &f) {
    return g.nx % 4 == 0 && aligned16(f.v) && aligned16(f.v_star) && aligned16(f.p) &&
           aligned16(f.pp[0]) && aligned16(f.pp[1]) && aligned16(f.rhs);
}

void launch_correct_head(const Geom &g, const Fields &f, int pass, float dt_override, bool has_next,
                         hipStream_t s) {
    const int nbx4 = cdiv(g.nx / 4, kBlock);
    const int hn = has_next ? 1 : 0;
    // the band march, kCfRows rows per thread, where it still fills the chip
    // (r6: C3 in the reference's control flow 10.37 -> 10.26 ms per step
    // against one row per thread, best of 3; profiles/r6/prof_r6p/ab_corrhead.log);
    // on small grids one row per thread (cf_rows)
    const int nrows = g.nyl + 1 + 2 * kGhostUV;
    const int rows = cf_rows(g, nbx4, nrows);
    const dim3 grid(nbx4 * cdiv(nrows, rows));
#define CFD_LAUNCH_CH(SPV, RW)                                                                    \
    hipLaunchKernelGGL((k_correct_head4<SPV, RW>), grid, dim3(kBlock), 0, s, g, f, pass, dt_override, \
                       nbx4, hn)
    if (rows == kCfRows) {
        if (g.sp_pow2) CFD_LAUNCH_CH(1, kCfRows); else CFD_LAUNCH_CH(0, kCfRows);
    } else {
        if (g.sp_pow2) CFD_LAUNCH_CH(1, 1); else CFD_LAUNCH_CH(0, 1);
    }
#undef CFD_LAUNCH_CH
}

void launch_correct_finish(const Geom &g, const Fields &f, float dt_override, hipStream_t s) {
    const int nbx = cdiv(g.nx / 4, kBlock);
    const int rows = cf_rows(g, nbx, g.nyl + 1);
    const dim3 grid(nbx * cdiv(g.nyl + 1, rows));
#define CFD_LAUNCH_CF(SPV, RW)                                                                     \
    hipLaunchKernelGGL((k_correct_finish4m<SPV, RW>), grid, dim3(kBlock), 0, s, g, f, dt_override, nbx)
    if (rows == kCfRows) {
        if (g.sp_pow2) CFD_LAUNCH_CF(1, kCfRows); else CFD_LAUNCH_CF(0, kCfRows);
    } else {
        if (g.sp_pow2) CFD_LAUNCH_CF(1, 1); else CFD_LAUNCH_CF(0, 1);
    }
#undef CFD_LAUNCH_CF
}

void launch_publish_sums_m0(const Geom &g, const Fields &f, hipStream_t s) {
    const size_t n = (size_t)g.nx * (size_t)g.nyl;
    hipLaunchKernelGGL(k_publish_sums_m0, dim3(copy_grid(n)), dim3(kBlock), 0, s, g, f);
}

}  // namespace cfd
