// cfd_correct.h — the reference's corrector arithmetic (apply_corrector,
// model.rs:1334-1404) and the publications that end a corrector launch, shared
// by the corrector kernels (cfd_correct.hip) and the fused finish of the
// predictor march (cfd_predict_march.hip).  Each helper keeps the
// reference's evaluation order, so every kernel that calls it stores the same
// bits.  The divergence of a pass head is div4 (cfd_device.h).
#pragma once
#include "cfd_device.h"

namespace cfd {
namespace {

// u face i from u* and the p' cells either side (model.rs:1336-1362); faces
// nx-7..nx-1 are the scalar tail: (dt * dp) / dx (Q9)
template <int SP>
__device__ __forceinline__ float u_corr(const Geom &g, float us, float pr, float pw, float dt, int i) {
    return i >= g.nx - 7 ? us - sdiv<SP>(dt * (pr - pw), g.dx, g.r_dx)
                         : us - dt * sdiv<SP>(pr - pw, g.dx, g.r_dx);
}

// v face from v* and the p' cells above and below (model.rs:1366-1389, rows
// 1..ny-1; nx % 8 == 0, so its scalar tail :1368-1376 never runs) ...
template <int SP>
__device__ __forceinline__ float v_corr(const Geom &g, float vs, float pt, float pb, float dt) {
    return vs - dt * sdiv<SP>(pt - pb, g.dy, g.r_dy);
}
// ... and of 4 consecutive columns, into o (written component by component:
// a float4 returned by value and copied whole reaches the optimiser as another
// type, and k_correct_finish4m's code came out different)
template <int SP>
__device__ __forceinline__ void v_corr4(const Geom &g, const float4 &vs, const float4 &pt,
                                        const float4 &pb, float dt, float4 &o) {
    o.x = v_corr<SP>(g, vs.x, pt.x, pb.x, dt);
    o.y = v_corr<SP>(g, vs.y, pt.y, pb.y, dt);
    o.z = v_corr<SP>(g, vs.z, pt.z, pb.z, dt);
    o.w = v_corr<SP>(g, vs.w, pt.w, pb.w, dt);
}

// Final u face value at (i, j) of the corrector finish, from its operands:
// ustar = u_star at the face (u_star of face nx-1 for the outflow face nx),
// p_right / p_left = the p' cells either side (p'(nx-1), p'(nx-2) for face nx:
// the outflow copies the corrected face nx-1, whose form is the Q9 tail's).
template <int SP>
__device__ __forceinline__ float cf_u_face(const Geom &g, float inlet, float dt, int i, int j,
                                           float ustar, float p_right, float p_left) {
    const int nx = g.nx;
    if (j == 0) return 0.0f;
    if (j == g.ny - 1) return (g.bc_kind == 1 && i > 0 && i < nx) ? inlet : 0.0f;
    if (i == 0) return g.bc_kind == 0 ? inlet_value(g, inlet, j) : 0.0f;
    if (i == nx) return g.bc_kind == 0 ? u_corr<SP>(g, ustar, p_right, p_left, dt, nx) : 0.0f;
    return u_corr<SP>(g, ustar, p_right, p_left, dt, i);
}

// p += p' (model.rs:1392-1403)
__device__ __forceinline__ float4 add4(float4 a, const float4 &b) {
    a.x = a.x + b.x;
    a.y = a.y + b.y;
    a.z = a.z + b.z;
    a.w = a.w + b.w;
    return a;
}

// The workgroup's four step maxima (max |u - u_old|, |v - v_old|, |u|, |v|:
// model.rs:333-344, :879-880) into the spread sets of Fields::red_slots: the
// waves fold, then one atomic per maximum and workgroup.  Every thread of the
// workgroup calls it.
__device__ __forceinline__ void publish_step_maxima(const Fields &f, int bid, float du, float dv,
                                                    float mu, float mv) {
    __shared__ float red[kBlock / 64][4];
    du = wave_max(du);
    dv = wave_max(dv);
    mu = wave_max(mu);
    mv = wave_max(mv);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[wv][0] = du;
        red[wv][1] = dv;
        red[wv][2] = mu;
        red[wv][3] = mv;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        float r = 0.f;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) r = fmaxf(r, red[w][threadIdx.x]);
        publish_max(f.red_slots + (size_t)threadIdx.x * kResSlots * kResStride, bid, r);
    }
}

// The fma form's p' bound (Ctl::sums_m0, sums_state 0 -> 1): a bound of max
// |p'| over the owned rows, the p' the next step's solve starts from (warm
// start), for its guard (the word is zero since the solve's finalize): the
// threshold, raised by any lane whose pm -- its maximum of abs_bits(p') --
// is larger (NaN and Inf included).  The next predictor march bounds the rhs
// in sums_rm.  Every thread of the launch calls it.
__device__ __forceinline__ void publish_sums_m0_bound(const Geom &g, Ctl *c, uint32_t pm) {
    const uint32_t thr = __float_as_uint(kSumsPLim * g.dx_sq);   // 2^122 / R, exact
    raise_bits_bound(&c->sums_m0, pm, thr);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        atomicMax(&c->sums_m0, thr);
        c->sums_rm = 0u;
        c->sums_state = 1u;
    }
}

}  // namespace
}  // namespace cfd
