// cfd_jacobi_script.hip — the JavaScript variant's default pressure solver
// (cfd_params.pressure_solver 5, index.html:796-838): damped Jacobi, omega 0.7,
// in the script's double arithmetic over f32 arrays.
//
// One iteration is one launch: the interior update (:804-812), max |new - old|
// (:813-820), the interior copy (:822-827) and the boundary copies (:828-835).
// p' ping-pongs: iteration `it` reads buffer (Ctl::cur + it) & 1 and writes the
// other, it = 0 reads nothing (p' restarts from 0, :798), and the caller's
// finalize flips Ctl::cur once per iteration run, so the result's buffer is
// named whichever parity the solve stopped at.
//
// The boundary cells are a function of the new interior alone: after the row
// loop (:828-831) and then the column loop (:832-835), every cell of column 0
// holds its row's new column 1, column nx-1 holds 0, and rows 0 / ny-1 are
// rows 1 / ny-2 with those two columns already applied (the corners follow the
// column loop, which runs last).  So the lane that holds an edge cell's source
// stores the edge cell too, into the buffer it writes: no launch reads a cell
// another workgroup of the same launch writes, and no workgroup waits.  The
// boundary cells an iteration reads are the previous iteration's copies, as in
// the script, where pPrime keeps them between iterations.
//
// Mapping: a wave owns 62 column pairs (lanes 1..62; lanes 0 and 63 only feed
// the horizontal neighbours through DPP lane shifts) and kJsRows interior
// rows; a workgroup is 4 waves = 4 consecutive row segments.  Rows stream
// through three registers per lane (south, centre, north), each p' row is read
// (kJsRows + 2) / kJsRows times from L2.  The early exit at p_tol is decided on
// the device: every launch after the converged iteration folds that
// iteration's residual slots and returns at once (the red-black SOR's
// predicate).  Every operation is a separate IEEE double operation in the
// script's order (-ffp-contract=off); one rounding to f32 on the store.
//
// F64 (k_jacobi_script_f64, cfd_script_options.residual_f64): the same body
// with the maximum kept as the script's double.  A wave raises set `it` of
// res64 with it and publishes (float) of it into err_slots as the other
// instantiation publishes its f32 maximum: rounding is monotone, so that is
// the same f32, and the exit test above and the finalize read it unchanged.
#include "cfd_device.h"

#include <type_traits>

namespace cfd {
namespace {

constexpr int kJsRows = 4;   // interior rows per wave

template <int FAST>
__device__ __forceinline__ float js_relax(const SorConst &k, float c, float e, float w, float n,
                                          float s, float rh) {
    const double old = (double)c;
    const double h = ddiv<FAST>((double)e + (double)w, k.dx2, k.r_dx2);
    const double v = ddiv<FAST>((double)n + (double)s, k.dy2, k.r_dy2);
    const double p_update = ddiv<FAST>(h + v - (double)rh, k.denom, k.r_denom);
    const double omega = 0.7;
    return (float)(omega * p_update + (1.0 - omega) * old);
}

// :817 on the stored values; a NaN difference is ignored (fmaxf) as `>` ignores it
__device__ __forceinline__ float js_err(float m, float nv, float old) {
    return fmaxf(m, (float)fabs((double)nv - (double)old));
}
__device__ __forceinline__ double js_err(double m, float nv, float old) {
    return fmax(m, fabs((double)nv - (double)old));
}

__device__ __forceinline__ float2 js_ld(const float *__restrict__ p, long off, bool on) {
    return on ? *reinterpret_cast<const float2 *>(p + off) : make_float2(0.0f, 0.0f);
}

template <int FAST, int F64>
__device__ __forceinline__ void jacobi_script_body(const float *__restrict__ pa,
                                                   const float *__restrict__ pb,
                                                   float *__restrict__ qa, float *__restrict__ qb,
                                                   const float *__restrict__ rhs, int nx, int ny,
                                                   const SorConst &k, Ctl *ctl, uint32_t *err_slots,
                                                   int pass, int it, int tol, float p_tol, int res,
                                                   int nwc, int nseg, unsigned long long *res64) {
    typedef typename std::conditional<F64 != 0, double, float>::type acc_t;
    // :836, decided here: the previous iteration was the solve's last
    if (tol && it > 0 &&
        read_max(err_slots + (size_t)(it - 1) * kResSlots * kResStride, ctl->err[it - 1]) < p_tol)
        return;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = (int)threadIdx.x & 63;
    const int bid = (int)blockIdx.x;
    const int wc = bid % nwc;
    const int seg = (bid / nwc) * (kBlock / 64) + wave;
    if (seg >= nseg) return;   // wave-uniform
    const int si = (ctl->cur + it) & 1;
    const float *__restrict__ src = si ? pb : pa;
    float *__restrict__ dst = si ? qa : qb;
    const int c = wc * 62 - 1 + lane;
    const int i0 = 2 * c;
    const bool in_dom = c >= 0 && i0 < nx;             // nx is even: the pair is inside
    const bool out = in_dom && lane >= 1 && lane <= 62;
    const bool rd = in_dom && it > 0;
    const int r0 = 1 + seg * kJsRows;
    const int r1 = min(r0 + kJsRows, ny - 1);          // interior rows [r0, r1), r0 < r1 <= ny-1
    float2 dn = js_ld(src, (long)(r0 - 1) * nx + i0, rd), a = js_ld(src, (long)r0 * nx + i0, rd);
    acc_t m = 0;
#pragma unroll
    for (int t = 0; t < kJsRows; ++t) {
        const int j = r0 + t;
        if (j >= r1) break;   // wave-uniform
        const float2 up = js_ld(src, (long)(j + 1) * nx + i0, rd);   // j + 1 <= ny - 1
        const float2 rh = js_ld(rhs, (long)j * nx + i0, in_dom);
        // every lane shifts (halo and out-of-domain lanes hold zeros)
        const float w_of_x = from_left(a.y), e_of_y = from_right(a.x);
        float2 o = a;
        acc_t mm = 0;
        if (i0 >= 1) {
            o.x = js_relax<FAST>(k, a.x, a.y, w_of_x, up.x, dn.x, rh.x);
            mm = js_err(mm, o.x, a.x);
        }
        if (i0 + 1 <= nx - 2) {
            o.y = js_relax<FAST>(k, a.y, e_of_y, a.x, up.y, dn.y, rh.y);
            mm = js_err(mm, o.y, a.y);
        }
        if (i0 == 0) o.x = o.y;            // :833 P(0,j) = P(1,j)
        if (i0 + 1 == nx - 1) o.y = 0.0f;  // :834 P(nx-1,j) = 0
        if (out) {
            m = acc_max(m, mm);
            *reinterpret_cast<float2 *>(dst + (long)j * nx + i0) = o;
            if (j == 1) *reinterpret_cast<float2 *>(dst + i0) = o;                               // :829 row 0
            if (j == ny - 2) *reinterpret_cast<float2 *>(dst + (long)(ny - 1) * nx + i0) = o;   // :830 row ny-1
        }
        dn = a;
        a = up;
    }
    if (!res) return;
    if (F64) {
        const double md = wave_max_pos_f64((double)m);
        if (lane == 0) {
            const int key = bid * (kBlock / 64) + wave;
            publish_max_pos_f64(res64 + (size_t)it * kResSlots * kRes64Stride, key, md);
            publish_max(err_slots + (size_t)it * kResSlots * kResStride, key, (float)md);
        }
        return;
    }
    const float mf = wave_max((float)m);
    if (lane == 0) publish_max(err_slots + (size_t)it * kResSlots * kResStride, bid * (kBlock / 64) + wave, mf);
}

template <int FAST>
__global__ __launch_bounds__(kBlock) void k_jacobi_script(const float *__restrict__ pa,
                                                          const float *__restrict__ pb,
                                                          float *__restrict__ qa, float *__restrict__ qb,
                                                          const float *__restrict__ rhs, int nx, int ny,
                                                          SorConst k, Ctl *ctl, uint32_t *err_slots,
                                                          int pass, int it, int tol, float p_tol,
                                                          int res, int nwc, int nseg) {
    if (pass_off(ctl, pass)) return;
    jacobi_script_body<FAST, 0>(pa, pb, qa, qb, rhs, nx, ny, k, ctl, err_slots, pass, it, tol, p_tol, res,
                                nwc, nseg, nullptr);
}

template <int FAST>
__global__ __launch_bounds__(kBlock) void k_jacobi_script_f64(
    const float *__restrict__ pa, const float *__restrict__ pb, float *__restrict__ qa,
    float *__restrict__ qb, const float *__restrict__ rhs, int nx, int ny, SorConst k, Ctl *ctl,
    uint32_t *err_slots, int pass, int it, int tol, float p_tol, int res, int nwc, int nseg,
    unsigned long long *res64) {
    if (pass_off(ctl, pass)) return;
    jacobi_script_body<FAST, 1>(pa, pb, qa, qb, rhs, nx, ny, k, ctl, err_slots, pass, it, tol, p_tol, res,
                                nwc, nseg, res64);
}

}  // namespace

void launch_jacobi_script(float *pa, float *pb, const float *rhs, int nx, int ny, const SorConst &k,
                          Ctl *ctl, uint32_t *err_slots, int pass, int it, int tol, float p_tol,
                          int res, hipStream_t s, unsigned long long *res64) {
    const int nwc = cdiv(nx / 2, 62);
    const int nseg = cdiv(ny - 2, kJsRows);
    const dim3 grid(nwc * cdiv(nseg, kBlock / 64));
    if (res64 && k.fast)
        hipLaunchKernelGGL(k_jacobi_script_f64<1>, grid, dim3(kBlock), 0, s, pa, pb, pa, pb, rhs, nx, ny,
                           k, ctl, err_slots, pass, it, tol, p_tol, res, nwc, nseg, res64);
    else if (res64)
        hipLaunchKernelGGL(k_jacobi_script_f64<0>, grid, dim3(kBlock), 0, s, pa, pb, pa, pb, rhs, nx, ny,
                           k, ctl, err_slots, pass, it, tol, p_tol, res, nwc, nseg, res64);
    else if (k.fast)
        hipLaunchKernelGGL(k_jacobi_script<1>, grid, dim3(kBlock), 0, s, pa, pb, pa, pb, rhs, nx, ny, k,
                           ctl, err_slots, pass, it, tol, p_tol, res, nwc, nseg);
    else
        hipLaunchKernelGGL(k_jacobi_script<0>, grid, dim3(kBlock), 0, s, pa, pb, pa, pb, rhs, nx, ny, k,
                           ctl, err_slots, pass, it, tol, p_tol, res, nwc, nseg);
}

}  // namespace cfd
