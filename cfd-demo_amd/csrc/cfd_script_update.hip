// cfd_script_update.hip — the device passes of one updateSimulation()
// (index.html:261-363) around its substeps, for cfd_script_update:
//   k_script_begin  :263-274  u = 2u - uPrev, v = 2v - vPrev (step > 0), then
//                             uOld = u, vOld = v: u and uPrev read once, u and
//                             uOld written;
//   k_script_pmax   :290-292  the running maximum of the substeps' pressure
//                             residuals, one word folded after each solve;
//   k_script_pmax64           the same on the doubles the solves publish under
//                             cfd_script_options.residual_f64, in its place;
//   k_script_end    :296-305, :1323-1333, :361-362  max |u - uOld|,
//                             max |v - vOld|, max(|u|, |v|) and uPrev = u,
//                             vPrev = v in one pass over u, v, uOld, vOld.
// Arithmetic is the script's: double on the f32 values widened, one rounding
// per store.  The three maxima stay doubles: a non-negative double orders as
// its 64 bits, so each is a 64-bit atomicMax on kResSlots spread words (one
// 64-byte line each); the host folds the slots after its one read-back.  A NaN
// never enters a maximum, as the script's `>` never takes it.
#include "cfd_device.h"

namespace cfd {
namespace {

constexpr int kSuPer = 4;   // elements per thread

__global__ __launch_bounds__(kBlock) void k_script_begin(float *__restrict__ u,
                                                         const float *__restrict__ u_prev,
                                                         float *__restrict__ u_old, long nu,
                                                         float *__restrict__ v,
                                                         const float *__restrict__ v_prev,
                                                         float *__restrict__ v_old, long nv,
                                                         int extrapolate) {
    const long base = ((long)blockIdx.x * kBlock) * kSuPer + threadIdx.x;
#pragma unroll
    for (int e = 0; e < kSuPer; ++e) {
        long i = base + (long)e * kBlock;
        if (i >= nu + nv) break;
        float *f = u, *o = u_old;
        const float *pv = u_prev;
        if (i >= nu) {
            i -= nu;
            f = v;
            o = v_old;
            pv = v_prev;
        }
        float x = f[i];
        if (extrapolate) {
            x = (float)(2.0 * (double)x - (double)pv[i]);   // :265, :268
            f[i] = x;
        }
        o[i] = x;   // :273-274
    }
}

__device__ __forceinline__ double wave_max_f64(double m) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double t = __shfl_xor(m, o, 64);
        m = t > m ? t : m;
    }
    return m;
}

__device__ __forceinline__ void publish_max_f64(unsigned long long *set, int key, double m) {
    if (m > 0.0)
        atomicMax(&set[(size_t)(key & (kResSlots - 1)) * kScrRedStride],
                  (unsigned long long)__double_as_longlong(m));
}

__global__ __launch_bounds__(kBlock) void k_script_end(const float *__restrict__ u,
                                                       const float *__restrict__ u_old,
                                                       float *__restrict__ u_prev, long nu,
                                                       const float *__restrict__ v,
                                                       const float *__restrict__ v_old,
                                                       float *__restrict__ v_prev, long nv,
                                                       unsigned long long *__restrict__ red) {
    const long base = ((long)blockIdx.x * kBlock) * kSuPer + threadIdx.x;
    double mu = 0.0, mv = 0.0, mvel = 0.0;
#pragma unroll
    for (int e = 0; e < kSuPer; ++e) {
        const long i = base + (long)e * kBlock;
        if (i >= nu + nv) break;
        if (i < nu) {
            const float x = u[i];
            const double d = fabs((double)x - (double)u_old[i]);   // :299
            if (d > mu) mu = d;
            const double a = fabs((double)x);                      // :1326
            if (a > mvel) mvel = a;
            u_prev[i] = x;                                         // :361
        } else {
            const long k = i - nu;
            const float x = v[k];
            const double d = fabs((double)x - (double)v_old[k]);   // :303
            if (d > mv) mv = d;
            const double a = fabs((double)x);                      // :1331
            if (a > mvel) mvel = a;
            v_prev[k] = x;                                         // :362
        }
    }
    mu = wave_max_f64(mu);
    mv = wave_max_f64(mv);
    mvel = wave_max_f64(mvel);
    if ((threadIdx.x & 63) == 0) {
        const int key = (int)blockIdx.x * (kBlock / 64) + ((int)threadIdx.x >> 6);
        publish_max_f64(red + (size_t)0 * kResSlots * kScrRedStride, key, mu);
        publish_max_f64(red + (size_t)1 * kResSlots * kScrRedStride, key, mv);
        publish_max_f64(red + (size_t)2 * kResSlots * kScrRedStride, key, mvel);
    }
}

// lastPResidual > maxPressureResidual (:290): the solve's finalize left the
// residual in Ctl::last_p; a NaN is not taken
__global__ void k_script_pmax(const Ctl *__restrict__ ctl, unsigned long long *__restrict__ red) {
    float *pm = reinterpret_cast<float *>(red + kScrRedPmax);
    const float r = ctl->last_p;
    if (r > *pm) *pm = r;
}

// its sibling for solves that publish the script's double (Ctl::last_p64): the
// same comparison on doubles, into the line's second 64-bit word
__global__ void k_script_pmax64(const Ctl *__restrict__ ctl, unsigned long long *__restrict__ red) {
    double *pm = reinterpret_cast<double *>(red + kScrRedPmax + 1);
    const double r = ctl->last_p64;
    if (r > *pm) *pm = r;
}

}  // namespace

void launch_script_begin(const Fields &f, float *u_prev, float *u_old, float *v_prev, float *v_old,
                         long nu, long nv, int extrapolate, hipStream_t s) {
    const int grid = cdiv(nu + nv, (long)kBlock * kSuPer);
    hipLaunchKernelGGL(k_script_begin, dim3(grid), dim3(kBlock), 0, s, f.u, u_prev, u_old, nu, f.v,
                       v_prev, v_old, nv, extrapolate);
}

void launch_script_end(const Fields &f, float *u_prev, const float *u_old, float *v_prev,
                       const float *v_old, long nu, long nv, unsigned long long *red, hipStream_t s) {
    const int grid = cdiv(nu + nv, (long)kBlock * kSuPer);
    hipLaunchKernelGGL(k_script_end, dim3(grid), dim3(kBlock), 0, s, f.u, u_old, u_prev, nu, f.v, v_old,
                       v_prev, nv, red);
}

void launch_script_pmax(const Fields &f, unsigned long long *red, hipStream_t s) {
    hipLaunchKernelGGL(k_script_pmax, dim3(1), dim3(1), 0, s, f.ctl, red);
}

void launch_script_pmax64(const Fields &f, unsigned long long *red, hipStream_t s) {
    hipLaunchKernelGGL(k_script_pmax64, dim3(1), dim3(1), 0, s, f.ctl, red);
}

}  // namespace cfd
