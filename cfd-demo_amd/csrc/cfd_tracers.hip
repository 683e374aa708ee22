// cfd_tracers.hip — the script's tracer particles (index.html:1472-1543) on
// the device: a Lagrangian pass over u, v once per step, plus the cull of the
// tracers that left the domain as a stable (order-preserving) compaction.
//
// Arithmetic follows getVelocityAt / updateTracers operation for operation in
// double (u, v widened on load), nothing contracted; division and floor are
// correctly rounded.  The clamps of :1504-1507 are applied to the double before
// it becomes an int, as the script clamps values no int holds.
//
// A tracer step is two launches whose arguments never change:
//   k_trc_advect   every lane moves one tracer in place (x, y; initialY is not
//                  touched) and forms the keep predicate; a wave ballot and an
//                  LDS sum give the survivors of each tile of kTrcBlock
//                  tracers.  Workgroups take a ticket as they finish; the one
//                  that draws the last ticket scans the tile counts and
//                  decides the injection.  A ticket is not a wait: no
//                  workgroup ever spins on another.
//   k_trc_scatter  survivors go to tile offset + rank within the tile in the
//                  other buffer, the injected tracers after them, and the new
//                  count and buffer index are written.
// Grids are sized from the capacity; workgroups past the device-side count
// leave at once, the others stride over the tiles.
#include "cfd_device.h"

#pragma clang fp contract(off)

namespace cfd {
namespace {

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

struct Vel {
    double u, v;
};

// getVelocityAt (index.html:1499-1525); x, y finite
__device__ __forceinline__ Vel velocity_at(const float *__restrict__ u, const float *__restrict__ v,
                                           int nx, int ny, double dx, double dy, double x, double y) {
    double fi = floor(x / dx);
    double fj = floor(y / dy);
    if (fi < 0.0) fi = 0.0;
    if (fi > (double)(nx - 2)) fi = (double)(nx - 2);
    if (fj < 0.0) fj = 0.0;
    if (fj > (double)(ny - 2)) fj = (double)(ny - 2);
    if (!(fi == fi)) fi = 0.0;   // never with finite x (cfd_tracers_set rejects the rest):
    if (!(fj == fj)) fj = 0.0;   // keeps every index in bounds all the same
    const double rx = (x - fi * dx) / dx;
    const double ry = (y - fj * dy) / dy;
    const int i = (int)fi, j = (int)fj;
    const long W = nx + 1;
    const float *ur0 = u + (long)j * W + i, *ur1 = ur0 + W;
    const float *vr0 = v + (long)j * nx + i, *vr1 = vr0 + nx, *vr2 = vr1 + nx;
    // cellCenterVelocity(i, j), (i+1, j), (i, j+1), (i+1, j+1)
    const double u00 = 0.5 * ((double)ur0[0] + (double)ur0[1]);
    const double u10 = 0.5 * ((double)ur0[1] + (double)ur0[2]);
    const double u01 = 0.5 * ((double)ur1[0] + (double)ur1[1]);
    const double u11 = 0.5 * ((double)ur1[1] + (double)ur1[2]);
    const double v00 = 0.5 * ((double)vr0[0] + (double)vr1[0]);
    const double v10 = 0.5 * ((double)vr0[1] + (double)vr1[1]);
    const double v01 = 0.5 * ((double)vr1[0] + (double)vr2[0]);
    const double v11 = 0.5 * ((double)vr1[1] + (double)vr2[1]);
    Vel r;
    r.u = (1.0 - rx) * ((1.0 - ry) * u00 + ry * u01) + rx * ((1.0 - ry) * u10 + ry * u11);
    r.v = (1.0 - rx) * ((1.0 - ry) * v00 + ry * v01) + rx * ((1.0 - ry) * v10 + ry * v11);
    return r;
}

// updateTracers' test (:1492): NaN fails it, -0 and exactly Lx pass
__device__ __forceinline__ bool inside(double x, double y, double lx, double ly) {
    return x >= 0.0 && x <= lx && y >= 0.0 && y <= ly;
}

__device__ __forceinline__ uint32_t tiles_of(uint32_t n) { return (n + kTrcBlock - 1) / kTrcBlock; }

__global__ __launch_bounds__(kTrcBlock) void k_trc_advect(Geom g, const float *__restrict__ u,
                                                          const float *__restrict__ v, const Ctl *ctl,
                                                          Tracers t, int in_step, double dt_arg) {
    __shared__ uint32_t s_w[kTrcBlock / 64];
    __shared__ uint32_t s_last;
    TrcCtl *tc = t.tc;
    // count / cur are not written by this launch (k_trc_scatter does)
    const uint32_t n = tc->count, cur = tc->cur;
    const uint32_t ntiles = tiles_of(n);
    const uint32_t nact = min((uint32_t)gridDim.x, max(ntiles, 1u));
    if (blockIdx.x >= nact) return;
    double *X = cur ? t.x1 : t.x0, *Y = cur ? t.y1 : t.y0;
    const double dt = in_step ? (double)ctl->dt : dt_arg;
    const int tid = (int)threadIdx.x, wave = tid >> 6;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t idx = tile * kTrcBlock + tid;
        bool keep = false;
        if (idx < n) {
            double x = X[idx], y = Y[idx];
            const Vel vel = velocity_at(u, v, g.nx, g.ny, t.dx, t.dy, x, y);
            x += dt * vel.u;
            y += dt * vel.v;
            X[idx] = x;
            Y[idx] = y;
            keep = inside(x, y, t.lx, t.ly);
        }
        const unsigned long long b = __ballot(keep);
        if ((tid & 63) == 0) s_w[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        if (tid == 0) {
            uint32_t c = 0;
            for (int w = 0; w < kTrcBlock / 64; ++w) c += s_w[w];
            __hip_atomic_store(&t.tile_cnt[tile], c, RLX_AGENT);   // read by the last workgroup
        }
        __syncthreads();
    }
    if (tid == 0) {
        // release: this workgroup's tile counts; acquire: everybody's, if last
        const uint32_t k = __hip_atomic_fetch_add(&tc->ticket, 1u, __ATOMIC_ACQ_REL,
                                                  __HIP_MEMORY_SCOPE_AGENT);
        s_last = k == nact - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last) return;

    // the last workgroup: exclusive scan of the tile counts (every count is
    // loaded at agent scope, past this CU's L1)
    const uint32_t per = (ntiles + kTrcBlock - 1) / kTrcBlock;
    const uint32_t t0 = min((uint32_t)tid * per, ntiles), t1 = min(t0 + per, ntiles);
    uint32_t mine = 0;
    for (uint32_t k = t0; k < t1; ++k) mine += __hip_atomic_load(&t.tile_cnt[k], RLX_AGENT);
    uint32_t inc = mine;   // inclusive scan over the wave, then over the waves
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)inc, o, 64);
        if ((tid & 63) >= o) inc += up;
    }
    if ((tid & 63) == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t run = inc - mine, total = 0;
    for (int w = 0; w < kTrcBlock / 64; ++w) {
        if (w < wave) run += s_w[w];
        total += s_w[w];
    }
    for (uint32_t k = t0; k < t1; ++k) {
        t.tile_off[k] = run;
        run += __hip_atomic_load(&t.tile_cnt[k], RLX_AGENT);
    }
    if (tid == 0) {
        uint32_t inject = in_step && (ctl->step % t.interval == 0u) ? 1u : 0u;
        if (inject && (uint64_t)total + (uint64_t)g.ny > (uint64_t)t.cap) {
            tc->overflow = 1u;
            inject = 0u;
        }
        tc->n_prev = n;
        tc->src = cur;
        tc->total = total;
        tc->do_inject = inject;
        __hip_atomic_store(&tc->ticket, 0u, RLX_AGENT);
    }
}

__global__ __launch_bounds__(kTrcBlock) void k_trc_scatter(Tracers t, int ny) {
    __shared__ uint32_t s_w[kTrcBlock / 64];
    TrcCtl *tc = t.tc;
    // written by the launch before this one; count / cur are not read here
    const uint32_t n = tc->n_prev, src = tc->src, total = tc->total, inject = tc->do_inject;
    const uint32_t ntiles = tiles_of(n);
    const uint32_t work = max(max(ntiles, inject ? tiles_of((uint32_t)ny) : 0u), 1u);
    if (blockIdx.x >= work) return;
    const double *X = src ? t.x1 : t.x0, *Y = src ? t.y1 : t.y0, *I = src ? t.i1 : t.i0;
    double *DX = src ? t.x0 : t.x1, *DY = src ? t.y0 : t.y1, *DI = src ? t.i0 : t.i1;
    const int tid = (int)threadIdx.x, wave = tid >> 6;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t idx = tile * kTrcBlock + tid;
        double x = 0.0, y = 0.0;
        bool keep = false;
        if (idx < n) {
            x = X[idx];
            y = Y[idx];
            keep = inside(x, y, t.lx, t.ly);
        }
        const unsigned long long b = __ballot(keep);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32),
                                                        __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        if ((tid & 63) == 0) s_w[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t off = t.tile_off[tile] + rank;
        for (int w = 0; w < wave; ++w) off += s_w[w];
        if (keep) {   // off < total <= n <= cap
            DX[off] = x;
            DY[off] = y;
            DI[off] = I[idx];
        }
        __syncthreads();
    }
    if (inject)   // injectTracers (:1537-1543); total + ny <= cap was checked
        for (uint32_t j = blockIdx.x * kTrcBlock + tid; j < (uint32_t)ny; j += gridDim.x * kTrcBlock) {
            const double y = ((double)j + 0.5) * t.dy;
            DX[total + j] = 0.0;
            DY[total + j] = y;
            DI[total + j] = y;
        }
    if (blockIdx.x == 0 && tid == 0) {
        tc->count = total + (inject ? (uint32_t)ny : 0u);
        tc->cur = src ^ 1u;
    }
}

// One workgroup: nobody reads the count while it changes.
__global__ __launch_bounds__(kTrcBlock) void k_trc_inject(Tracers t, int ny) {
    TrcCtl *tc = t.tc;
    const uint32_t n = tc->count, cur = tc->cur;
    __syncthreads();
    if ((uint64_t)n + (uint64_t)ny > (uint64_t)t.cap) {
        if (threadIdx.x == 0) tc->overflow = 1u;
        return;
    }
    double *X = cur ? t.x1 : t.x0, *Y = cur ? t.y1 : t.y0, *I = cur ? t.i1 : t.i0;
    for (uint32_t j = threadIdx.x; j < (uint32_t)ny; j += kTrcBlock) {
        const double y = ((double)j + 0.5) * t.dy;
        X[n + j] = 0.0;
        Y[n + j] = y;
        I[n + j] = y;
    }
    if (threadIdx.x == 0) tc->count = n + (uint32_t)ny;
}

// floor(x / dx), floor(y / dy) clipped to the grid; integer atomics: exact in any order
__global__ __launch_bounds__(kTrcBlock) void k_trc_density(Tracers t, int nx, int ny,
                                                           uint32_t *__restrict__ counts) {
    const TrcCtl *tc = t.tc;
    const uint32_t n = tc->count, cur = tc->cur;
    const double *X = cur ? t.x1 : t.x0, *Y = cur ? t.y1 : t.y0;
    for (uint32_t idx = blockIdx.x * kTrcBlock + threadIdx.x; idx < n; idx += gridDim.x * kTrcBlock) {
        double fi = floor(X[idx] / t.dx), fj = floor(Y[idx] / t.dy);
        if (!(fi >= 0.0)) fi = 0.0;
        if (fi > (double)(nx - 1)) fi = (double)(nx - 1);
        if (!(fj >= 0.0)) fj = 0.0;
        if (fj > (double)(ny - 1)) fj = (double)(ny - 1);
        atomicAdd(&counts[(size_t)(int)fj * (size_t)nx + (size_t)(int)fi], 1u);
    }
}

}  // namespace

void launch_trc_step(const Geom &g, const Fields &f, const Tracers &t, int grid, bool in_step,
                     double dt, hipStream_t s) {
    hipLaunchKernelGGL(k_trc_advect, dim3(grid), dim3(kTrcBlock), 0, s, g, (const float *)f.u,
                       (const float *)f.v, (const Ctl *)f.ctl, t, in_step ? 1 : 0, dt);
    hipLaunchKernelGGL(k_trc_scatter, dim3(grid), dim3(kTrcBlock), 0, s, t, g.ny);
}

void launch_trc_inject(const Geom &g, const Tracers &t, hipStream_t s) {
    hipLaunchKernelGGL(k_trc_inject, dim3(1), dim3(kTrcBlock), 0, s, t, g.ny);
}

void launch_trc_density(const Geom &g, const Tracers &t, int grid, uint32_t *counts, hipStream_t s) {
    hipLaunchKernelGGL(k_trc_density, dim3(grid), dim3(kTrcBlock), 0, s, t, g.nx, g.ny, counts);
}

}  // namespace cfd
