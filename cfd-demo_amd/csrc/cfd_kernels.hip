// cfd_kernels.hip — CDNA4 (gfx950) kernels for cfd-demo's Model::update hot path:
// the step's copies, the separate predictors and divergence, the one-sweep
// Jacobi with the solve's finalize and speculative helpers, the velocity
// boundaries, the step reduce and finalize.  The correctors are
// cfd_correct.hip, the fused predictor march cfd_predict_march.hip, the
// blocked Jacobi marches cfd_jacobi_*.hip.
//
// Every kernel reproduces the reference's f32 arithmetic bit for bit: the
// file is compiled with -ffp-contract=off (Rust never fuses a*b+c), `/` is
// HIP's default correctly-rounded f32 division, denormals are kept, and each
// expression keeps the reference's evaluation order.  Maxima are exact and
// order-independent, so the reductions (wave shuffles + one atomicMax on the
// f32 bit pattern of a non-negative value) are deterministic.
//
// Citations are /root/reference/src/model.rs line numbers.
#include "cfd_device.h"
#include "cfd_predict.h"

namespace cfd {

namespace {
// Exhaustive proof of the fast forms for one divisor c (r = RN(1/c)):
// counts inputs x where x*r (mode 1) or the corrected form (mode 2) differs
// from IEEE x/c; NaN results compare equal to NaN.
__global__ __launch_bounds__(kBlock) void k_verify_division(float c, float r,
                                                            unsigned long long *counts) {
    const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t bad1 = 0, bad2 = 0, bad3 = 0;
    for (uint64_t k = tid; k < (1ull << 32); k += stride) {
        const float x = __uint_as_float((uint32_t)k);
        const float ref = x / c;
        const float m1 = fdiv<1>(x, c, r);
        const float m2 = fdiv<2>(x, c, r);
        const float m3 = fdiv<3>(x, c, r);
        const bool rn = ref != ref;
        bad1 += (rn ? (m1 == m1) : (__float_as_uint(m1) != __float_as_uint(ref))) ? 1u : 0u;
        bad2 += (rn ? (m2 == m2) : (__float_as_uint(m2) != __float_as_uint(ref))) ? 1u : 0u;
        bad3 += (rn ? (m3 == m3) : (__float_as_uint(m3) != __float_as_uint(ref))) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bad1 += __shfl_xor(bad1, o, 64);
        bad2 += __shfl_xor(bad2, o, 64);
        bad3 += __shfl_xor(bad3, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (bad1) atomicAdd(&counts[0], (unsigned long long)bad1);
        if (bad2) atomicAdd(&counts[1], (unsigned long long)bad2);
        if (bad3) atomicAdd(&counts[2], (unsigned long long)bad3);
    }
}

// ------------------------------------------------------------- copies (K0/K5b)

__device__ __forceinline__ void copy4(float *__restrict__ dst, const float *__restrict__ src,
                                      size_t n4, size_t tid, size_t stride) {
    const float4 *s = reinterpret_cast<const float4 *>(src);
    float4 *d = reinterpret_cast<float4 *>(dst);
    for (size_t k = tid; k < n4; k += stride) d[k] = s[k];
}

// update() prologue (model.rs:307-316): u_old <- u, v_old <- v, inlet ramp.
// With `copy` 0 (the fused corrector computes the residuals from the values it
// overwrites) only the control words are touched.
__global__ __launch_bounds__(kBlock) void k_step_begin(Geom g, Fields f, int copy) {
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    if (copy) {
        copy4(f.u_old_base, f.u_alloc_base, f.u_alloc / 4, tid, stride);
        copy4(f.v_old_base, f.v_alloc_base, f.v_alloc / 4, tid, stride);
    }
    if (tid == 0) {
        Ctl *c = f.ctl;
        const uint32_t st = c->step;
        // (simulation_step as f32 / ramp_up_steps as f32) * target (model.rs:311-316)
        c->inlet = st < 100u ? ((float)st / 100.0f) * g.target_inlet : g.target_inlet;
        c->go[0] = 1;
    }
}

// u_star <- u, v_star <- v before each extra correction pass (model.rs:698-699).
__global__ __launch_bounds__(kBlock) void k_copy_star(Fields f, int pass) {
    if (pass_off(f.ctl, pass)) return;
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    copy4(f.u_star_base, f.u_alloc_base, f.u_alloc / 4, tid, stride);
    copy4(f.v_star_base, f.v_alloc_base, f.v_alloc / 4, tid, stride);
}

// Predictor face arithmetic (u_pred_val / v_pred_val) and GAcc: cfd_predict.h.

template <int SCHEME, int SP>
__global__ __launch_bounds__(kBlock) void k_u_predictor(Geom g, Fields f, float dt_override,
                                                        int row_lo, int nbx) {
    const int bid = xcd_block(g);
    const int i = 1 + (bid % nbx) * kBlock + (int)threadIdx.x;
    const int lj = row_lo + bid / nbx;
    if (i > g.nx) return;
    const GAcc a{f.u, f.v, (long)lj * (g.nx + 1) + i, (long)lj * g.nx + i, g.nx + 1, g.nx};
    f.u_star[(long)lj * (g.nx + 1) + i] = u_pred_val<SCHEME, SP>(g, f, dt_of(f.ctl, dt_override), i, lj, a);
}


template <int SCHEME, int SP>
__global__ __launch_bounds__(kBlock) void k_v_predictor(Geom g, Fields f, float dt_override,
                                                        int row_lo, int nbx) {
    const int bid = xcd_block(g);
    const int i = 1 + (bid % nbx) * kBlock + (int)threadIdx.x;
    const int lj = row_lo + bid / nbx;
    if (i > g.nx - 1) return;
    const GAcc a{f.u, f.v, (long)lj * (g.nx + 1) + i, (long)lj * g.nx + i, g.nx + 1, g.nx};
    f.v_star[(long)lj * g.nx + i] = v_pred_val<SCHEME, SP>(g, f, dt_of(f.ctl, dt_override), i, lj, a);
}

// Both predictors in one pass (piso_step's K1 + K2): each thread computes the
// u face and the v face at (i, lj), sharing the u / v loads through L1; u rows
// run to u_hi, v rows to v_hi (v also covers the slab's top face row).  Same
// values as the two single kernels (one launch and one pass over u, v less).
// Measured alternatives on the bench workload (r1): 4 columns per thread
// with strided scalar loads 185 us, an LDS-staged 256 x 16 tile 147 us,
// this form 113 us.
template <int SCHEME, int SP>
__global__ __launch_bounds__(kBlock) void k_predict(Geom g, Fields f, float dt_override, int row_lo,
                                                    int u_hi, int v_hi, int nbx) {
    const int bid = xcd_block(g);
    const int i = 1 + (bid % nbx) * kBlock + (int)threadIdx.x;
    const int lj = row_lo + bid / nbx;
    const GAcc a{f.u, f.v, (long)lj * (g.nx + 1) + i, (long)lj * g.nx + i, g.nx + 1, g.nx};
    if (lj <= u_hi && i <= g.nx)
        f.u_star[(long)lj * (g.nx + 1) + i] = u_pred_val<SCHEME, SP>(g, f, dt_of(f.ctl, dt_override), i, lj, a);
    if (lj <= v_hi && i <= g.nx - 1)
        f.v_star[(long)lj * g.nx + i] = v_pred_val<SCHEME, SP>(g, f, dt_of(f.ctl, dt_override), i, lj, a);
}

// Both first-order predictors with four columns per thread (i0 = 4t): the
// pitch-nx v rows move as float4 (v row lj-1, lj, lj+1 and the v* store), the
// pitch-(nx+1) u rows as scalars, and each value is loaded once for the eight
// faces it feeds (u_pred_val / v_pred_val over an RAccN, so the arithmetic is
// the single-face kernel's, bit for bit).  Face 0 and column 0 are not
// predicted (model.rs:538, :586); the thread owning columns nx-4..nx-1 also
// predicts u face nx, through the flat-indexed GAcc (its east and north
// neighbours wrap to the next row, Q1-Q3).  Requires 16-byte aligned v and
// v* rows (checked by the launcher).
// Each thread takes RPT = 2 consecutive rows (96 vs 104 us for one row and
// 107 for four, r1): the window of u and v rows
// lj-1 .. lj+RPT is loaded up front (every load in flight at once, and the
// rows shared by neighbouring output rows loaded once), then the 8 x RPT
// faces are computed with the same u_pred_val / v_pred_val arithmetic.
// Rows past the last row a predictor needs are clamped to it (their values
// are never used), so no load leaves the allocation.
struct RAccN {
    const float (*ur)[6];
    const float (*vr)[6];
    int q;
    __device__ __forceinline__ float U(int di, int dj) const { return ur[dj + 1][q + 1 + di]; }
    __device__ __forceinline__ float V(int di, int dj) const { return vr[dj + 1][q + 1 + di]; }
};

template <int SP, int RPT>
__global__ __launch_bounds__(kBlock) void k_predict4r(Geom g, Fields f, float dt_override,
                                                      int row_lo, int u_hi, int v_hi, int nbx) {
    const int bid = xcd_block(g);
    const int i0 = 4 * ((bid % nbx) * kBlock + (int)threadIdx.x);
    const int lj0 = row_lo + (bid / nbx) * RPT;
    const int nx = g.nx, W = nx + 1;
    if (i0 >= nx) return;
    const float dtv = dt_of(f.ctl, dt_override);   // once: a per-face reload waits on every load
    const float *__restrict__ u = f.u;
    const float *__restrict__ v = f.v;
    const int u_cap = u_hi + 1 > v_hi ? u_hi + 1 : v_hi;   // last u row any face reads
    const int v_cap = v_hi + 1;                            // last v row any face reads
    float ur[RPT + 2][6], vr[RPT + 2][6];
#pragma unroll
    for (int r = 0; r < RPT + 2; ++r) {
        const int ru = min(lj0 - 1 + r, u_cap), rv = min(lj0 - 1 + r, v_cap);
        const long ku = (long)ru * W + i0, kv = (long)rv * nx + i0;
        const bool mid = r >= 1 && r <= RPT;   // output rows: their east/west neighbours too
        ur[r][0] = (mid && i0 > 0) ? u[ku - 1] : 0.0f;
#pragma unroll
        for (int c = 0; c < 4; ++c) ur[r][c + 1] = u[ku + c];
        ur[r][5] = mid ? u[ku + 4] : 0.0f;
        const float4 a = *reinterpret_cast<const float4 *>(v + kv);
        vr[r][1] = a.x; vr[r][2] = a.y; vr[r][3] = a.z; vr[r][4] = a.w;
        vr[r][0] = (mid && i0 > 0) ? v[kv - 1] : 0.0f;
        vr[r][5] = mid ? v[kv + 4] : 0.0f;   // column nx wraps to the next row's column 0
    }
#pragma unroll
    for (int r = 0; r < RPT; ++r) {
        const int lj = lj0 + r;
        const long ku = (long)lj * W + i0, kv = (long)lj * nx + i0;
        if (lj <= u_hi) {
            float o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                o[q] = u_pred_val<0, SP>(g, f, dtv, i0 + q, lj, RAccN{ur + r, vr + r, q});
            float *__restrict__ us = f.u_star + ku;
            if (i0 > 0) us[0] = o[0];
            us[1] = o[1];
            us[2] = o[2];
            us[3] = o[3];
            if (i0 + 4 == nx) {
                const GAcc a{f.u, f.v, ku + 4, kv + 4, W, nx};
                us[4] = u_pred_val<0, SP>(g, f, dtv, nx, lj, a);
            }
        }
        if (lj <= v_hi) {
            float o[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                o[q] = v_pred_val<0, SP>(g, f, dtv, i0 + q, lj, RAccN{ur + r, vr + r, q});
            float *__restrict__ vs = f.v_star + kv;
            if (i0 > 0) {
                *reinterpret_cast<float4 *>(vs) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
                vs[1] = o[1];
                vs[2] = o[2];
                vs[3] = o[3];
            }
        }
    }
}

// ------------------------------------------------------------ divergence (K3)

// rhs = div(u*, v*) / dt on every owned pressure cell (model.rs:1406-1440).
// A thread owns 4 consecutive cells: v* rows and the rhs row are 16-byte
// aligned (pitch nx, nx % 8 == 0) and move as float4; the u* row (pitch nx+1)
// is read as 5 scalars.  One float per thread capped this stream at ~3 TB/s.
template <int SP>
__global__ __launch_bounds__(kBlock) void k_divergence(Geom g, Fields f, int pass,
                                                       float dt_override, int nbx) {
    if (pass_off(f.ctl, pass)) return;
    const int bid = xcd_block(g);
    const int i0 = 4 * ((bid % nbx) * kBlock + (int)threadIdx.x);
    const int lj = bid / nbx;
    const int nx = g.nx, W = nx + 1;
    if (i0 >= nx) return;
    const float dt = dt_of(f.ctl, dt_override);
    const float *__restrict__ us = f.u_star + (long)lj * W + i0;
    const float4 vs = *reinterpret_cast<const float4 *>(f.v_star + (long)lj * nx + i0);
    const float4 vn = *reinterpret_cast<const float4 *>(f.v_star + (long)(lj + 1) * nx + i0);
    const float u0 = us[0], u1 = us[1], u2 = us[2], u3 = us[3], u4 = us[4];
    *reinterpret_cast<float4 *>(f.rhs + (long)lj * nx + i0) = div4<SP>(g, u0, u1, u2, u3, u4, vs, vn, dt);
}

// The head of a corrector-loop pass (model.rs:698-704): u* <- u, v* <- v and
// rhs = div(u*, v*) / dt in one pass.  The divergence is formed from the u
// and v values the copy has just read (they are the new u*, v*), so u* and v*
// are not read back: 20 B per cell instead of the 28 of k_copy_star +
// k_divergence, and one launch.  A thread owns 4 cells of one allocation row;
// ghost rows are copied too (k_copy_star copies whole allocations), owned rows
// also get rhs, with k_divergence's arithmetic bit for bit.
template <int SP>
__global__ __launch_bounds__(kBlock) void k_copy_star_div(Geom g, Fields f, int pass,
                                                          float dt_override, int nbx) {
    if (pass_off(f.ctl, pass)) return;
    const int bid = xcd_block(g);
    const int i0 = 4 * ((bid % nbx) * kBlock + (int)threadIdx.x);
    const int lr = bid / nbx - kGhostUV;   // local row: v rows -G..nyl+G, u rows -G..nyl+G-1
    const int nx = g.nx, W = nx + 1;
    if (i0 >= nx) return;
    const float4 vs = *reinterpret_cast<const float4 *>(f.v + (long)lr * nx + i0);
    *reinterpret_cast<float4 *>(f.v_star + (long)lr * nx + i0) = vs;
    if (lr >= g.nyl + kGhostUV) return;   // v's extra face row
    const float *__restrict__ ur = f.u + (long)lr * W + i0;
    float *__restrict__ us = f.u_star + (long)lr * W + i0;
    const float u0 = ur[0], u1 = ur[1], u2 = ur[2], u3 = ur[3], u4 = ur[4];
    us[0] = u0;
    us[1] = u1;
    us[2] = u2;
    us[3] = u3;
    if (i0 + 4 == nx) us[4] = u4;   // face nx
    if (lr < 0 || lr >= g.nyl) return;
    const float4 vn = *reinterpret_cast<const float4 *>(f.v + (long)(lr + 1) * nx + i0);
    const float dt = dt_of(f.ctl, dt_override);
    *reinterpret_cast<float4 *>(f.rhs + (long)lr * nx + i0) = div4<SP>(g, u0, u1, u2, u3, u4, vs, vn, dt);
}

// ---------------------------------------------------------------- Jacobi (K4)

// One weighted-Jacobi sweep (omega 0.75) with the p' boundary conditions
// fused into the stores (model.rs:748-815).
//
// Mapping: a wave owns 64 float4 column chunks (256 columns) of one row
// segment of R rows and marches up the segment, keeping rows j-1, j, j+1 in
// registers: p' and rhs are each read from HBM once per sweep, p'_new written
// once (12 B per cell-update), and horizontal neighbours come from adjacent
// lanes (__shfl) instead of re-reads.  Rows are processed 4 at a time with all
// 8 row loads of a group issued before any arithmetic.
//
// Boundary conditions, as stores (model.rs:807-815 applied after the swap):
// the reference's final values are P(0,j) = N(1,j), P(nx-1,j) = 0,
// P(i,0) = N(i,1), P(i,ny-1) = N(i,ny-2) for the freshly computed interior
// N — so column 0 takes column 1's value, column nx-1 stores 0, and the
// threads computing global rows 1 and ny-2 also store rows 0 and ny-1.
// Column nx-1's own update (which reads the wrapped P(0,j+1), Q5) is never
// stored, exactly as the reference overwrites it.
//
// Residual: max |N - P| over columns 1..=nx-8 only (the reference's full
// 8-lane chunks; the scalar tail :755-772 never updates max_error), owned
// rows only, NaN-ignoring like reduce_max.  One atomicMax per wave, into the
// sweep's spread slot set (only when `res`: a fixed-count solve needs the last
// sweep's residual alone).
template <int R, int FAST>
__global__ __launch_bounds__(kJacWavesPerBlock * 64) void k_jacobi(
    Geom g, float *__restrict__ pa, float *__restrict__ pb, const float *__restrict__ rhs,
    Ctl *ctl, uint32_t *slots, int pass, int it, int row_lo, int row_hi, int nbx, int res) {
    if (pass_off(ctl, pass)) return;
    // early exit of the previous sweep (model.rs:816): a skipped sweep leaves
    // its slots at 0 so every later sweep of the solve skips too.
    if (g.tol_enabled && it > 0 &&
        read_max(slots + (size_t)(it - 1) * kResSlots * kResStride, ctl->err[it - 1]) < g.p_tol)
        return;

    const int nx = g.nx, nch = nx >> 2, hg = g.hg, nyl = g.nyl;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int bid = xcd_block(g);
    const int bx = bid % nbx, seg = bid / nbx;
    const int wcol = bx * kJacWavesPerBlock + wave;
    if (wcol * 64 >= nch) return;                         // wave-uniform
    const int ch = wcol * 64 + lane;
    const bool valid = ch < nch;
    const int r0 = row_lo + seg * R;
    const int r1 = min(r0 + R, row_hi);
    if (r0 >= r1) return;

    // pa/pb: the two p' allocations (first ghost row); (cur + it) picks the
    // source.  Loads go through buffer descriptors: a lane with nothing to
    // load gets an out-of-range offset and reads 0 without a branch.
    const int si = (ctl->cur + it) & 1;
    float *src_alloc = si ? pb : pa;
    float *dst_alloc = si ? pa : pb;
    const int pbytes = (nyl + 2 * hg) * nx * 4;
    const __amdgpu_buffer_rsrc_t rs_p =
        __builtin_amdgcn_make_buffer_rsrc(src_alloc, 0, pbytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_r =
        __builtin_amdgcn_make_buffer_rsrc((void *)(rhs - (long)hg * nx), 0, pbytes, 0x00020000);
    float *__restrict__ dst = dst_alloc + (long)hg * nx;

    const float dx_sq = g.dx_sq, dy_sq = g.dy_sq, denom = g.denom;
    const float r_dx_sq = g.r_dx_sq, r_dy_sq = g.r_dy_sq, r_denom = g.r_denom;
    const float omega = 0.75f;
    const float om1 = 1.0f - omega;

    constexpr int kOOB = -16;   // >= num_records as unsigned: reads 0
    const int col = 4 * ch;
    const int row_bytes = nx * 4;
    // byte offsets at local row 0 (p' offsets include the hg ghost rows)
    const int off_p = valid ? (hg * nx + col) * 4 : kOOB;
    const int off_r = valid ? (hg * nx + col) * 4 : kOOB;
    const int off_l = (lane == 0 && ch > 0 && valid) ? (hg * nx + col - 1) * 4 : kOOB;
    const int off_rt = (lane == 63 && ch + 1 < nch) ? (hg * nx + col + 4) * 4 : kOOB;
    const bool e0 = (col >= 1) && (col <= nx - 8);   // residual columns 1..=nx-8
    const bool e1 = (col + 1 <= nx - 8);
    const bool e2 = (col + 2 <= nx - 8);
    const bool e3 = (col + 3 <= nx - 8);
    const int gj_first = 1 - g.j0, gj_last = g.ny - 2 - g.j0;   // local rows of global 1, ny-2

    auto ld4 = [&](const __amdgpu_buffer_rsrc_t &rs, int off, int row) -> float4 {
        const int o = off < 0 ? off : off + row * row_bytes;
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z),
                           __uint_as_float(v.w));
    };
    auto ld1 = [&](int off, int row) -> float {
        const int o = off < 0 ? off : off + row * row_bytes;
        return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs_p, o, 0, 0));
    };

    float m = 0.0f;
    // sliding window: w0..w5 = p' rows j-1 .. j+4 of the current 4-row group;
    // rows past r1 are clamped to r1 (always inside the allocation, unused)
    float4 w0 = ld4(rs_p, off_p, r0 - 1);
    float4 w1 = ld4(rs_p, off_p, r0);
    for (int j = r0; j < r1; j += 4) {
        const bool l1 = j + 1 < r1, l2 = j + 2 < r1, l3 = j + 3 < r1;
        const int j1c = l1 ? j + 1 : j, j2c = l2 ? j + 2 : j, j3c = l3 ? j + 3 : j;
        // issue every load of the group before any arithmetic
        const float4 w2 = ld4(rs_p, off_p, j + 1);
        const float4 w3 = ld4(rs_p, off_p, j1c + 1);
        const float4 w4 = ld4(rs_p, off_p, j2c + 1);
        const float4 w5 = ld4(rs_p, off_p, j3c + 1);
        const float4 h0 = ld4(rs_r, off_r, j);
        const float4 h1 = ld4(rs_r, off_r, j1c);
        const float4 h2 = ld4(rs_r, off_r, j2c);
        const float4 h3 = ld4(rs_r, off_r, j3c);
        const float lf0 = ld1(off_l, j), lf1 = ld1(off_l, j1c), lf2 = ld1(off_l, j2c),
                    lf3 = ld1(off_l, j3c);
        const float rt0 = ld1(off_rt, j), rt1 = ld1(off_rt, j1c), rt2 = ld1(off_rt, j2c),
                    rt3 = ld1(off_rt, j3c);

        auto row_update = [&](int row, const float4 &B, const float4 &C, const float4 &T,
                              const float4 &Rh, float lf, float rt) {
            const float horiz_l = __shfl_up(C.w, 1, 64);
            const float horiz_r = __shfl_down(C.x, 1, 64);
            const float L0 = (lane == 0) ? lf : horiz_l;
            const float R3 = (lane == 63) ? rt : horiz_r;
            const float cc[4] = {C.x, C.y, C.z, C.w};
            const float rr[4] = {C.y, C.z, C.w, R3};
            const float ll[4] = {L0, C.x, C.y, C.z};
            const float tt[4] = {T.x, T.y, T.z, T.w};
            const float bb[4] = {B.x, B.y, B.z, B.w};
            const float hh[4] = {Rh.x, Rh.y, Rh.z, Rh.w};
            float n[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float horizontal = fdiv<FAST>(rr[k] + ll[k], dx_sq, r_dx_sq);
                const float vertical = fdiv<FAST>(tt[k] + bb[k], dy_sq, r_dy_sq);
                const float p_update = fdiv<FAST>(horizontal + vertical - hh[k], denom, r_denom);
                n[k] = omega * p_update + om1 * cc[k];
            }
            if (row >= 0 && row < nyl) {
                if (e0) m = fmaxf(m, fabsf(n[0] - cc[0]));
                if (e1) m = fmaxf(m, fabsf(n[1] - cc[1]));
                if (e2) m = fmaxf(m, fabsf(n[2] - cc[2]));
                if (e3) m = fmaxf(m, fabsf(n[3] - cc[3]));
            }
            float4 o = make_float4(n[0], n[1], n[2], n[3]);
            if (ch == 0) o.x = n[1];          // P(0,j) = P(1,j)
            if (ch == nch - 1) o.w = 0.0f;    // P(nx-1,j) = 0
            if (valid) {
                *reinterpret_cast<float4 *>(dst + (long)row * nx + col) = o;
                if (row == gj_first)          // P(i,0) = P(i,1)
                    *reinterpret_cast<float4 *>(dst + (long)(row - 1) * nx + col) = o;
                if (row == gj_last)           // P(i,ny-1) = P(i,ny-2)
                    *reinterpret_cast<float4 *>(dst + (long)(row + 1) * nx + col) = o;
            }
        };
        row_update(j, w0, w1, w2, h0, lf0, rt0);
        if (l1) row_update(j + 1, w1, w2, w3, h1, lf1, rt1);
        if (l2) row_update(j + 2, w2, w3, w4, h2, lf2, rt2);
        if (l3) row_update(j + 3, w3, w4, w5, h3, lf3, rt3);
        w0 = w4;
        w1 = w5;
    }
    if (!res) return;
    m = wave_max(m);
    if (lane == 0) publish_max(slots + (size_t)it * kResSlots * kResStride, bid * kJacWavesPerBlock + wave, m);
}

// (solve_finalize_body: cfd_device.h, shared with the resident solve).
// r6: 1,024 threads -- a tolerance-mode solve's finalize folds and clears
// every sweep's 32 residual slots (50 sets), one set per wave at a time: 16
// waves take 4 rounds of slot reads instead of 13 (C3 in the reference's
// control flow spent 12.9 us per solve here, 21 solves per step).
constexpr int kFinThreads = 1024;
__global__ __launch_bounds__(kFinThreads) void k_finalize_solve(Geom g, Fields f, int pass, int iters,
                                                           int check_break, int flips,
                                                           int exact_flips) {
    solve_finalize_body(g, f, pass, iters, check_break, flips, exact_flips);
}

// After the speculative launch covering sweeps [it, it+T) (launch_jacobi_spec):
// fold its T residual slot sets into Ctl::err, and find the first of its
// sweeps whose residual is below p_tol (model.rs:816).  That sweep ends the
// solve: later launches skip (spec_stop), and unless it is the launch's last
// sweep the launch is re-run with exactly that many sweeps (spec_redo).
__global__ __launch_bounds__(kBlock) void k_spec_check(Geom g, Fields f, int pass, int it, int T,
                                                       int par) {
    Ctl *c = f.ctl;
    if (pass_off(c, pass) || c->spec_stop) return;
    const int wv = (int)threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    for (int k = it + wv; k < it + T; k += nw) {
        uint32_t *set = f.err_slots + (size_t)k * kResSlots * kResStride;
        const float v = read_max(set, c->err[k]);
        if ((threadIdx.x & 63) < kResSlots) set[(threadIdx.x & 63) * kResStride] = 0u;
        if ((threadIdx.x & 63) == 0) c->err[k] = __float_as_uint(v);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int j = 0;
    while (j < T && !(__uint_as_float(c->err[it + j]) < g.p_tol)) ++j;
    c->spec_launches = par + 1;
    if (j < T) {
        c->spec_stop = 1;
        c->spec_launch = par;
        c->spec_redo = j + 1 < T ? j + 1 : 0;
    }
}

// The speculative solve on slabs (r5): the host counts every launch of the
// solve as a buffer flip (it must know which buffer's ghost rows to exchange
// before each launch), so when a launch L < n-1 converged and its re-run
// left the result in buffer cur + L + 1 of the other parity, that buffer's
// owned rows are copied to buffer cur + n (the ghost rows are re-exchanged
// before they are read again).
__global__ __launch_bounds__(kBlock) void k_spec_align(Geom g, Fields f, int pass, int n) {
    const Ctl *c = f.ctl;
    if (pass_off(c, pass) || !c->spec_stop) return;
    const int L = c->spec_launch;
    if (((n - (L + 1)) & 1) == 0) return;
    const float4 *src = reinterpret_cast<const float4 *>(f.pp[(c->cur + L + 1) & 1]);
    float4 *dst = reinterpret_cast<float4 *>(f.pp[(c->cur + n) & 1]);
    const size_t n4 = (size_t)g.nyl * g.nx / 4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

// dst[q] = max(dst[q], slots of set q), then zero the slots (q < n).
__global__ void k_fold_slots(uint32_t *dst, uint32_t *slots, int n) {
    const int q = (int)threadIdx.x;
    if (q >= n) return;
    uint32_t *set = slots + (size_t)q * kResSlots * kResStride;
    uint32_t v = dst[q];
    for (int s = 0; s < kResSlots; ++s) {
        v = max(v, set[s * kResStride]);
        set[s * kResStride] = 0u;
    }
    dst[q] = v;
}

// ------------------------------------------------- velocity boundaries (K6)

// apply_boundary_conditions (model.rs:826-875), in the reference's order; a
// single workgroup with barriers between the phases that touch the same
// faces.  bc_kind 1 = build-defined lid-driven cavity.
__global__ __launch_bounds__(1024) void k_boundary(Geom g, Fields f) {
    const int nx = g.nx, W = nx + 1, nyl = g.nyl;
    const float inlet = f.ctl->inlet;
    float *__restrict__ u = f.u;
    float *__restrict__ v = f.v;
    const int t = threadIdx.x, nt = blockDim.x;
    for (int lj = t; lj < nyl; lj += nt) {
        const int j = g.j0 + lj;
        if (g.bc_kind == 0) {
            u[(long)lj * W] = inlet_value(g, inlet, j);
            u[(long)lj * W + nx] = u[(long)lj * W + nx - 1];
        } else {
            u[(long)lj * W] = 0.0f;
            u[(long)lj * W + nx] = 0.0f;
        }
    }
    __syncthreads();
    const bool has_bottom = g.j0 == 0;
    const bool has_top = g.j0 + nyl == g.ny;
    for (int i = t; i <= nx; i += nt) {
        if (has_bottom) u[i] = 0.0f;
        if (has_top) {
            const float lid = (g.bc_kind == 1 && i > 0 && i < nx) ? inlet : 0.0f;
            u[(long)(nyl - 1) * W + i] = lid;
        }
    }
    for (int i = t; i < nx; i += nt) {
        if (has_bottom) v[i] = 0.0f;
        if (has_top) v[(long)nyl * nx + i] = 0.0f;
    }
    __syncthreads();
    for (int k = t; k < f.n_obs; k += nt) {
        const int oi = f.obs[2 * k], oj = f.obs[2 * k + 1];
        const int lj = oj - g.j0;
        if (lj >= 0 && lj < nyl) u[(long)lj * W + oi] = 0.0f;
        if (lj >= 0 && lj <= nyl) v[(long)lj * nx + oi] = 0.0f;
    }
}

// ------------------------------------------------------ step finalize

// k_step_finalize's work (model.rs:333-377, :877-889) for one workgroup (its
// own launch: the maxima the previous launches published are visible).
__device__ __forceinline__ void step_finalize_body(const Geom &g, const Fields &f) {
    auto ld_ctl = [](const uint32_t *p) { return *p; };
    Ctl *c = f.ctl;
    if (threadIdx.x < 4) {   // fold the spread step maxima (sharded: already folded)
        uint32_t *set = f.red_slots + (size_t)threadIdx.x * kResSlots * kResStride;
        uint32_t v = ld_ctl(&c->red[threadIdx.x]);
        for (int s = 0; s < kResSlots; ++s) {
            v = max(v, ld_ctl(&set[s * kResStride]));
            set[s * kResStride] = 0u;
        }
        c->red[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    // failure detection: red[4] is this step's non-finite flag
    // (all-reduced across slabs with the maxima); the first such step sticks
    if (ld_ctl(&c->red[4]) && !c->nonfinite_step) {
        c->nonfinite_step = c->step + 1u;
        if (f.host_nonfinite) *f.host_nonfinite = c->step + 1u;   // zero-copy host mirror
    }
    c->res_u = __uint_as_float(c->red[0]);
    c->res_v = __uint_as_float(c->red[1]);
    const float max_vel = fmaxf(__uint_as_float(c->red[2]), __uint_as_float(c->red[3]));
    c->step += 1u;
    if (f.host_progress) *f.host_progress = c->step;   // watchdog progress (zero-copy)
    c->time = c->time + c->dt;
    const float previous_dt = c->dt;
    float new_dt;
    if (max_vel == 0.0f) {
        new_dt = c->dt;
    } else {
        const float cfl = 0.2f;
        const float dt_cfl = cfl * fminf(g.dx, g.dy) / max_vel;
        new_dt = fminf(dt_cfl, c->dt);
    }
    c->dt = (new_dt > previous_dt) ? fminf(new_dt, previous_dt * 1.1f) : new_dt;
    // the step's last solve residual: all-reduced across slabs with the
    // maxima (a sharded fixed-count step skips the solve's own all-reduce)
    c->last_p = __uint_as_float(ld_ctl(&c->red[5]));
    c->red[0] = c->red[1] = c->red[2] = c->red[3] = c->red[4] = c->red[5] = 0u;
    // a persistent solve on some slab timed out this step (all-reduced,
    // launch_abort_to_red): every rank's host sees CFD_ETIMEOUT at its next
    // synchronisation and all of them re-run from their checkpoints
    // (cfd_model::recover); later persistent launches of this rank leave at once
    if (ld_ctl(&c->red[6])) {
        if (f.persist) __hip_atomic_store(f.persist + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (f.host_nonfinite)
            __hip_atomic_store(f.host_nonfinite + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ void k_abort_to_red(Fields f) {
    if (threadIdx.x == 0 && f.persist)
        f.ctl->red[6] = __hip_atomic_load(f.persist + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? 1u : 0u;
}

// The all-reduced abort word back into this rank's abort flag and host word
// (k_step_finalize's part of it, for the entry points with no step finalize:
// cfd_piso_step, cfd_pressure_solve).
__global__ void k_abort_from_red(Fields f) {
    if (threadIdx.x != 0 || !f.ctl->red[6]) return;
    if (f.persist) __hip_atomic_store(f.persist + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (f.host_nonfinite)
        __hip_atomic_store(f.host_nonfinite + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void k_step_finalize(Geom g, Fields f) { step_finalize_body(g, f); }

// ------------------------------------------------- step reductions (K7)

// max |u - u_old|, max |v - v_old| (model.rs:333-344) and max |u|, max |v|
// (compute_automatic_time_step :879-880) over the owned rows; f32::max
// ignores NaN, as fmaxf does.
__global__ __launch_bounds__(kBlock) void k_step_reduce(Geom g, Fields f) {
    const size_t tid = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t nu = (size_t)g.nyl * (g.nx + 1), nv = (size_t)(g.nyl + 1) * g.nx;
    float du = 0.f, dv = 0.f, mu = 0.f, mv = 0.f;
    bool bad = false;
    for (size_t k = tid; k < nu; k += stride) {
        const float a = f.u[k];
        du = fmaxf(du, fabsf(a - f.u_old[k]));
        mu = fmaxf(mu, fabsf(a));
        bad |= nonfinite(a);
    }
    for (size_t k = tid; k < nv; k += stride) {
        const float a = f.v[k];
        dv = fmaxf(dv, fabsf(a - f.v_old[k]));
        mv = fmaxf(mv, fabsf(a));
        bad |= nonfinite(a);
    }
    flag_nonfinite(f.ctl, bad);
    du = wave_max(du);
    dv = wave_max(dv);
    mu = wave_max(mu);
    mv = wave_max(mv);
    if ((threadIdx.x & 63) == 0) {
        const int key = (int)(tid >> 6);
        constexpr size_t S = (size_t)kResSlots * kResStride;
        publish_max(f.red_slots, key, du);
        publish_max(f.red_slots + S, key, dv);
        publish_max(f.red_slots + 2 * S, key, mu);
        publish_max(f.red_slots + 3 * S, key, mv);
    }
}

}  // namespace

// ------------------------------------------------------------------ launchers

void launch_step_begin(const Geom &g, const Fields &f, int copy, hipStream_t s) {
    size_t n4 = f.u_alloc > f.v_alloc ? f.u_alloc / 4 : f.v_alloc / 4;
    hipLaunchKernelGGL(k_step_begin, dim3(copy ? copy_grid(n4) : 1), dim3(kBlock), 0, s, g, f,
                       copy);
}

void launch_copy_star(const Geom &g, const Fields &f, int pass, hipStream_t s) {
    size_t n4 = f.u_alloc > f.v_alloc ? f.u_alloc / 4 : f.v_alloc / 4;
    hipLaunchKernelGGL(k_copy_star, dim3(copy_grid(n4)), dim3(kBlock), 0, s, f, pass);
}

void launch_u_predictor(const Geom &g, const Fields &f, float dt_override, hipStream_t s) {
    const int glo = g.j0 > 1 ? g.j0 : 1;
    const int ghi = (g.j0 + g.nyl - 1) < (g.ny - 2) ? (g.j0 + g.nyl - 1) : (g.ny - 2);
    if (ghi < glo) return;
    const int nbx = cdiv(g.nx, kBlock);
    const dim3 grid(nbx * (ghi - glo + 1));
#define CFD_LAUNCH_U(SC, SPV) hipLaunchKernelGGL((k_u_predictor<SC, SPV>), grid, dim3(kBlock), 0, s, \
                                                 g, f, dt_override, glo - g.j0, nbx)
    if (g.scheme == 0) {
        if (g.sp_pow2) CFD_LAUNCH_U(0, 1); else CFD_LAUNCH_U(0, 0);
    } else {
        if (g.sp_pow2) CFD_LAUNCH_U(1, 1); else CFD_LAUNCH_U(1, 0);
    }
#undef CFD_LAUNCH_U
}

void launch_v_predictor(const Geom &g, const Fields &f, float dt_override, hipStream_t s) {
    const int glo = g.j0 > 1 ? g.j0 : 1;
    const int ghi = (g.j0 + g.nyl) < (g.ny - 1) ? (g.j0 + g.nyl) : (g.ny - 1);
    if (ghi < glo) return;
    const int nbx = cdiv(g.nx - 1, kBlock);
    const dim3 grid(nbx * (ghi - glo + 1));
#define CFD_LAUNCH_V(SC, SPV) hipLaunchKernelGGL((k_v_predictor<SC, SPV>), grid, dim3(kBlock), 0, s, \
                                                 g, f, dt_override, glo - g.j0, nbx)
    if (g.scheme == 0) {
        if (g.sp_pow2) CFD_LAUNCH_V(0, 1); else CFD_LAUNCH_V(0, 0);
    } else {
        if (g.sp_pow2) CFD_LAUNCH_V(1, 1); else CFD_LAUNCH_V(1, 0);
    }
#undef CFD_LAUNCH_V
}

void launch_predict(const Geom &g, const Fields &f, float dt_override, bool vec, hipStream_t s) {
    const int glo = g.j0 > 1 ? g.j0 : 1;
    const int u_hi = (g.j0 + g.nyl - 1) < (g.ny - 2) ? (g.j0 + g.nyl - 1) : (g.ny - 2);
    const int v_hi = (g.j0 + g.nyl) < (g.ny - 1) ? (g.j0 + g.nyl) : (g.ny - 1);
    const int ghi = u_hi > v_hi ? u_hi : v_hi;
    if (ghi < glo) return;
    if (vec && g.scheme == 0 && g.nx % 4 == 0 && aligned16(f.v) && aligned16(f.v_star)) {
        const int nbx4 = cdiv(g.nx / 4, kBlock);
        const dim3 gr(nbx4 * cdiv(ghi - glo + 1, 2));
        if (g.sp_pow2)
            hipLaunchKernelGGL((k_predict4r<1, 2>), gr, dim3(kBlock), 0, s, g, f, dt_override,
                               glo - g.j0, u_hi - g.j0, v_hi - g.j0, nbx4);
        else
            hipLaunchKernelGGL((k_predict4r<0, 2>), gr, dim3(kBlock), 0, s, g, f, dt_override,
                               glo - g.j0, u_hi - g.j0, v_hi - g.j0, nbx4);
        return;
    }
    const int nbx = cdiv(g.nx, kBlock);
    const dim3 grid(nbx * (ghi - glo + 1));
#define CFD_LAUNCH_P(SC, SPV) hipLaunchKernelGGL((k_predict<SC, SPV>), grid, dim3(kBlock), 0, s, g, f, \
                                                 dt_override, glo - g.j0, u_hi - g.j0, v_hi - g.j0, nbx)
    if (g.scheme == 0) {
        if (g.sp_pow2) CFD_LAUNCH_P(0, 1); else CFD_LAUNCH_P(0, 0);
    } else {
        if (g.sp_pow2) CFD_LAUNCH_P(1, 1); else CFD_LAUNCH_P(1, 0);
    }
#undef CFD_LAUNCH_P
}

void launch_copy_star_div(const Geom &g, const Fields &f, int pass, float dt_override,
                          hipStream_t s) {
    const int nbx = cdiv(g.nx / 4, kBlock);
    const dim3 grid(nbx * (g.nyl + 1 + 2 * kGhostUV));
    if (g.sp_pow2)
        hipLaunchKernelGGL(k_copy_star_div<1>, grid, dim3(kBlock), 0, s, g, f, pass, dt_override, nbx);
    else
        hipLaunchKernelGGL(k_copy_star_div<0>, grid, dim3(kBlock), 0, s, g, f, pass, dt_override, nbx);
}

void launch_divergence(const Geom &g, const Fields &f, int pass, float dt_override,
                       hipStream_t s) {
    const int nbx = cdiv(g.nx / 4, kBlock);
    if (g.sp_pow2)
        hipLaunchKernelGGL(k_divergence<1>, dim3(nbx * g.nyl), dim3(kBlock), 0, s, g, f, pass,
                           dt_override, nbx);
    else
        hipLaunchKernelGGL(k_divergence<0>, dim3(nbx * g.nyl), dim3(kBlock), 0, s, g, f, pass,
                           dt_override, nbx);
}

void launch_jacobi_sweep(const Geom &g, const Fields &f, int pass, int it, int row_lo,
                         int row_hi, int res, hipStream_t s) {
    if (row_hi <= row_lo) return;
    const int nch = g.nx / 4;
    const int nwc = cdiv(nch, 64);
    const int nbx = cdiv(nwc, kJacWavesPerBlock);
    const int nseg = cdiv(row_hi - row_lo, kJacRowsPerWave);
    float *pa = f.pp[0] - (long)g.hg * g.nx, *pb = f.pp[1] - (long)g.hg * g.nx;
    const dim3 grid(nbx * nseg), block(kJacWavesPerBlock * 64);
    with_fastdiv(g.fastdiv, [&](auto F) {
        hipLaunchKernelGGL((k_jacobi<kJacRowsPerWave, F()>), grid, block, 0, s, g, pa, pb, f.rhs,
                           f.ctl, f.err_slots, pass, it, row_lo, row_hi, nbx, res);
    });
}

void launch_jacobi_block(const Geom &g, const Fields &f, int pass, int it, int par, int T,
                         int out_lo, int out_hi, int res, hipStream_t s) {
    if (out_hi <= out_lo) return;
    uint32_t *rs = res ? f.err_slots + (size_t)(it + T - 1) * kResSlots * kResStride : nullptr;
    if (g.tb_kind == 4)
        launch_pipe(g, f, T, pass, it, par, out_lo, out_hi, rs, s);
    else if (g.tb_kind == 5)
        launch_lds(g, f, T, pass, it, par, out_lo, out_hi, rs, s);
    else
        launch_tb1(g, f, T, pass, it, par, out_lo, out_hi, rs, s);
}

bool launch_jacobi_persist(const Geom &g, const Fields &f, int pass, int par0, int nblk,
                           int out_lo, int out_hi, uint32_t epoch, int res_it, hipStream_t s) {
    if (out_hi <= out_lo || nblk < 1 || g.tb_kind != 5 || !f.persist) return false;
    uint32_t *rs = res_it >= 0 ? f.err_slots + (size_t)res_it * kResSlots * kResStride : nullptr;
    return launch_lds_persist8(g, f, pass, par0, nblk, out_lo, out_hi, epoch, rs, s);
}

void launch_jacobi_spec(const Geom &g, const Fields &f, int pass, int it, int par, int T,
                        int out_lo, int out_hi, hipStream_t s, int lag) {
    if (out_hi <= out_lo) return;
    launch_lds(g, f, T, pass, it, par, out_lo, out_hi,
               f.err_slots + (size_t)it * kResSlots * kResStride, s, 2, lag);
}

void launch_spec_check(const Geom &g, const Fields &f, int pass, int it, int T, int par,
                       hipStream_t s) {
    hipLaunchKernelGGL(k_spec_check, dim3(1), dim3(kBlock), 0, s, g, f, pass, it, T, par);
}

void launch_jacobi_redo(const Geom &g, const Fields &f, int pass, int out_lo, int out_hi,
                        hipStream_t s, int last_it, int last_par, int last_T) {
    if (out_hi <= out_lo) return;
    launch_lds(g, f, kMaxTemporal, pass, last_it, last_par, out_lo, out_hi,
               last_T > 0 ? f.err_slots + (size_t)last_it * kResSlots * kResStride : nullptr, s, 3,
               last_T);
}

void launch_spec_align(const Geom &g, const Fields &f, int pass, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_spec_align, dim3(256), dim3(kBlock), 0, s, g, f, pass, n);
}

void launch_fold_slots(uint32_t *dst, uint32_t *slots, int n, hipStream_t s) {
    hipLaunchKernelGGL(k_fold_slots, dim3(1), dim3(64), 0, s, dst, slots, n);
}

void launch_verify_division(float c, float r, unsigned long long *dev_counts, hipStream_t s) {
    hipLaunchKernelGGL(k_verify_division, dim3(8192), dim3(kBlock), 0, s, c, r, dev_counts);
}

void launch_finalize_solve(const Geom &g, const Fields &f, int pass, int iters, int check_break,
                           int flips, hipStream_t s, int exact_flips) {
    hipLaunchKernelGGL(k_finalize_solve, dim3(1), dim3(kFinThreads), 0, s, g, f, pass, iters,
                       check_break, flips, exact_flips);
}

void launch_boundary(const Geom &g, const Fields &f, hipStream_t s) {
    hipLaunchKernelGGL(k_boundary, dim3(1), dim3(1024), 0, s, g, f);
}

void launch_step_reduce(const Geom &g, const Fields &f, hipStream_t s) {
    const size_t n = (size_t)(g.nyl + 1) * (g.nx + 1);
    hipLaunchKernelGGL(k_step_reduce, dim3(copy_grid(n / 4 + 1)), dim3(kBlock), 0, s, g, f);
}

void launch_abort_to_red(const Fields &f, hipStream_t s) {
    hipLaunchKernelGGL(k_abort_to_red, dim3(1), dim3(64), 0, s, f);
}

void launch_abort_from_red(const Fields &f, hipStream_t s) {
    hipLaunchKernelGGL(k_abort_from_red, dim3(1), dim3(64), 0, s, f);
}

void launch_step_finalize(const Geom &g, const Fields &f, hipStream_t s) {
    hipLaunchKernelGGL(k_step_finalize, dim3(1), dim3(64), 0, s, g, f);
}

}  // namespace cfd
