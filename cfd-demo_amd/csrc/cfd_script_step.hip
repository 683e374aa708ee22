// cfd_script_step.hip — the script's own substep around its pressure solve
// (index.html:366-867 pisoStep, :870-930 applyBoundaryConditions):
//   k_script_predict   u*, v* and rhs (:368-739) in one row march, first- and
//                      second-order upwind and QUICK
//   k_script_correct   the corrector, p += p' and the whole boundary pass
//                      (:842-866, :870-930) as per-face selects
//
// Arithmetic is the script's, in double on the model's f32 fields widened,
// operation for operation, nothing contracted; every stored value is rounded
// to f32 once (a Float32Array store).  Guards and quirks are kept: faces the
// loops do not visit keep u / v, the second-order / QUICK y-Laplacian of v is
// (v[idx+2] - 2 v[idx] + v[idx]) / dy^2 with the flat index (at i = nx-2 it
// reads the next row's first value), the upwind tests are `>= 0` (-0 and 0
// take the first side, NaN the second).  A guard is a select between two
// computed values: a value the script would not compute is formed from
// in-bounds registers and dropped.
//
// Predictor mapping (cfd_predict_march.hip's): a lane owns 4 columns (chunk
// c, i0 = 4c), a wave 64 consecutive chunks and marches up R rows [r0, r0+R).
// At row k it holds u rows k-2..k+2 and v rows k-1..k+3 as f32 in registers
// (five rows each, the reach of the QUICK and second-order stencils, plus the
// row loaded one step ahead; values are widened where they are used, so the
// windows cost what the f32 march's do) and forms
//   v*(k+1)  from v rows k-1..k+3 and u row k+1,
//   u*(k)    from u rows k-2..k+2 and v rows k, k+1,
//   rhs(k)   from u*(k), the lane on the right's u*(k, i0+4), the carried
//            v*(k) and v*(k+1), all as the f32 values just stored,
// so each u / v row is loaded once per segment and u*, v* never come back from
// memory.  Two columns each side come from the adjacent lanes by DPP shifts;
// waves step 62 chunks (248 columns): lanes 0 and 63 only feed their
// neighbours.  Row loads are flat, so the chunk past the last column (c =
// nx/4) holds u face nx and v "columns" nx..nx+3 = the next row's first
// values, which is what the script's flat v[idx+2] reads; that lane stores u
// face nx (unvisited: u itself).  Rows outside the grid are clamped to it; no
// guard selects them.  The obstacle test is the host's per-row face interval
// (two ints per row; see cfd_model::script_build).
#include "cfd_device.h"

#pragma clang fp contract(off)

namespace cfd {
namespace {

// register windows of a step: u row k-2+r in u[r], v row k-1+r in v[r],
// columns i0-2..i0+5 at index 2 + column - i0; CU / CV: window rows of the
// face's own u / v row
template <int CU, int CV>
struct SAcc {
    const float (&u)[5][8];
    const float (&v)[5][8];
    int q;
    __device__ __forceinline__ double U(int di, int dj) const { return (double)u[CU + dj][q + 2 + di]; }
    __device__ __forceinline__ double V(int di, int dj) const { return (double)v[CV + dj][q + 2 + di]; }
};

// (-a + 6 b + 3 c) / 8 and (3 a + 6 b - c) / 8 as the script writes them; / 8 is exact
__device__ __forceinline__ double quick_up(double a, double b, double c) {
    return (-a + 6.0 * b + 3.0 * c) * 0.125;
}
__device__ __forceinline__ double quick_dn(double a, double b, double c) {
    return (3.0 * a + 6.0 * b - c) * 0.125;
}
__device__ __forceinline__ double so(double a, double b) { return 1.5 * a - 0.5 * b; }

// u*(i, j), 1 <= i <= nx-1, 1 <= j <= ny-2 (:382-549)
template <int S, int FAST, class A>
__device__ __forceinline__ double u_face(const A &a, int i, int j, int nx, int ny, const ScriptStep &k) {
    const double u0 = a.U(0, 0), ue = a.U(1, 0), uw = a.U(-1, 0), un = a.U(0, 1), us = a.U(0, -1);
    const double vn = 0.5 * (a.V(-1, 1) + a.V(0, 1));
    const double vs = 0.5 * (a.V(-1, 0) + a.V(0, 0));
    double fe, fw, fn, fs;
    if (S == CFD_SCRIPT_FIRST) {
        fe = 0.5 * (u0 + ue) >= 0.0 ? u0 : ue;
        fw = 0.5 * (uw + u0) >= 0.0 ? uw : u0;
        fn = vn >= 0.0 ? u0 : un;
        fs = vs >= 0.0 ? us : u0;
    } else {
        const double uee = a.U(2, 0), uww = a.U(-2, 0), unn = a.U(0, 2), uss = a.U(0, -2);
        if (S == CFD_SCRIPT_SECOND) {
            fe = u0 >= 0.0 ? (i > 1 ? so(u0, uw) : u0) : (i < nx - 1 ? so(ue, uee) : ue);
            fw = uw >= 0.0 ? (i > 2 ? so(uw, uww) : uw) : so(u0, ue);
            fn = vn >= 0.0 ? (j > 1 ? so(u0, us) : u0) : (j < ny - 2 ? so(un, unn) : un);
            fs = vs >= 0.0 ? (j > 1 ? so(us, uss) : us) : so(u0, un);
        } else {
            fe = u0 >= 0.0 ? (i >= 2 ? quick_up(uw, u0, ue) : so(u0, uw))
                           : (i <= nx - 2 ? quick_dn(u0, ue, uee) : ue);
            fw = uw >= 0.0 ? (i >= 3 ? quick_up(uww, uw, u0) : so(uw, u0)) : quick_dn(uw, u0, ue);
            fn = vn >= 0.0 ? (j >= 2 ? quick_up(us, u0, un) : so(u0, us))
                           : (j < ny - 2 ? quick_dn(u0, un, unn) : un);
            fs = vs >= 0.0 ? (j >= 2 ? quick_up(uss, us, u0) : so(us, u0)) : quick_dn(us, u0, un);
        }
    }
    const double Fe = fe * fe, Fw = fw * fw, Fn = vn * fn, Fs = vs * fs;
    const double conv = ddiv<FAST>(Fe - Fw, k.dx, k.r_dx) + ddiv<FAST>(Fn - Fs, k.dy, k.r_dy);
    const double lap = ddiv<FAST>(ue - 2.0 * u0 + uw, k.dxx, k.r_dxx) +
                       ddiv<FAST>(un - 2.0 * u0 + us, k.dyy, k.r_dyy);
    return u0 + k.dt * (-conv + k.nu * lap);
}

// v*(i, j), 1 <= i <= nx-2, 1 <= j <= ny-1 (:564-723)
template <int S, int FAST, class A>
__device__ __forceinline__ double v_face(const A &a, int i, int j, int nx, int ny, const ScriptStep &k) {
    const double v0 = a.V(0, 0), ve = a.V(1, 0), vw = a.V(-1, 0), vn = a.V(0, 1), vs = a.V(0, -1);
    const double u_e = a.U(1, 0), u_w = a.U(0, 0);
    const double vna = 0.5 * (v0 + vn), vsa = 0.5 * (vs + v0);
    double fe, fw, fn, fs, lap_y;
    if (S == CFD_SCRIPT_FIRST) {
        fe = u_e >= 0.0 ? v0 : ve;
        fw = u_w >= 0.0 ? vw : v0;
        fn = vna >= 0.0 ? v0 : vn;
        fs = vsa >= 0.0 ? vs : v0;
        lap_y = vn - 2.0 * v0 + vs;
    } else {
        const double vee = a.V(2, 0), vww = a.V(-2, 0), vnn = a.V(0, 2), vss = a.V(0, -2);
        if (S == CFD_SCRIPT_SECOND) {
            fe = u_e >= 0.0 ? so(v0, vw) : (i < nx - 2 ? so(ve, vee) : ve);
            fw = u_w >= 0.0 ? (i > 1 ? so(vw, vww) : vw) : so(v0, ve);
            fn = vna >= 0.0 ? (j > 1 ? so(v0, vs) : v0) : (j < ny - 1 ? so(vn, vnn) : vn);
            fs = vsa >= 0.0 ? (j > 1 ? so(vs, vss) : vs) : so(v0, vn);
        } else {
            fe = u_e >= 0.0 ? (i >= 2 ? quick_up(vw, v0, ve) : so(v0, vw))
                            : (i < nx - 2 ? quick_dn(v0, ve, vee) : ve);
            fw = u_w >= 0.0 ? (i >= 3 ? quick_up(vww, vw, v0) : so(vw, v0)) : quick_dn(vw, v0, ve);
            fn = vna >= 0.0 ? (j >= 2 ? quick_up(vs, v0, vn) : so(v0, vs))
                            : (j < ny - 1 ? quick_dn(v0, vn, vnn) : vn);
            fs = vsa >= 0.0 ? (j >= 2 ? quick_up(vss, vs, v0) : so(vs, v0))
                            : (j < ny - 1 ? quick_dn(vs, v0, vn) : v0);
        }
        lap_y = vee - 2.0 * v0 + v0;   // the script's own (:641, :721)
    }
    const double Fe = u_e * fe, Fw = u_w * fw, Fn = fn * fn, Fs = fs * fs;
    const double conv = ddiv<FAST>(Fe - Fw, k.dx, k.r_dx) + ddiv<FAST>(Fn - Fs, k.dy, k.r_dy);
    const double lap = ddiv<FAST>(ve - 2.0 * v0 + vw, k.dxx, k.r_dxx) + ddiv<FAST>(lap_y, k.dyy, k.r_dyy);
    return v0 + k.dt * (-conv + k.nu * lap);
}

#ifndef CFD_SS_WPE
#define CFD_SS_WPE 2   // minimum waves per SIMD (caps VGPRs at 256)
#endif

template <int S, int FAST, int R>
__global__ __launch_bounds__(kBlock, CFD_SS_WPE) void k_script_predict(Geom g, Fields f, ScriptStep k,
                                                                       int nwc, int nseg) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lane = (int)threadIdx.x & 63;
    const int bid = (int)blockIdx.x;
    const int wc = bid % nwc;
    const int seg = (bid / nwc) * (kBlock / 64) + wave;
    if (seg >= nseg) return;   // wave-uniform
    const int nx = g.nx, ny = g.ny, W = nx + 1, nch = nx / 4;
    // the last segment ends at ny and overlaps its neighbour (both store the
    // same values; no segment reads what another stores)
    const int r0 = min(seg * R, ny - R), r1 = r0 + R;
    const int c = wc * 62 - 1 + lane;
    const bool in_dom = c >= 0 && c <= nch;
    const int i0 = in_dom ? 4 * c : 0;
    const bool st_lane = in_dom && lane >= 1 && lane <= 62;
    const int vo = in_dom ? 16 * c : 0x7FFF0000;   // far offset: the load returns 0
    const __amdgpu_buffer_rsrc_t rs_u =
        __builtin_amdgcn_make_buffer_rsrc(f.u_alloc_base, 0, (int)(f.u_alloc * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_v =
        __builtin_amdgcn_make_buffer_rsrc(f.v_alloc_base, 0, (int)(f.v_alloc * 4), 0x00020000);
    auto ld = [&](float(&d)[4], __amdgpu_buffer_rsrc_t rs, int row, int hi, int pitch) {
        row = row < 0 ? 0 : (row > hi ? hi : row);
        const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rs, vo, (row + kGhostUV) * pitch * 4, 0);
        d[0] = __uint_as_float(x.x); d[1] = __uint_as_float(x.y);
        d[2] = __uint_as_float(x.z); d[3] = __uint_as_float(x.w);
    };
    // UQ[r]: u row kk-2+r, VQ[r]: v row kk-1+r (r < 5); [5]: the row one step ahead
    float UQ[6][4], VQ[6][4];
    float vs[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // v*(kk), carried from the previous step
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        ld(UQ[r], rs_u, r0 - 3 + r, ny - 1, W);
        ld(VQ[r], rs_v, r0 - 2 + r, ny, nx);
    }
#pragma unroll 1
    for (int kk = r0 - 1; kk < r1; ++kk) {
        ld(UQ[5], rs_u, kk + 3, ny - 1, W);
        ld(VQ[5], rs_v, kk + 4, ny, nx);
        float ux[5][8], vx[5][8];
#pragma unroll
        for (int r = 0; r < 5; ++r)
#pragma unroll
            for (int x = 0; x < 8; ++x) {
                ux[r][x] = x >= 2 && x < 6 ? UQ[r][x - 2] : 0.0f;
                vx[r][x] = x >= 2 && x < 6 ? VQ[r][x - 2] : 0.0f;
            }
        // neighbour columns the faces read: u row kk (+-2), u row kk+1 (+1),
        // v row kk (-1), v row kk+1 (+-2)
        ux[2][0] = from_left(ux[2][4]);
        ux[2][1] = from_left(ux[2][5]);
        ux[2][6] = from_right(ux[2][2]);
        ux[2][7] = from_right(ux[2][3]);
        ux[3][6] = from_right(ux[3][2]);
        vx[1][1] = from_left(vx[1][5]);
        vx[2][0] = from_left(vx[2][4]);
        vx[2][1] = from_left(vx[2][5]);
        vx[2][6] = from_right(vx[2][2]);
        vx[2][7] = from_right(vx[2][3]);

        // v*(kk+1): faces the loop visits (:554-555), else v itself
        const int rv = kk + 1;
        const int ovl = k.obs_v[2 * rv], ovh = k.obs_v[2 * rv + 1];
        float vn[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q;
            const double val = v_face<S, FAST>(SAcc<3, 2>{ux, vx, q}, i, rv, nx, ny, k);
            const bool visited = rv >= 1 && rv <= ny - 1 && i >= 1 && i <= nx - 2;
            const bool obst = i >= ovl && i < ovh;
            vn[q] = visited ? (obst ? 0.0f : (float)val) : vx[2][q + 2];
        }
        if (st_lane && c < nch && (kk >= r0 || r0 == 0))
            *reinterpret_cast<f4u *>(f.v_star + (long)rv * nx + i0) = (f4u){vn[0], vn[1], vn[2], vn[3]};
        if (kk >= r0) {
            // u*(kk): faces the loop visits (:372-373), else u itself
            const int oul = k.obs_u[2 * kk], ouh = k.obs_u[2 * kk + 1];
            float us[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + q;
                const double val = u_face<S, FAST>(SAcc<2, 1>{ux, vx, q}, i, kk, nx, ny, k);
                const bool visited = kk >= 1 && kk <= ny - 2 && i >= 1 && i <= nx - 1;
                const bool obst = i >= oul && i < ouh;
                us[q] = visited ? (obst ? 0.0f : (float)val) : ux[2][q + 2];
            }
            const float east = from_right(us[0]);
            if (st_lane) {
                if (c < nch) {
                    *reinterpret_cast<f4u *>(f.u_star + (long)kk * W + i0) = (f4u){us[0], us[1], us[2], us[3]};
                    // rhs = ((u*_r - u*_l) / dx + (v*_t - v*_b) / dy) / dt_sub (:730-739)
                    const float ur[5] = {us[0], us[1], us[2], us[3], east};
                    f4u rh;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const double div =
                            ddiv<FAST>((double)ur[q + 1] - (double)ur[q], k.dx, k.r_dx) +
                            ddiv<FAST>((double)vn[q] - (double)vs[q], k.dy, k.r_dy);
                        rh[q] = (float)(div / k.dt);
                    }
                    *reinterpret_cast<f4u *>(f.rhs + (long)kk * nx + i0) = rh;
                } else {
                    f.u_star[(long)kk * W + nx] = us[0];   // face nx
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) vs[q] = vn[q];
#pragma unroll
        for (int r = 0; r < 5; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                UQ[r][q] = UQ[r + 1][q];
                VQ[r][q] = VQ[r + 1][q];
            }
    }
}

// One lane: 4 columns of one row j in [0, ny] (row ny: v only); the chunk past
// the last column: u face nx.  Each face gets the value the script's ordered
// overwrites leave (:842-866, then :873-929: inlet, outlet copy, rows 0 and
// ny-1 of u, rows 0 and ny of v, obstacle faces).
template <int FAST>
__global__ __launch_bounds__(kBlock) void k_script_correct(Geom g, Fields f, ScriptStep k) {
    const int nx = g.nx, ny = g.ny, W = nx + 1, nch = nx / 4;
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= (long)(ny + 1) * (nch + 1)) return;
    const int j = (int)(t / (nch + 1)), c = (int)(t % (nch + 1)), i0 = 4 * c;
    const float *__restrict__ pp = f.pp[f.ctl->cur & 1];
    // u face (i, j), 1 <= i <= nx-1: u* - dt_sub (p'_r - p'_l) / dx, stored as f32
    auto ucorr = [&](int i, float ustar, float pl, float pr) {
        return (float)((double)ustar - ddiv<FAST>(k.dt * ((double)pr - (double)pl), k.dx, k.r_dx));
    };
    if (c == nch) {
        if (j >= ny) return;
        const int oul = k.obs_u[2 * j], ouh = k.obs_u[2 * j + 1];
        const long pj = (long)j * nx;
        // the outlet copy reads the corrected u(nx-1, j) before walls and obstacle zero anything
        float val = ucorr(nx - 1, f.u_star[(long)j * W + nx - 1], pp[pj + nx - 2], pp[pj + nx - 1]);
        if (j == 0 || j == ny - 1 || (nx >= oul && nx < ouh)) val = 0.0f;
        f.u[(long)j * W + nx] = val;
        return;
    }
    // v row j
    {
        const int ovl = k.obs_v[2 * j], ovh = k.obs_v[2 * j + 1];
        f4u out = {0.0f, 0.0f, 0.0f, 0.0f};
        if (j >= 1 && j <= ny - 1) {
            const f4u vs = *reinterpret_cast<const f4u *>(f.v_star + (long)j * nx + i0);
            const f4u pt = *reinterpret_cast<const f4u *>(pp + (long)j * nx + i0);
            const f4u pb = *reinterpret_cast<const f4u *>(pp + (long)(j - 1) * nx + i0);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = i0 + q;
                const float val = (float)((double)vs[q] -
                                          ddiv<FAST>(k.dt * ((double)pt[q] - (double)pb[q]), k.dy, k.r_dy));
                out[q] = (i >= ovl && i < ovh) ? 0.0f : val;
            }
        }
        *reinterpret_cast<f4u *>(f.v + (long)j * nx + i0) = out;
    }
    if (j >= ny) return;
    const int oul = k.obs_u[2 * j], ouh = k.obs_u[2 * j + 1];
    const f4u pc = *reinterpret_cast<const f4u *>(pp + (long)j * nx + i0);
    {   // p += p' over all cells (:858-863)
        const f4u p0 = *reinterpret_cast<const f4u *>(f.p + (long)j * nx + i0);
        f4u pn;
#pragma unroll
        for (int q = 0; q < 4; ++q) pn[q] = (float)((double)p0[q] + (double)pc[q]);
        *reinterpret_cast<f4u *>(f.p + (long)j * nx + i0) = pn;
    }
    const f4u us = *reinterpret_cast<const f4u *>(f.u_star + (long)j * W + i0);
    const float pl = c > 0 ? pp[(long)j * nx + i0 - 1] : 0.0f;
    const float pw[5] = {pl, pc[0], pc[1], pc[2], pc[3]};
    f4u out;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = i0 + q;
        float val = i == 0 ? k.inlet[j] : ucorr(i, us[q], pw[q], pw[q + 1]);
        if (j == 0 || j == ny - 1 || (i >= oul && i < ouh)) val = 0.0f;
        out[q] = val;
    }
    *reinterpret_cast<f4u *>(f.u + (long)j * W + i0) = out;
}

}  // namespace

bool script_step_ok(const Geom &g, const Fields &f) {
    return g.nx % 4 == 0 && g.nx >= 8 && g.ny >= 4 && g.j0 == 0 && g.nyl == g.ny &&
           (uint64_t)f.u_alloc * 4u < (1ull << 31) && (uint64_t)f.v_alloc * 4u < (1ull << 31);
}

void launch_script_predict(const Geom &g, const Fields &f, const ScriptStep &k, int scheme,
                           hipStream_t s) {
    // 8 rows per wave segment (the f32 march's choice for the second-order
    // scheme), 4 on grids under 8 rows
    const int rows = g.ny >= 8 ? 8 : 4;
    const int nwc = cdiv(g.nx / 4 + 1, 62);
    const int nseg = cdiv(g.ny, rows);
    const dim3 grid(nwc * cdiv(nseg, kBlock / 64));
#define CFD_LAUNCH_SS(SC, FV, R) \
    hipLaunchKernelGGL((k_script_predict<SC, FV, R>), grid, dim3(kBlock), 0, s, g, f, k, nwc, nseg)
#define CFD_LAUNCH_SS2(SC, FV) \
    if (rows == 8) CFD_LAUNCH_SS(SC, FV, 8); else CFD_LAUNCH_SS(SC, FV, 4)
#define CFD_LAUNCH_SS3(SC) \
    if (k.fast) { CFD_LAUNCH_SS2(SC, 1); } else { CFD_LAUNCH_SS2(SC, 0); }
    if (scheme == CFD_SCRIPT_FIRST) {
        CFD_LAUNCH_SS3(CFD_SCRIPT_FIRST);
    } else if (scheme == CFD_SCRIPT_SECOND) {
        CFD_LAUNCH_SS3(CFD_SCRIPT_SECOND);
    } else {
        CFD_LAUNCH_SS3(CFD_SCRIPT_QUICK);
    }
#undef CFD_LAUNCH_SS3
#undef CFD_LAUNCH_SS2
#undef CFD_LAUNCH_SS
}

void launch_script_correct(const Geom &g, const Fields &f, const ScriptStep &k, hipStream_t s) {
    const long n = (long)(g.ny + 1) * (g.nx / 4 + 1);
    const dim3 grid(cdiv(n, kBlock));
    if (k.fast)
        hipLaunchKernelGGL(k_script_correct<1>, grid, dim3(kBlock), 0, s, g, f, k);
    else
        hipLaunchKernelGGL(k_script_correct<0>, grid, dim3(kBlock), 0, s, g, f, k);
}

}  // namespace cfd
