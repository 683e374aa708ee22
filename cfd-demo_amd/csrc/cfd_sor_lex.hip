// cfd_sor_lex.hip — the SOR of the reference's JavaScript variant in the
// script's own order (cfd_params.pressure_solver 4, index.html:741-774): p' is
// updated in place, row by row, left to right, omega 1.7, in double with f32
// stores, then the boundary rows and columns are copied (:761-770).
//
// Cell (i, j) of iteration k reads the NEW (i-1, j) and (i, j-1) of iteration
// k and the OLD (i+1, j) and (i, j+1), i.e. iteration k-1's values: the cells
// of an anti-diagonal are independent, and iteration k+1 can follow iteration
// k two diagonals behind.  That is a pipelined wavefront, and it reproduces
// the in-place sweep bit for bit.
//
// Mapping.  A wave owns a band of 64 interior rows, one row per lane; lane l
// runs one column behind lane l-1 (at step s it updates column s - l), so its
// new south value is what the lane below formed one step earlier and its old
// north value is the old east value the lane above holds at the same step:
// both cross lanes by DPP (from_left / from_right).  Lane 0 reads the band
// below from memory, the band's top lane the band above.  p' lives in the
// model's two p' buffers: iteration k reads buffer (cur + k) & 1 for old
// values and writes the other, as the fused red-black SOR does, so the solve's
// finalize flips the current buffer once per iteration run.  A write of
// iteration k+1 to (i, j) comes after iteration k finished (i+1, j) and
// (i, j+1), which have then read (i, j): the read-after-write waits below also
// order every write after the reads of the value it replaces.
//
// A task is (iteration k, band b), ticket t = k * B + b, taken from an atomic
// counter — never from blockIdx: every task a task waits for, (k, b-1),
// (k-1, b) and (k-1, b+1), has a lower ticket, so it is running or finished
// whatever the number of workgroups and the order they start in, one
// workgroup included (then every dependency is complete when its ticket is
// taken).  A task walks its rows in chunks of kLexC steps: it waits until
// the tasks it reads have published enough steps, loads the chunk's old
// values, runs the steps, drains its stores (written through, agent scope)
// and publishes its own step count from one lane.  Waits poll relaxed, one
// agent-scope acquire follows each, and a wait already covered by the last
// value seen is skipped.  Every polled word and the ticket counter are zeroed
// by the launcher's memset before each launch.  Waits are bounded by the
// persistent solves' deadline (CFD_PERSIST_DEADLINE_US): past it the waiter
// sets the timeout word and the model's host word, every workgroup leaves at
// its next poll or ticket, and the next synchronising call reports
// CFD_ETIMEOUT.
//
// Tolerance: iterations run ahead of the exit test.  The band that finishes
// an iteration last compares its folded max |new - old| with p_tol and
// records the first iteration below it in the exit word; tasks of later
// iterations that see the word do nothing.  Their partial writes may have
// overwritten the buffer holding that iteration's result, so a second launch
// of the same kernel (replay) runs exactly that many iterations again with the
// test off; it reads the count from the exit word on the device and returns
// at once when no later iteration had started (no early exit, or an exit at
// the last iteration).
//
// F64 (k_sor_lex_f64, cfd_script_options.residual_f64): the same body with the
// band's maximum kept as the script's double; it raises set k of res64 and
// folds (float) of it into ctl->err[k] as the other instantiation folds its f32
// maximum -- the same f32, rounding being monotone -- so the exit test, the
// waits and the replay are unchanged.
#include "cfd_device.h"

#include <type_traits>

#include <cstdlib>

namespace cfd {
namespace {

constexpr int kLexC = 16;                      // steps per chunk (one progress publish each)
constexpr int kLexHead = 16;                   // polled block: [0] ticket, [1] timeout; then the
                                               // tasks' step counts, then bands finished per iteration
constexpr uint32_t kLexExitBase = 1u << 20;    // exit word: base - first converged iteration (0: none)
static_assert(kLexExitBase > (uint32_t)kMaxSweeps, "exit word layout");

__device__ __forceinline__ uint32_t lex_poll(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// p' values other workgroups read inside the launch: written through
__device__ __forceinline__ void lex_store(float *p, float v) {
    __hip_atomic_store(reinterpret_cast<uint32_t *>(p), __float_as_uint(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}

template <int FAST, int F64>
__device__ __forceinline__ void sor_lex_body(float *pa, float *pb, const float *__restrict__ rhs, int nx,
                                             int ny, const SorConst &kc, Ctl *ctl, uint32_t *pol,
                                             uint32_t *exitw, uint32_t *host_fail, int pass, int iters,
                                             int B, int tol, float p_tol, int replay, uint32_t deadline,
                                             unsigned long long *res64) {
    typedef typename std::conditional<F64 != 0, double, float>::type acc_t;
    const int lane = (int)threadIdx.x;
    int n_it = iters;
    if (replay) {
        const uint32_t ev = lex_poll(exitw);
        if (ev == 0u) return;
        n_it = (int)(kLexExitBase - ev) + 1;
        if (n_it >= iters) return;   // the exit came at the last iteration: nothing ran past it
        tol = 0;
    }
    const int ntasks = n_it * B;
    const int cur = ctl->cur;
    // steps 0 .. nx - 2 + 63 (lane l updates column s - l at step s; at step l
    // it only fetches column 1, its first cell's old value)
    const int NC = (nx + 62 + kLexC - 1) / kLexC;   // chunks per task
    const int smax = NC * kLexC;                    // a finished task's step count
    uint32_t *prog = pol + kLexHead;
    uint32_t *done = prog + (size_t)iters * B;
    const double omega = 1.7;
    for (;;) {
        int tk = 0;
        if (lane == 0) tk = (int)__hip_atomic_fetch_add(pol, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tk = __builtin_amdgcn_readfirstlane(tk);
        if (tk >= ntasks) break;
        const int k = tk / B, b = tk - k * B;
        {
            // an exit recorded below this iteration: nothing to do; a timeout: leave
            const uint32_t w = lane == 0 && tol ? lex_poll(exitw) : lane == 1 ? lex_poll(pol + 1) : 0u;
            if (__any(lane == 1 && w != 0u)) break;
            if (__any(lane == 0 && w != 0u && (uint32_t)k > kLexExitBase - w)) continue;
        }
        const int nl = min(64, ny - 2 - 64 * b);   // rows of this band
        const int j = 1 + 64 * b + lane;
        const bool valid = lane < nl, top = lane == nl - 1, bot = lane == 0;
        const bool old = k > 0;                    // iteration 0 reads zeros (index.html:743)
        float *src = ((cur + k) & 1) ? pb : pa;
        float *dst = ((cur + k) & 1) ? pa : pb;
        const long row = (long)min(j, ny - 2) * nx;
        // lane 0's south row: the band below in this iteration, or row 0 as
        // the previous iteration's boundary copy left it
        const float *srow = (b > 0 ? dst : src) + row - nx;
        const bool s_ld = b > 0 || old;
        float nv_prev = 0.0f;   // this row's new value of the previous column
        float pe_prev = 0.0f;   // old value of this step's own cell (last step's east)
        acc_t m = 0;
        int seenA = 0, seenB = 0, seenC = 0;
        int status = 0;         // 1: an exit below this iteration, 2: timeout
        for (int c = 0; c < NC; ++c) {
            const int s0 = c * kLexC, s1 = s0 + kLexC - 1;
            // step counts (steps 0 .. count-1 done) the chunk's reads need:
            // (k, b-1) top lane's columns <= s1 (each done in step column + 63),
            // (k-1, b) this lane's columns <= s1 - lane + 1 (step s1 + 1),
            // (k-1, b+1) lane 0's columns <= s1 - 63 (step s1 - 63)
            const int needA = b > 0 ? min(min(s1, nx - 2) + 64, smax) : 0;
            const int needB = old ? min(s1 + 2, smax) : 0;
            const int needC = old && b + 1 < B ? min(s1 - 62, smax) : 0;
            if (needA > seenA || needB > seenB || needC > seenC) {
                const uint32_t *w = lane == 0   ? (b > 0 ? prog + tk - 1 : nullptr)
                                    : lane == 1 ? (old ? prog + tk - B : nullptr)
                                    : lane == 2 ? (old && b + 1 < B ? prog + tk - B + 1 : nullptr)
                                    : lane == 3 ? (tol ? exitw : nullptr)
                                    : lane == 4 ? pol + 1
                                                : nullptr;
                const int want = lane == 0 ? needA : lane == 1 ? needB : lane == 2 ? needC : 0;
                const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
                uint32_t v = 0u;
                for (;;) {
                    v = w ? lex_poll(w) : 0u;
                    const bool ok = lane >= 3 || (int)v >= want;
                    if (__any(lane == 4 && v != 0u)) {
                        status = 2;
                        break;
                    }
                    if (__any(lane == 3 && v != 0u && (uint32_t)k > kLexExitBase - v)) {
                        status = 1;
                        break;
                    }
                    if (__all(ok)) break;
                    if (__builtin_amdgcn_s_memrealtime() - t0 > (uint64_t)deadline) {
                        if (lane == 0) {
                            __hip_atomic_store(pol + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            if (host_fail)   // zero-copy host word: cfd_* calls report CFD_ETIMEOUT
                                __hip_atomic_store(host_fail, 1u, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_SYSTEM);
                        }
                        status = 2;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                if (status) break;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                seenA = (int)__shfl(v, 0, 64);
                seenB = (int)__shfl(v, 1, 64);
                seenC = (int)__shfl(v, 2, 64);
            }
            // the chunk's inputs: old east, rhs, old north (top lane), south (lane 0)
            float pe[kLexC], rh[kLexC], pn[kLexC], ps0[kLexC];
#pragma unroll
            for (int t = 0; t < kLexC; ++t) {
                const int i = s0 + t - lane;
                const int ce = min(max(i + 1, 1), nx - 1), ci = min(max(i, 1), nx - 2);
                pe[t] = old ? src[row + ce] : 0.0f;
                rh[t] = rhs[row + ci];
                pn[t] = old && top ? src[row + nx + ci] : 0.0f;
                ps0[t] = s_ld && bot ? srow[ci] : 0.0f;
            }
            const float pw0 = old ? src[row] : 0.0f;   // column 0 as iteration k-1 left it
#pragma unroll
            for (int t = 0; t < kLexC; ++t) {
                const int i = s0 + t - lane;
                const bool active = valid && i >= 1 && i <= nx - 2;
                const float sth = from_left(nv_prev), nth = from_right(pe[t]);
                const double p_old = (double)pe_prev;
                const double p_w = (double)(i == 1 ? pw0 : nv_prev);
                const double p_s = (double)(bot ? ps0[t] : sth);
                const double p_n = (double)(top ? pn[t] : nth);
                const double vt = ddiv<FAST>(p_n + p_s, kc.dy2, kc.r_dy2);
                const double hz = ddiv<FAST>((double)pe[t] + p_w, kc.dx2, kc.r_dx2);
                const double p_update = ddiv<FAST>(hz + vt - (double)rh[t], kc.denom, kc.r_denom);
                const float nv = (float)((1.0 - omega) * p_old + omega * p_update);
                pe_prev = pe[t];
                if (active) {
                    m = acc_max(m, (acc_t)fabs((double)nv - p_old));
                    nv_prev = nv;
                    float *d = dst + row + i;
                    lex_store(d, nv);
                    // the boundary copies of :761-770 (rows, then columns)
                    if (i == 1) lex_store(d - 1, nv);
                    if (i == nx - 2) lex_store(d + 1, 0.0f);
                    if (j == 1) {
                        lex_store(d - nx, nv);
                        if (i == 1) lex_store(d - nx - 1, nv);
                        if (i == nx - 2) lex_store(d - nx + 1, 0.0f);
                    }
                    if (j == ny - 2) {
                        lex_store(d + nx, nv);
                        if (i == 1) lex_store(d + nx - 1, nv);
                        if (i == nx - 2) lex_store(d + nx + 1, 0.0f);
                    }
                }
            }
            // publish: every store of the (single) storing wave has drained
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (lane == 0)
                __hip_atomic_store(prog + tk, (uint32_t)((c + 1) * kLexC), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        }
        if (status == 2) break;
        if (status || replay) continue;
        // the iteration's max |new - old| (index.html:757-758, NaN ignored as
        // there), folded by the solve's finalize; with the tolerance on, the
        // band that completes the iteration tests it
        float mf;
        if (F64) {
            const double md = wave_max_pos_f64(valid ? (double)m : 0.0);
            if (lane == 0) publish_max_pos_f64(res64 + (size_t)k * kResSlots * kRes64Stride, b, md);
            mf = (float)md;
        } else {
            mf = wave_max(valid ? (float)m : 0.0f);
        }
        if (lane == 0) {
            if (mf > 0.0f)
                __hip_atomic_fetch_max(&ctl->err[k], __float_as_uint(mf), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            if (tol) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const uint32_t n = __hip_atomic_fetch_add(done + k, 1u, __ATOMIC_RELAXED,
                                                          __HIP_MEMORY_SCOPE_AGENT);
                if ((int)n == B - 1 && __uint_as_float(lex_poll(&ctl->err[k])) < p_tol)
                    __hip_atomic_fetch_max(exitw, kLexExitBase - (uint32_t)k, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

template <int FAST>
__global__ __launch_bounds__(64) void k_sor_lex(float *pa, float *pb, const float *__restrict__ rhs,
                                                int nx, int ny, SorConst kc, Ctl *ctl, uint32_t *pol,
                                                uint32_t *exitw, uint32_t *host_fail, int pass,
                                                int iters, int B, int tol, float p_tol, int replay,
                                                uint32_t deadline) {
    if (pass_off(ctl, pass)) return;
    sor_lex_body<FAST, 0>(pa, pb, rhs, nx, ny, kc, ctl, pol, exitw, host_fail, pass, iters, B, tol, p_tol,
                          replay, deadline, nullptr);
}

template <int FAST>
__global__ __launch_bounds__(64) void k_sor_lex_f64(float *pa, float *pb, const float *__restrict__ rhs,
                                                    int nx, int ny, SorConst kc, Ctl *ctl, uint32_t *pol,
                                                    uint32_t *exitw, uint32_t *host_fail, int pass,
                                                    int iters, int B, int tol, float p_tol, int replay,
                                                    uint32_t deadline, unsigned long long *res64) {
    if (pass_off(ctl, pass)) return;
    sor_lex_body<FAST, 1>(pa, pb, rhs, nx, ny, kc, ctl, pol, exitw, host_fail, pass, iters, B, tol, p_tol,
                          replay, deadline, res64);
}

}  // namespace

size_t sor_lex_words(int iters, int ny) {
    const int B = cdiv(ny - 2, 64);
    const size_t w = (size_t)kLexHead + (size_t)iters * B + (size_t)iters;
    return (w + 3) & ~(size_t)3;
}

hipError_t launch_sor_lex(float *pa, float *pb, const float *rhs, int nx, int ny, const SorConst &k,
                          Ctl *ctl, uint32_t *pol, uint32_t *exitw, uint32_t *host_fail, int pass,
                          int iters, int tol, float p_tol, int n_cu, int *launches, hipStream_t s,
                          unsigned long long *res64) {
    const int B = cdiv(ny - 2, 64);
    const size_t bytes = sor_lex_words(iters, ny) * 4;
    const int ntasks = iters * B;
    // CFD_SOR_LEX_WGS caps the workgroups (1: the single-workgroup form of
    // the same kernel); read per launch so tests can switch
    int wgs = std::min(ntasks, 4 * std::max(1, n_cu));
    if (const char *e = getenv("CFD_SOR_LEX_WGS"))
        if (atoi(e) > 0) wgs = std::min(wgs, atoi(e));
    const char *de = getenv("CFD_PERSIST_DEADLINE_US");
    const double dl_us = de ? std::max(0.0, atof(de)) : 10e6;
    const uint32_t deadline = (uint32_t)std::min(4.0e9, dl_us * 100.0);
    *launches = 0;
    if (tol) {
        hipError_t e = hipMemsetAsync(exitw, 0, 16, s);
        if (e != hipSuccess) return e;
    }
    for (int replay = 0; replay <= (tol ? 1 : 0); ++replay) {
        hipError_t e = hipMemsetAsync(pol, 0, bytes, s);
        if (e != hipSuccess) return e;
        if (res64 && k.fast)
            hipLaunchKernelGGL(k_sor_lex_f64<1>, dim3(wgs), dim3(64), 0, s, pa, pb, rhs, nx, ny, k, ctl,
                               pol, exitw, host_fail, pass, iters, B, tol, p_tol, replay, deadline,
                               res64);
        else if (res64)
            hipLaunchKernelGGL(k_sor_lex_f64<0>, dim3(wgs), dim3(64), 0, s, pa, pb, rhs, nx, ny, k, ctl,
                               pol, exitw, host_fail, pass, iters, B, tol, p_tol, replay, deadline,
                               res64);
        else if (k.fast)
            hipLaunchKernelGGL(k_sor_lex<1>, dim3(wgs), dim3(64), 0, s, pa, pb, rhs, nx, ny, k, ctl,
                               pol, exitw, host_fail, pass, iters, B, tol, p_tol, replay, deadline);
        else
            hipLaunchKernelGGL(k_sor_lex<0>, dim3(wgs), dim3(64), 0, s, pa, pb, rhs, nx, ny, k, ctl,
                               pol, exitw, host_fail, pass, iters, B, tol, p_tol, replay, deadline);
        ++*launches;
    }
    return hipSuccess;
}

}  // namespace cfd
