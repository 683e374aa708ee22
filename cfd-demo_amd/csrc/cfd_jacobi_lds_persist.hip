// cfd_jacobi_lds_persist.hip — kind 5 (cfd_jacobi_lds.h): the persistent
// fixed-count solve, T = 8, one launch for all its blocks.
#include "cfd_jacobi_lds.h"

namespace cfd {
namespace {

// Persistent fixed-count solve: ONE launch runs nblk blocks of T sweeps
// (par0.. launches of the per-launch form) over ntiles tiles (tile = the four
// wave segments of one workgroup of the per-launch form).  Task (t, b), block
// b of tile t, reads the rows that t and its 3 x 3 neighbours (adjacent wave
// columns hold the halo lanes' columns, adjacent row groups the T-row input
// bands) wrote in block b-1, and overwrites the buffer they read in block
// b-1, so it starts once all nine have finished block b-1 — no launch
// boundary, no grid-wide drain, and a slow tile holds back only its
// neighbours.
//
// Ownership with stealing.  Workgroup w owns tile w (XCD-renumbered, as the
// per-launch form maps it) and runs its blocks in order, so on a GPU that
// holds every workgroup at once each one keeps its tile (and its rows' L2) for
// the whole solve.  A block is CLAIMED before it runs: tile t's line holds a
// claim counter beside its done flag, advanced by compare-and-swap, so every
// task runs exactly once.  An owner claims all its tile's unclaimed blocks
// with one CAS when it starts (no atomic per block on the fast path).  A
// workgroup that has waited more than `steal` ticks for a
// neighbour's block b-1 that nobody has claimed — its owner is not resident
// (a co-tenant kernel, another model's launch, RCCL kernels, a grid larger
// than the GPU holds) — claims that block itself, runs it when ready and then
// returns to its own task (a small stack of claimed tasks in LDS).
// Deadlock-free by construction: a wait is on a block that is either claimed
// by a running workgroup or stealable; the owner's own task sits at the
// bottom of its stack and a thief takes only a block below the one it waits
// to run (one CAS from the value it read, never "the next one"), so blocks
// fall strictly up every stack, no task depends on one below it, and waits
// never form a cycle.  The launch completes with any number of its workgroups resident.
// (The r3 form needed all of them resident at once: a co-tenant could strand
// it until its spin limit, with p' left invalid; a ticketed form that took
// tasks in block order measured 7.6 us per sweep against 4.7: a workgroup
// then waits for an arbitrary tile's neighbourhood, in effect a grid barrier
// per block.)
//
// Hand-off (MI355X_MICROARCH.md "Valid forms", Consumer, always): p' stores
// write through (sc1) and every wave drains them (s_waitcnt vmcnt(0)) before
// the workgroup's barrier, then ONE lane stores the tile's flag (agent scope);
// a waiting workgroup's wave 0 polls the nine flags (relaxed agent loads,
// s_sleep), then ONE agent acquire (buffer_inv sc1) + vmcnt(0) + the
// workgroup barrier before any p' load.  The launch runs several workgroups
// per CU, outside the table under which sc1 loads alone may replace the
// acquire, so the acquire stays (acq = 1).  Flags and claim counters hold epoch * 2^kPersistBlockBits
// + blocks done / claimed (a solve has at most kMaxSweeps / 8 = 512 blocks);
// the host gives every persistent launch a new epoch (never under graph
// capture: arguments would freeze), so a value below the epoch's base reads
// as 0 and nothing needs clearing between launches.  Waits are bounded by
// wall time (s_memrealtime, `deadline` ticks of 10 ns): past it the waiter
// sets the abort word persist[1], every workgroup leaves at its next poll or
// at entry, and a zero-copy host word makes the model's next cfd_* call report
// CFD_ETIMEOUT (a fault: residency no longer causes one).
//
// SUMS guard (r4; sums != 0 when the grid allows the form at all, LdsMarch):
// task (t, b) of the owner runs the SUMS form when every p' value it reads is
// below plim = 2^124 / R and every rhs value below rlim = 2^124, which keeps
// every value its 8 sweeps form below 2^126 / R (a sweep adds at most
// 0.1875 |rhs| / R to max |p'|: |hz + vt| <= 4 R max|p'| = denom max|p'|), so
// R |h|, R |v| < 2^127.  What a task reads: rows its 3 x 3 neighbours stored in
// block b-1 -- each wave publishes max |p'| of its stores with the tile's
// flag, in the tile's line (words 2-5 / 6-9 by block parity) -- and rows no
// tile of this launch writes (a slab's rows beyond its band), constant during
// the launch but different in the two p' buffers: blocks 0 and 1 run the
// reference's form and measure the tile's inputs in each buffer (and its rhs
// rows); a stolen task runs the reference's form.  max is NaN-ignoring: a NaN
// propagates through either form as the same operand.
constexpr int kStealDepth = 16;
template <int T, int FAST>
__global__ __launch_bounds__(kLdsWaves * 64, CFD_PERSIST_WPE) void k_jacobi_persist(
    Geom g, float *__restrict__ pa, float *__restrict__ pb, const float *__restrict__ rhs,
    Ctl *ctl, uint32_t *persist, uint32_t *host_fail, uint32_t *res_slots, uint32_t epoch, int pass,
    int par0, int nblk, int out_lo, int out_hi, int nwc, int nseg, int wlo, int whi, int ngrp,
    int acq, uint32_t deadline, uint32_t steal, int late, int sums, float plim, float rlim) {
    using M = LdsMarch<T, FAST, 4>;
    __shared__ f2 lds[kLdsWaves * M::D * 64];
    // control (wave 0 writes, everyone reads after a barrier): the task to
    // run, the claimed-task stack, the owner's next claimed block
    // (-2: claim it now, -1: none left)
    __shared__ int run_tile_s, run_blk_s, abort_s, own_next_s, sp_s, fast_s;
    __shared__ int stk_tile[kStealDepth], stk_blk[kStealDepth];
    // the SUMS guard: per-wave maxima of the block just run (lds_block trk),
    // the own tile's input maxima per p' buffer and its rhs maximum
    __shared__ float trk_s[3 * kLdsWaves], own_im_s[2], own_rm_s;
    __shared__ int own_ok_s[2], nfast_s;
    if (pass_off(ctl, pass)) return;
    const int ntiles = ngrp * nwc;
    const int own = xcd_block(g);
    if (own >= ntiles) return;   // a grid larger than the tiles: nothing owned
    const unsigned base = epoch << kPersistBlockBits;
    uint32_t *lines = persist + kPersistHeadLines * kPersistFlagStride;   // per tile: [0] done, [1] claimed
    const int lane = (int)threadIdx.x & 63;
    // blocks claimed of a tile from its claim word (values of older epochs read 0)
    auto count = [&](unsigned v) -> int { return v < base ? 0 : (int)(v - base); };
    // claim blocks of tile t by CAS from `v` (a read or guess of its claim
    // word): the first block claimed, or -1 when every block is claimed or
    // (thief) the word was not `v`.  all = true (the owner, once, when it
    // starts): every block not yet claimed, retrying from the word's actual
    // value -- a resident owner thus holds its whole tile and no thief ever
    // touches it, with no atomic per block.  A thief (all = false) takes
    // exactly the one block it saw unclaimed, or nothing: a later block of
    // that tile could depend on a task the thief holds below it on its stack
    // (a cycle).
    auto claim = [&](int t, unsigned v, bool all) -> int {
        uint32_t *w = lines + (size_t)t * kPersistFlagStride + 1;
        for (;;) {
            const int c = count(v);
            if (c >= nblk) return -1;
            unsigned exp = v;
            if (__hip_atomic_compare_exchange_strong(w, &exp, base + (unsigned)(all ? nblk : c + 1),
                                                     __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT))
                return c;
            if (!all) return -1;
            v = exp;   // the word as it was: retry from it
        }
    };
    if (threadIdx.x == 0) {
        sp_s = 0;
        own_next_s = -2;
        own_ok_s[0] = own_ok_s[1] = 0;
        own_im_s[0] = own_im_s[1] = own_rm_s = 0.0f;
        nfast_s = 0;
        // fail fast after an abort (every later launch of the model too)
        abort_s = __hip_atomic_load(persist + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        if (late > 0 && own % late == 1) {   // test knob: this owner starts late (not resident)
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            while (__builtin_amdgcn_s_memrealtime() - t0 < 200000u) __builtin_amdgcn_s_sleep(127);
        }
    }
    __syncthreads();
    if (abort_s) return;
    for (;;) {
        if (threadIdx.x < 64) {
            // ---- wave 0: the next task that is ready (claiming / stealing) ----
            int sp = sp_s, run_t = -1, run_b = -1;
            bool fail = false, fast = false;
            if (sp == 0) {
                int nb = own_next_s;
                if (nb == -2) {
                    int c = -1;
                    if (lane == 0) c = claim(own, 0u, true);
                    nb = __builtin_amdgcn_readfirstlane(c);
                }
                if (nb >= 0) {
                    if (lane == 0) {
                        stk_tile[0] = own;
                        stk_blk[0] = nb;
                    }
                    sp = 1;
                }
                own_next_s = -1;
            }
            while (sp > 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // stack writes before reads
                const int tt = stk_tile[sp - 1], bb = stk_blk[sp - 1];
                if (bb == 0) {
                    run_t = tt, run_b = bb;
                    --sp;
                    break;
                }
                // lanes 0..8 watch the task's tile and its neighbours, lane 9 the abort word
                const int wc = tt % nwc, gi = tt / nwc;
                const int c = wc + lane % 3 - 1, r = gi + lane / 3 - 1;
                const bool nbr = lane < 9 && c >= 0 && c < nwc && r >= 0 && r < ngrp;
                const int nt = nbr ? r * nwc + c : -1;
                const uint32_t *w = nbr ? lines + (size_t)nt * kPersistFlagStride
                                        : (lane == 9 ? persist + 1 : nullptr);
                const unsigned want = base + (unsigned)bb;
                const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
                bool ready = false, pushed = false;
                for (;;) {
                    const unsigned v = w ? __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                         : 0u;
                    const bool ok = lane < 9 ? (!nbr || v >= want) : v == 0u;
                    if (__all(ok)) {
                        ready = true;
                        break;
                    }
                    const uint64_t el = __builtin_amdgcn_s_memrealtime() - t0;
                    if (__any(lane == 9 && v != 0u) || el > (uint64_t)deadline) {
                        fail = true;
                        break;
                    }
                    if (el > (uint64_t)steal && sp < kStealDepth) {
                        // a neighbour block this task needs that nobody has claimed
                        const unsigned cw = nbr && v < want
                                                ? __hip_atomic_load(w + 1, __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_AGENT)
                                                : 0u;
                        const bool cand = nbr && v < want && count(cw) < bb;
                        const uint64_t m = __ballot(cand);
                        if (m) {
                            const int l = __builtin_ctzll(m);
                            const int st = __shfl(nt, l, 64);
                            const unsigned sv = __shfl(cw, l, 64);
                            int got = -1;
                            if (lane == 0) {
                                got = claim(st, sv, false);
                                if (got >= 0)   // steals counted for diagnostics (cfd_get_persist_steals)
                                    __hip_atomic_fetch_add(persist + 2, 1u, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT);
                            }
                            got = __builtin_amdgcn_readfirstlane(got);
                            if (got >= 0) {   // run it first, then come back to this task
                                if (lane == 0) {
                                    stk_tile[sp] = st;
                                    stk_blk[sp] = got;
                                }
                                ++sp;
                                pushed = true;
                                break;
                            }
                        }
                    }
                    __builtin_amdgcn_s_sleep(2);
                }
                if (fail) break;
                if (pushed) continue;
                if (ready) {
                    run_t = tt, run_b = bb;
                    --sp;
                    if (acq) {
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    } else {
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // keeps loads below the poll
                    }
                    if (sums && tt == own && bb >= 2 && own_ok_s[bb & 1] && own_rm_s < rlim &&
                        own_im_s[bb & 1] < plim) {
                        // the neighbours' stores of block bb-1 (published with their flags)
                        float mo = 0.0f;
                        if (nbr) {
                            const uint32_t *q = w + 2 + 4 * ((bb - 1) & 1);
#pragma unroll
                            for (int k = 0; k < kLdsWaves; ++k)
                                mo = fmaxf(mo, __uint_as_float(__hip_atomic_load(
                                                   q + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
                        }
                        fast = wave_max(mo) < plim;
                    }
                    break;
                }
            }
            if (lane == 0) {
                sp_s = sp;
                run_tile_s = run_t;
                run_blk_s = run_b;
                fast_s = fast;
                abort_s = fail;
                if (fail) {
                    __hip_atomic_store(persist + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (host_fail)   // zero-copy host word: cfd_* calls report CFD_ETIMEOUT
                        __hip_atomic_store(host_fail, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
        __syncthreads();
        const int tile = run_tile_s, b = run_blk_s;
        if (abort_s || tile < 0) {   // workgroup-uniform
            if (threadIdx.x == 0 && nfast_s)   // diagnostics: blocks run in the SUMS form
                __hip_atomic_fetch_add(persist + 3, (uint32_t)nfast_s, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        const bool fast = fast_s;
        const bool res = res_slots && b == nblk - 1;   // the solve's last block: its residual too
        if constexpr (FAST == 1) {
            if (fast) {
                if (res)
                    lds_block<T, FAST, 5, 1>(g, pa, pb, rhs, ctl, res_slots, par0 + b, out_lo, out_hi,
                                             nwc, nseg, wlo, whi, lds, 0, tile, trk_s);
                else
                    lds_block<T, FAST, 4, 1>(g, pa, pb, rhs, ctl, nullptr, par0 + b, out_lo, out_hi,
                                             nwc, nseg, wlo, whi, lds, 0, tile, trk_s);
            }
        }
        if (!fast) {
            if (res)
                lds_block<T, FAST, 5>(g, pa, pb, rhs, ctl, res_slots, par0 + b, out_lo, out_hi, nwc,
                                      nseg, wlo, whi, lds, 0, tile, trk_s);
            else
                lds_block<T, FAST, 4>(g, pa, pb, rhs, ctl, nullptr, par0 + b, out_lo, out_hi, nwc,
                                      nseg, wlo, whi, lds, 0, tile, trk_s);
        }
        // every wave's max |p'| stored, with (before) the flag: the next
        // block's guard of the neighbours (written through, drained below)
        if (sums && lane == 0) {
            const int wv = (int)threadIdx.x >> 6;
            __hip_atomic_store(lines + (size_t)tile * kPersistFlagStride + 2 + 4 * (b & 1) + wv,
                               __float_as_uint(trk_s[3 * wv]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // publish: every wave's write-through stores drained, then one flag
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0) {
            // the owner's next block (it claimed all of them when it started)
            if (tile == own) {
                own_next_s = b + 1 < nblk ? b + 1 : -1;
                if (fast) {
                    ++nfast_s;
                } else {
                    // the tile's inputs in the buffer block b read, and its rhs
                    float im = 0.0f, rm = 0.0f;
#pragma unroll
                    for (int k = 0; k < kLdsWaves; ++k) {
                        im = fmaxf(im, trk_s[3 * k + 1]);
                        rm = fmaxf(rm, trk_s[3 * k + 2]);
                    }
                    own_im_s[b & 1] = fmaxf(own_im_s[b & 1], im);
                    own_ok_s[b & 1] = 1;
                    own_rm_s = fmaxf(own_rm_s, rm);
                }
            }
            __hip_atomic_store(lines + (size_t)tile * kPersistFlagStride, base + (unsigned)b + 1u,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Workgroups of k_jacobi_persist<T, FAST> one CU holds at once with `pad`
// bytes of dynamic LDS: the occupancy API on the launched kernel itself,
// capped by the SGPR rule of MI355X_MICROARCH.md (Residency): at 97-112 SGPRs
// the hardware admits 6 four-wave workgroups where the API may say 7.  Used to
// size the tiles so one round of workgroups covers them; residency is no
// longer a correctness condition (claims and stealing, k_jacobi_persist).
template <int T, int FAST>
int persist_blocks_per_cu(int pad) {
    static int cache[2] = {0, 0};
    int &nb = cache[pad > 0 ? 1 : 0];
    if (nb == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &n, reinterpret_cast<const void *>(&k_jacobi_persist<T, FAST>), kLdsWaves * 64, pad) !=
                hipSuccess ||
            n < 1)
            n = 1;
        nb = std::min(n, 6);
    }
    return nb;
}

}  // namespace

int persist_blocks_per_cu8(const Geom &g, int pad) {
    return with_fastdiv(g.fastdiv, [&](auto F) { return persist_blocks_per_cu<8, F()>(pad); });
}

// The persistent form of launch_lds_t<8, 0> over nblk blocks: the same tile
// geometry (lds_tiles), its round sized by the persistent kernel's own
// occupancy; one workgroup per tile.  false (nothing launched): more tiles
// than kPersistMaxGroups lines, or row groups shorter than two T-row bands.
bool launch_lds_persist8(const Geom &g, const Fields &f, int pass, int par0, int nblk, int out_lo,
                         int out_hi, uint32_t epoch, uint32_t *rs, hipStream_t s) {
    constexpr int T = 8;
    const LdsTiles t =
        lds_tiles(g, T, out_lo, out_hi, 0, persist_blocks_per_cu8(g, lds_pad_bytes(g, 0)), true);
    const int ngrp = cdiv(t.nseg, kLdsWaves);
    // rows for a T-row band per group: a task's input rows lie in its 3 x 3
    // neighbourhood
    if (ngrp * t.nwc > kPersistMaxGroups || out_hi - out_lo < ngrp * 2 * T) return false;
    // one workgroup per tile (each owns one); CFD_PERSIST_GRID=<n> launches
    // n >= tiles (the surplus owns nothing and leaves).  Knobs are read per
    // launch (one getenv each per solve) so tests can change them.
    const char *ge = getenv("CFD_PERSIST_GRID");
    const int nwg = std::max(ngrp * t.nwc, ge ? atoi(ge) : 0);
    const dim3 grid(nwg), block(kLdsWaves * 64);
    float *pa = f.pp[0] - (long)g.hg * g.nx, *pb = f.pp[1] - (long)g.hg * g.nx;
    // the agent acquire after each poll (MI355X_MICROARCH.md); always 1, and an
    // argument still: folded into the kernel, all three instantiations come
    // out rescheduled and up to 9 KB different in size (profiles/r10/isa_compare.md)
    const int acq = 1;
    // wait deadline in s_memrealtime ticks (100 MHz): CFD_PERSIST_DEADLINE_US,
    // default 10 s (a wait that long is a fault; time-sliced GPUs stay far
    // below it)
    const char *de = getenv("CFD_PERSIST_DEADLINE_US");
    const double dl_us = de ? std::max(0.0, atof(de)) : 10e6;
    const uint32_t deadline = (uint32_t)std::min(4.0e9, dl_us * 100.0);
    // a neighbour block unclaimed after this long is stolen
    // (CFD_PERSIST_STEAL_US, default 50 us: a block takes ~40 us at 4096^2)
    const char *se = getenv("CFD_PERSIST_STEAL_US");
    const double st_us = se ? std::max(0.0, atof(se)) : 50.0;
    const uint32_t steal = (uint32_t)std::min(4.0e9, st_us * 100.0);
    // test knob: owners of tiles w % k == 1 start 2 ms late (CFD_PERSIST_LATE=k)
    const char *le = getenv("CFD_PERSIST_LATE");
    const int late = le ? std::max(0, atoi(le)) : 0;
    // the SUMS form's limits (k_jacobi_persist's guard)
    const int sums = lds_sums_grid(g);
    const float plim = sums ? std::ldexp(1.0f, 124) / g.r_dx_sq : 0.0f, rlim = std::ldexp(1.0f, 124);
    with_fastdiv(g.fastdiv, [&](auto F) {
        hipLaunchKernelGGL((k_jacobi_persist<T, F()>), grid, block, t.pad, s, g, pa, pb, f.rhs, f.ctl,
                           f.persist, f.host_nonfinite ? f.host_nonfinite + 2 : nullptr, rs, epoch, pass,
                           par0, nblk, out_lo, out_hi, t.nwc, t.nseg, t.wlo, t.whi, ngrp, acq,
                           deadline, steal, late, sums, plim, rlim);
    });
    return true;
}

}  // namespace cfd
