"""CPU, multi-process (gloo, world size 2 and 3): the 1D row-slab plan that
cfd_create_sharded drives on the GPUs (cfd-demo_amd/csrc/slab_plan.h, through
the C ABI cfd_plan_*) reproduces the single-domain result bit for bit.

Each rank holds its slab with ghost rows, runs Jacobi sweeps over exactly the
rows cfd_plan_sweep names (a numpy emulation of k_jacobi's arithmetic and
fused p' boundary stores), exchanges exactly the rows cfd_plan_halo names via
torch.distributed send/recv, and the gathered result must equal the
single-domain oracle (oracle/cfd_oracle.c) word for word.  The exchange
geometry of u and v is checked by shipping global row ids.  Since r5 the
tolerance mode's speculative slab blocks (enqueue_spec_slabs) run the same
way: exits at every block position equal the oracle's p', residual and sweep
count, with one exchange and one all-reduce per block.
"""
import ctypes as C
import os
import socket

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _lib():
    import sys
    for p in (os.path.join(ROOT, "cfd-demo_amd"), os.path.join(ROOT, "oracle")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from cfdamd import _lib as L
    return L.load()


def plan_slab(ny, n, r):
    a, b = C.c_uint64(), C.c_uint64()
    assert _lib().cfd_plan_slab(ny, n, r, C.byref(a), C.byref(b)) == 0
    return int(a.value), int(b.value)


def plan_sweep(j0, nyl, ny, hg, it, iters):
    lo, hi, ex = C.c_int(), C.c_int(), C.c_int()
    assert _lib().cfd_plan_sweep(j0, nyl, ny, hg, it, iters, C.byref(lo), C.byref(hi),
                                 C.byref(ex)) == 0
    return lo.value, hi.value, bool(ex.value)


def plan_block(j0, nyl, ny, hg, it, t_max, iters):
    T, lo, hi, ex = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert _lib().cfd_plan_block(j0, nyl, ny, hg, it, t_max, iters, C.byref(T), C.byref(lo),
                                 C.byref(hi), C.byref(ex)) == 0
    return T.value, lo.value, hi.value, bool(ex.value)


def plan_overlap(nyl, hg, r, n, lo, hi):
    out = (C.c_int * 6)()
    split = _lib().cfd_plan_overlap(nyl, hg, r, n, lo, hi, out)
    return bool(split), list(out)


def block_band(src, rhs, g0, a, b, T, nx, ny, j0, dx, dy):
    """The final sweep of a T-sweep block, stored rows [a, b) only, from src
    alone: what one launch of the temporally blocked kernel over [a, b)
    computes (its intermediate sweeps live on chip, here in private copies)."""
    cur, nxt = src.copy(), src.copy()
    for s_ in range(T):
        e = T - 1 - s_
        lo_, hi_ = max(a - e, 1 - j0), min(b + e, ny - 1 - j0)
        sweep_rows(cur, nxt, rhs, g0, lo_, hi_, nx, ny, j0, dx, dy)
        cur, nxt = nxt, cur
    return cur


def plan_halo(kind, nyl, depth, r, n):
    out = (C.c_int * 6)()
    assert _lib().cfd_plan_halo(kind, nyl, depth, r, n, out) == 0
    return list(out)


def sweep_rows(src, dst, rhs, g0, lo, hi, nx, ny, j0, dx, dy):
    """k_jacobi on local rows [lo, hi); src, dst and rhs all carry g0 ghost
    rows in front (rhs ghosts are exchanged once per solve)."""
    omega, om1 = F(0.75), F(1.0) - F(0.75)
    dx2, dy2 = dx * dx, dy * dy
    denom = F(2.0) / (dx * dx) + F(2.0) / (dy * dy)
    for lj in range(lo, hi):
        r = lj + g0
        Cc, T, B = src[r], src[r + 1], src[r - 1]
        L = np.concatenate(([F(0)], Cc[:-1]))
        R = np.concatenate((Cc[1:], [F(0)]))
        h = (R + L) / dx2
        v = (T + B) / dy2
        n = omega * ((h + v - rhs[r]) / denom) + om1 * Cc
        n[0] = n[1]
        n[nx - 1] = F(0)
        dst[r] = n
        if j0 + lj == 1:
            dst[r - 1] = n
        if j0 + lj == ny - 2:
            dst[r + 1] = n


def exchange(arr, g0, spec, rank, n):
    """arr rows indexed local+g0; spec = cfd_plan_halo output."""
    reqs = []
    for peer, (s, rcv, rows) in ((rank - 1, spec[0:3]), (rank + 1, spec[3:6])):
        if rows == 0:
            continue
        buf = torch.from_numpy(np.ascontiguousarray(arr[s + g0:s + g0 + rows]))
        reqs.append(dist.isend(buf, peer))
    for peer, (s, rcv, rows) in ((rank - 1, spec[0:3]), (rank + 1, spec[3:6])):
        if rows == 0:
            continue
        buf = torch.empty((rows, arr.shape[1]), dtype=torch.float32)
        dist.recv(buf, peer)
        arr[rcv + g0:rcv + g0 + rows] = buf.numpy()
    for q in reqs:
        q.wait()


def exchange_start(arr, g0, spec, rank, n):
    """Post the sends of the band rows and the receives of the ghost rows
    (non-blocking, like the RCCL group on the comm stream)."""
    sends, recvs = [], []
    for peer, (s, rcv, rows) in ((rank - 1, spec[0:3]), (rank + 1, spec[3:6])):
        if rows == 0:
            continue
        buf = torch.from_numpy(np.ascontiguousarray(arr[s + g0:s + g0 + rows]))
        sends.append(dist.isend(buf, peer))
    for peer, (s, rcv, rows) in ((rank - 1, spec[0:3]), (rank + 1, spec[3:6])):
        if rows == 0:
            continue
        buf = torch.empty((rows, arr.shape[1]), dtype=torch.float32)
        recvs.append((dist.irecv(buf, peer), buf, rcv))
    return sends, recvs


def exchange_finish(arr, g0, pend):
    sends, recvs = pend
    for q, buf, rcv in recvs:
        q.wait()
        arr[rcv + g0:rcv + g0 + buf.shape[0]] = buf.numpy()
    for q in sends:
        q.wait()


def _worker(rank, n, port, cases, results):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    try:
        out = []
        for (nx, ny, hg, iters, seed, t_max, ovl) in cases:
            rng = np.random.default_rng(seed)
            P = rng.uniform(-1, 1, (ny, nx)).astype(F)
            RHS = rng.uniform(-1, 1, (ny, nx)).astype(F)
            dx, dy = F(F(2.0) / F(nx)), F(F(1.0) / F(ny))
            j0, j1 = plan_slab(ny, n, rank)
            nyl = j1 - j0
            g0 = hg
            bufs = [np.zeros((nyl + 2 * hg, nx), F) for _ in range(2)]
            rhs = np.zeros((nyl + 2 * hg, nx), F)
            # owned rows only, then the ghost exchanges the GPU path performs:
            # p' (end of the previous solve / cfd_set_state) and rhs (solve start)
            bufs[0][g0:g0 + nyl] = P[j0:j1]
            rhs[g0:g0 + nyl] = RHS[j0:j1]
            exchange(bufs[0], g0, plan_halo(2, nyl, hg, rank, n), rank, n)
            exchange(rhs, g0, plan_halo(2, nyl, hg, rank, n), rank, n)
            cur = 0
            it = 0
            while it < iters:
                if t_max == 1:
                    lo, hi, ex = plan_sweep(j0, nyl, ny, hg, it, iters)
                    sweep_rows(bufs[cur], bufs[cur ^ 1], rhs, g0, lo, hi, nx, ny, j0, dx, dy)
                    cur ^= 1
                    it += 1
                else:
                    # k_jacobi_tb: T sweeps, sweep s recomputing T-1-s extra rows
                    # each side of the stored band (clipped to global 1..ny-2)
                    T, lo, hi, ex = plan_block(j0, nyl, ny, hg, it, t_max, iters)
                    split, ov = plan_overlap(nyl, hg, rank, n, lo, hi) if (ovl and ex) else (False, None)
                    if split:
                        # the overlapped schedule of enqueue_jacobi_slabs (cfd_model_jacobi.hip): bands the
                        # exchange sends first, their exchange in flight while
                        # the interior is computed, then the wait
                        src, dst = bufs[cur], bufs[cur ^ 1]
                        for b in range(2):
                            a_, b_ = ov[2 * b], ov[2 * b + 1]
                            if b_ > a_:
                                band = block_band(src, rhs, g0, a_, b_, T, nx, ny, j0, dx, dy)
                                dst[a_ + g0:b_ + g0] = band[a_ + g0:b_ + g0]
                                if j0 + a_ <= 1 < j0 + b_:       # fused P(i,0) = P(i,1) store
                                    dst[g0 - j0] = band[g0 - j0]
                                if j0 + a_ <= ny - 2 < j0 + b_:  # fused P(i,ny-1) store
                                    dst[g0 + ny - 1 - j0] = band[g0 + ny - 1 - j0]
                        pend = exchange_start(dst, g0, plan_halo(2, nyl, hg, rank, n), rank, n)
                        a_, b_ = ov[4], ov[5]
                        inner = block_band(src, rhs, g0, a_, b_, T, nx, ny, j0, dx, dy)
                        dst[a_ + g0:b_ + g0] = inner[a_ + g0:b_ + g0]
                        if j0 + a_ <= 1 < j0 + b_:
                            dst[g0 - j0] = inner[g0 - j0]
                        if j0 + a_ <= ny - 2 < j0 + b_:
                            dst[g0 + ny - 1 - j0] = inner[g0 + ny - 1 - j0]
                        exchange_finish(dst, g0, pend)
                        cur ^= 1
                        it += T
                        continue
                    for s_ in range(T):
                        e = T - 1 - s_
                        a, b = max(lo - e, 1 - j0), min(hi + e, ny - 1 - j0)
                        sweep_rows(bufs[cur], bufs[cur ^ 1], rhs, g0, a, b, nx, ny, j0, dx, dy)
                        cur ^= 1
                    it += T
                if ex:
                    exchange(bufs[cur], g0, plan_halo(2, nyl, hg, rank, n), rank, n)
            mine = torch.from_numpy(np.ascontiguousarray(bufs[cur][g0:g0 + nyl]))
            if rank == 0:
                parts = [mine.numpy()]
                for r in range(1, n):
                    a, b = plan_slab(ny, n, r)
                    t = torch.empty((b - a, nx), dtype=torch.float32)
                    dist.recv(t, r)
                    parts.append(t.numpy())
                out.append(np.concatenate(parts).ravel())
            else:
                dist.send(mine, 0)
            # u / v ghost geometry: ship global row ids
            for kind, rows_owned, pitch in ((0, nyl, nx + 1), (1, nyl + 1, nx)):
                arr = np.full((nyl + 1 + 4, pitch), -1.0, F)
                for lj in range(rows_owned):
                    arr[lj + 2] = j0 + lj
                exchange(arr, 2, plan_halo(kind, nyl, 2, rank, n), rank, n)
                want_rows = list(range(-2, 0)) if rank > 0 else []
                if rank < n - 1:
                    want_rows += list(range(nyl, nyl + 2)) if kind == 0 else \
                        list(range(nyl + 1, nyl + 3))
                for lj in want_rows:
                    assert (arr[lj + 2] == j0 + lj).all(), (kind, rank, lj, arr[lj + 2][:3])
        if rank == 0:
            results.put(out)
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


CASES = [  # nx, ny, halo depth, sweeps, seed, sweeps per launch, overlapped exchange
    (16, 40, 1, 5, 1, 1, 0),
    (24, 40, 3, 7, 2, 1, 0),
    (32, 44, 8, 20, 3, 1, 0),
    (16, 30, 4, 4, 4, 1, 0),
    (16, 37, 2, 9, 5, 1, 0),
    (16, 40, 8, 21, 6, 4, 0),
    (24, 44, 6, 13, 7, 4, 0),
    (16, 37, 3, 10, 8, 2, 0),
    (16, 40, 5, 12, 9, 3, 0),
    (16, 40, 4, 21, 10, 4, 1),
    (24, 44, 6, 13, 11, 4, 1),
    (16, 37, 3, 10, 12, 2, 1),
    (16, 48, 8, 25, 13, 8, 1),
]


@pytest.mark.parametrize("n", [2, 3])
def test_sharded_jacobi_plan_matches_single_domain(n):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from oracle import OracleModel
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, n, port, CASES, q)) for r in range(n)]
    for p in procs:
        p.start()
    got = q.get(timeout=240)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for (nx, ny, hg, iters, seed, _, _), res in zip(CASES, got):
        rng = np.random.default_rng(seed)
        P = rng.uniform(-1, 1, (ny, nx)).astype(F)
        RHS = rng.uniform(-1, 1, (ny, nx)).astype(F)
        o = OracleModel(nx, ny, 2.0, 1.0, jacobi_iters=iters, tol_enabled=0)
        o.field("p_prime")[:] = P.ravel()
        o.field("rhs")[:] = RHS.ravel()
        o.jacobi()
        want = o.field("p_prime")
        assert np.array_equal(res.view(np.uint32), want.view(np.uint32)), (nx, ny, hg, iters)


def test_plan_slab_partition_properties():
    for ny in (4, 5, 37, 4096, 8192):
        for n in (1, 2, 3, 4, 8):
            if ny < n:
                continue
            rows = [plan_slab(ny, n, r) for r in range(n)]
            assert rows[0][0] == 0 and rows[-1][1] == ny
            assert all(rows[k][1] == rows[k + 1][0] for k in range(n - 1))
            sizes = [b - a for a, b in rows]
            assert max(sizes) - min(sizes) <= 1


def test_single_domain_blocks_split_evenly():
    """Unsharded solves (hg = 0): ceil(iters / t_max) launches -- as many as
    t_max-sized blocks -- whose sweep counts differ by at most one and run
    longest first (50 = 8 + 6 x 7, never a short tail launch); the whole
    interior rows every time.  The persistent solve takes the leading run
    of 8-sweep blocks from this split."""
    for t_max in range(1, 9):
        for iters in range(1, 260):
            it, Ts = 0, []
            while it < iters:
                T, lo, hi, ex = plan_block(0, 96, 96, 0, it, t_max, iters)
                assert 1 <= T <= t_max and (lo, hi, ex) == (1, 95, False)
                Ts.append(T)
                it += T
            assert it == iters
            assert len(Ts) == -(-iters // t_max), (t_max, iters, Ts)
            assert max(Ts) - min(Ts) <= 1 and Ts == sorted(Ts, reverse=True), (t_max, iters, Ts)


# ---------------------------------------------------------------------------
# r5: the tolerance mode on slabs as speculative T-sweep blocks
# (enqueue_spec_slabs, cfd_model_jacobi.hip; opt-in CFD_SPEC_SLABS=1).  The same
# schedule in numpy over gloo: per block ONE p' exchange T rows deep (the
# first block's also carries the rhs ghosts, r6), T sweeps of the owned rows
# (sweep s recomputing T-1-s ghost rows each side), ONE all-reduce of the
# block's T residuals, the first sweep below p_tol ends the solve (later
# blocks skip); the converged block re-runs with exactly its sweeps from its
# untouched source, the result is copied to the buffer the host counted (one
# flip per block), and one 1-row exchange follows.
# r6: the host reads each block's all-reduced residuals (block 0 at once,
# later blocks one block behind) and enqueues no block past the one where
# the solve ended, so the collective calls track convergence: never more than
# the host-driven loop's 2 per enqueued sweep (it enqueues one sweep past the
# exit), and a fraction of them when solves run long.

def simd_end(nx):
    e = 1
    while e + 8 <= nx - 1:
        e += 8
    return e


def spec_block(src, rhs, g0, lo, hi, T, nx, ny, j0, dx, dy):
    """T sweeps from src over owned rows [lo, hi) (cones into the ghosts);
    returns the last sweep's buffer and every sweep's residual over the owned
    rows (columns [1, simd_end), model.rs:755-772)."""
    cur, nxt = src.copy(), src.copy()
    se = simd_end(nx)
    errs = []
    for s_ in range(T):
        e = T - 1 - s_
        a, b = max(lo - e, 1 - j0), min(hi + e, ny - 1 - j0)
        sweep_rows(cur, nxt, rhs, g0, a, b, nx, ny, j0, dx, dy)
        d = np.abs(nxt[lo + g0:hi + g0, 1:se] - cur[lo + g0:hi + g0, 1:se])
        errs.append(F(d.max()) if d.size else F(0))
        cur, nxt = nxt, cur
    return cur, errs


def _spec_worker(rank, n, port, cases, results):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    try:
        out = []
        for (nx, ny, hg, iters, seed, p_tol) in cases:
            P, RHS = _spec_inputs(nx, ny, seed)
            dx, dy = F(F(2.0) / F(nx)), F(F(1.0) / F(ny))
            j0, j1 = plan_slab(ny, n, rank)
            nyl = j1 - j0
            g0 = hg
            lo, hi = max(0, 1 - j0), min(nyl, ny - 1 - j0)
            bufs = [np.zeros((nyl + 2 * hg, nx), F) for _ in range(2)]
            rhs = np.zeros((nyl + 2 * hg, nx), F)
            bufs[0][g0:g0 + nyl] = P[j0:j1]
            rhs[g0:g0 + nyl] = RHS[j0:j1]
            exchange(bufs[0], g0, plan_halo(2, nyl, hg, rank, n), rank, n)
            Tm = min(8, hg)
            nb = -(-iters // Tm)
            it, launches, stop, collectives = 0, 0, None, 0
            blk_errs, checked, host_stop = [], 0, False
            for b in range(nb):
                if host_stop:   # the host enqueues nothing past the exit
                    break
                T = iters // nb + (1 if b < iters % nb else 0)
                src = bufs[launches & 1]
                if b == 0:   # one group: the rhs ghosts hg deep + the source T deep
                    exchange(rhs, g0, plan_halo(2, nyl, hg, rank, n), rank, n)
                exchange(src, g0, plan_halo(2, nyl, T, rank, n), rank, n)
                collectives += 2   # that exchange group + the block's all-reduce
                errs = np.zeros(T, F)   # a skipped block publishes nothing
                if stop is None:   # the device skips the blocks after the exit
                    res, errs = spec_block(src, rhs, g0, lo, hi, T, nx, ny, j0, dx, dy)
                    e = torch.tensor(np.array(errs, F))
                    dist.all_reduce(e, op=dist.ReduceOp.MAX)
                    errs = e.numpy()
                    # owned rows and the fused global boundary rows
                    dst = bufs[(launches + 1) & 1]
                    dst[g0:g0 + nyl] = res[g0:g0 + nyl]
                    hit = [k for k in range(T) if errs[k] < F(p_tol)]
                    if hit:
                        stop = (launches, hit[0] + 1, F(errs[hit[0]]), it + hit[0] + 1)
                    last = (F(errs[-1]), it + T)
                blk_errs.append(errs)
                it += T
                launches += 1
                # the host's check: block 0 at once, later blocks one behind
                while not host_stop and checked <= (0 if b == 0 else b - 1):
                    host_stop = any(x < F(p_tol) for x in blk_errs[checked])
                    checked += 1
            if stop is not None:
                L, nsw, resid, sweeps = stop
                src = bufs[L & 1]
                res, _ = spec_block(src, rhs, g0, lo, hi, nsw, nx, ny, j0, dx, dy)
                bufs[(L + 1) & 1][g0:g0 + nyl] = res[g0:g0 + nyl]
                if (launches - (L + 1)) & 1:   # k_spec_align
                    bufs[launches & 1][g0:g0 + nyl] = bufs[(L + 1) & 1][g0:g0 + nyl]
            else:
                resid, sweeps = last
            final = bufs[launches & 1]
            exchange(final, g0, plan_halo(2, nyl, 1, rank, n), rank, n)
            collectives += 1
            # the ghost row the corrector reads holds the neighbour's owned row
            if rank > 0:
                a_, _ = plan_slab(ny, n, rank - 1)
                prev = torch.empty(nx, dtype=torch.float32)
                dist.recv(prev, rank - 1)
                assert np.array_equal(final[g0 - 1], prev.numpy())
            if rank < n - 1:
                dist.send(torch.from_numpy(np.ascontiguousarray(final[g0 + nyl - 1])), rank + 1)
            mine = torch.from_numpy(np.ascontiguousarray(final[g0:g0 + nyl]))
            if rank == 0:
                parts = [mine.numpy()]
                for r in range(1, n):
                    a, b_ = plan_slab(ny, n, r)
                    t = torch.empty((b_ - a, nx), dtype=torch.float32)
                    dist.recv(t, r)
                    parts.append(t.numpy())
                out.append((np.concatenate(parts).ravel(), float(resid), int(sweeps), collectives))
            else:
                dist.send(mine, 0)
        if rank == 0:
            results.put(out)
    finally:
        dist.destroy_process_group()


def _spec_inputs(nx, ny, seed):
    """A smooth-ish start whose Jacobi residual decays through the tolerances
    below within 50 sweeps (random noise of amplitude 1e-3, zero rhs)."""
    rng = np.random.default_rng(seed)
    P = (1e-3 * rng.uniform(-1, 1, (ny, nx))).astype(F)
    RHS = np.zeros((ny, nx), F)
    return P, RHS


def _oracle_solve(nx, ny, iters, seed, p_tol):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from oracle import OracleModel
    P, RHS = _spec_inputs(nx, ny, seed)
    o = OracleModel(nx, ny, 2.0, 1.0, jacobi_iters=iters, tol_enabled=1, p_tol=p_tol)
    o.field("p_prime")[:] = P.ravel()
    o.field("rhs")[:] = RHS.ravel()
    s0 = o.scalars().jacobi_sweeps_total
    r = o.jacobi()
    return o.field("p_prime").copy(), F(r), int(o.scalars().jacobi_sweeps_total - s0)


def _spec_cases():
    """Tolerances just above the single-domain residual after k sweeps, so the
    solve ends at or before sweep k: exits in the first block, mid-block, at
    a block's last sweep, and none (k = 50)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    from oracle import OracleModel
    cases = []
    for (nx, ny, hg, seed) in ((32, 48, 8, 21), (24, 40, 5, 22), (16, 44, 3, 23)):
        P, RHS = _spec_inputs(nx, ny, seed)
        for k in (1, 3, 8, 13, 22, 50):
            o = OracleModel(nx, ny, 2.0, 1.0, jacobi_iters=k, tol_enabled=0)
            o.field("p_prime")[:] = P.ravel()
            o.field("rhs")[:] = RHS.ravel()
            r = F(o.jacobi())
            cases.append((nx, ny, hg, 50, seed, float(np.nextafter(r, F(1)))))
    return cases


@pytest.mark.parametrize("n", [2, 3])
def test_sharded_spec_blocks_match_single_domain(n):
    cases = _spec_cases()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_spec_worker, args=(r, n, port, cases, q)) for r in range(n)]
    for p in procs:
        p.start()
    got = q.get(timeout=240)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    exits = set()
    for (nx, ny, hg, iters, seed, p_tol), (res, resid, sweeps, coll) in zip(cases, got):
        want, wres, wsweeps = _oracle_solve(nx, ny, iters, seed, p_tol)
        assert np.array_equal(res.view(np.uint32), want.view(np.uint32)), (nx, ny, hg, p_tol)
        assert F(resid).view(np.uint32) == wres.view(np.uint32) and sweeps == wsweeps, \
            (nx, ny, hg, p_tol, resid, wres, sweeps, wsweeps)
        exits.add(sweeps)
        # the host-driven loop (enqueue_solve_host_driven): an all-reduce and a
        # 1-row exchange per sweep, one sweep enqueued past the exit
        host_driven = 2 * min(sweeps + 1, iters)
        # blocks enqueued: up to the exit's block, one more when the exit was
        # seen one block behind (not in block 0, not in the last block)
        Tm = min(8, hg)
        nb = -(-iters // Tm)
        split = [iters // nb + (1 if b < iters % nb else 0) for b in range(nb)]
        L = next(b for b in range(nb) if sum(split[:b + 1]) >= sweeps)
        enq = nb if F(resid) >= F(p_tol) else (1 if L == 0 else min(L + 2, nb))
        assert coll == 2 * enq + 1, (coll, enq, sweeps)
        assert coll <= host_driven, (coll, host_driven, sweeps)
        if sweeps == iters:   # a full-length solve: a fraction of the calls
            assert 2 * coll < host_driven, (coll, host_driven)
            if Tm == 8:   # 8-sweep blocks: 15 calls against 100
                assert 6 * coll <= host_driven, (coll, host_driven)
    assert len(exits) >= 4 and 50 in exits, sorted(exits)
