// cfd_model_comm.hip — halo exchanges, the all-reduce, RCCL deadlines and the LocalHub forms
// (the host runtime behind include/cfd.h; see cfd_model.h)
#include <chrono>
#include <cstring>
#include <memory>
#include <thread>

#include "cfd_model.h"

using namespace cfd;

float *cfd_model::field_ptr(int id) {
    switch (id) {
    case FLD_U: return f.u;
    case FLD_V: return f.v;
    case FLD_PP0: return f.pp[0];
    case FLD_PP1: return f.pp[1];
    default: return f.rhs;
    }
}

// Ghost-row exchange of `items` (field, plan_halo kind, depth) with both
// neighbours: ONE RCCL group of at most two sends and two receives per item,
// counted as one collective call.  The LocalHub does its fields one after
// another.  exchange, exchange_uv, exchange_pp and exchange_rhs_pp
// (cfd_model.h) are this call with their items.
int cfd_model::exchange_group(std::initializer_list<HaloX> items, hipStream_t st) {
    if (!sharded()) return 0;
    ++comm_calls;
    if (!st) st = stream;
    if (hub) {
        for (const HaloX &x : items)
            if (int rc = exchange_local(x.id, x.kind, x.depth, st)) return rc;
        return 0;
    }
    if (!comm) return fail(CFD_ERCCL, "the RCCL communicator was aborted after an earlier failure");
    phase_mark(2, false, st);
    RCCL_TRY(ncclGroupStart());
    int rc = 0;
    for (const HaloX &x : items)
        if (!rc) rc = exchange_ops(x.id, x.kind, x.depth, st);
    RCCL_OP(ncclGroupEnd());
    phase_mark(2, true, st);
    return rc;
}

// The sends and receives of one field's ghost exchange (inside a group).
int cfd_model::exchange_ops(int id, int kind, int depth, hipStream_t st) {
    float *base = field_ptr(id);
    const size_t pitch = field_pitch(id);
    int h[6];
    plan_halo(kind, g.nyl, depth, rank, n_ranks, h);
    if (h[2] > 0) {
        RCCL_OP(ncclSend(base + (long)h[0] * (long)pitch, (size_t)h[2] * pitch, ncclFloat,
                          rank - 1, comm, st));
        RCCL_OP(ncclRecv(base + (long)h[1] * (long)pitch, (size_t)h[2] * pitch, ncclFloat,
                          rank - 1, comm, st));
    }
    if (h[5] > 0) {
        RCCL_OP(ncclSend(base + (long)h[3] * (long)pitch, (size_t)h[5] * pitch, ncclFloat,
                          rank + 1, comm, st));
        RCCL_OP(ncclRecv(base + (long)h[4] * (long)pitch, (size_t)h[5] * pitch, ncclFloat,
                          rank + 1, comm, st));
    }
    return 0;
}

// LocalHub form: copy the neighbours' send rows straight into our ghosts.
int cfd_model::exchange_local(int id, int kind, int depth, hipStream_t st) {
    HIP_TRY(hipStreamSynchronize(st));
    hub->barrier();   // every member's rows are final
    float *base = field_ptr(id);
    const size_t pitch = field_pitch(id);
    int h[6];
    plan_halo(kind, g.nyl, depth, rank, n_ranks, h);
    for (int side = 0; side < 2; ++side) {
        const int rows = h[3 * side + 2];
        if (rows == 0) continue;
        cfd_model *peer = hub->members[side == 0 ? rank - 1 : rank + 1];
        int ph[6];
        plan_halo(kind, peer->g.nyl, depth, peer->rank, n_ranks, ph);
        const int psend = side == 0 ? ph[3] : ph[0];   // peer's rows facing us
        HIP_TRY(hipMemcpyAsync(base + (long)h[3 * side + 1] * (long)pitch,
                               peer->field_ptr(id) + (long)psend * (long)pitch,
                               (size_t)rows * pitch * 4, hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    hub->barrier();   // nobody overwrites rows a peer is still copying
    return 0;
}

int cfd_model::allreduce_max_u32(uint32_t *dev, size_t n) {
    if (!sharded()) return 0;
    ++comm_calls;
    if (hub) {
        std::vector<uint32_t> acc(n, 0u), mine(n);
        HIP_TRY(hipStreamSynchronize(stream));
        hub->barrier();
        const size_t off = (size_t)(dev - (uint32_t *)f.ctl);   // same slot in every member
        for (cfd_model *peer : hub->members) {
            HIP_TRY(hipMemcpy(mine.data(), (uint32_t *)peer->f.ctl + off, n * 4,
                              hipMemcpyDeviceToHost));
            for (size_t k = 0; k < n; ++k) acc[k] = std::max(acc[k], mine[k]);
        }
        hub->barrier();
        HIP_TRY(hipMemcpy(dev, acc.data(), n * 4, hipMemcpyHostToDevice));
        return 0;
    }
    if (!comm) return fail(CFD_ERCCL, "the RCCL communicator was aborted after an earlier failure");
    phase_mark(2, false);
    RCCL_OP(ncclAllReduce(dev, dev, n, ncclUint32, ncclMax, comm, stream));
    phase_mark(2, true);
    return 0;
}

// Resolve the result of a call on the (non-blocking) communicator: poll
// its asynchronous state while it is ncclInProgress, up to the deadline.
int cfd_model::settle(ncclResult_t r, const char *what) {
    if (r == ncclSuccess) return 0;
    if (r == ncclInProgress && comm) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            ncclResult_t st = ncclInProgress;
            r = ncclCommGetAsyncError(comm, &st);
            if (r == ncclSuccess) r = st;
            if (r != ncclInProgress) break;
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >
                opt.rccl_timeout_s) {
                ncclCommAbort(comm);
                comm = nullptr;
                comm_aborted = true;
                return fail(CFD_ERCCL, std::string(what) + ": still in progress after " +
                                           std::to_string((int)opt.rccl_timeout_s) +
                                           " s; the communicator was aborted");
            }
            std::this_thread::sleep_for(std::chrono::microseconds(20));
        }
        if (r == ncclSuccess) return 0;
    }
    return fail(CFD_ERCCL, std::string(what) + ": " + ncclGetErrorString(r));
}

// Wait for the stream (ev == nullptr) or for one event, with the RCCL
// communicator watched: a peer that failed (ncclCommGetAsyncError) or made
// no progress for CFD_RCCL_TIMEOUT_S seconds aborts the communicator and
// fails with CFD_ERCCL instead of blocking forever.
int cfd_model::wait_done(hipEvent_t ev) {
    if (!comm) {
        HIP_TRY(ev ? hipEventSynchronize(ev) : hipStreamSynchronize(stream));
        return 0;
    }
    // the deadline runs from the last forward progress the host saw (a
    // finished step: the device mirrors Ctl::step into h_nonfinite[1]),
    // not from the start of the wait, so a long healthy queue never trips it
    auto t0 = std::chrono::steady_clock::now();
    uint32_t seen = *(volatile uint32_t *)(h_nonfinite + 1);
    for (int spin = 0;; ++spin) {
        const hipError_t q = ev ? hipEventQuery(ev) : hipStreamQuery(stream);
        if (q == hipSuccess) return 0;
        if (q != hipErrorNotReady)
            return fail(CFD_EHIP, std::string("stream/event query: ") + hipGetErrorString(q));
        const uint32_t now_step = *(volatile uint32_t *)(h_nonfinite + 1);
        if (now_step != seen) {
            seen = now_step;
            t0 = std::chrono::steady_clock::now();
        }
        ncclResult_t ar = ncclSuccess;
        const ncclResult_t r = ncclCommGetAsyncError(comm, &ar);
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (r != ncclSuccess || ar != ncclSuccess || el > opt.rccl_timeout_s) {
            const std::string why = (r != ncclSuccess || ar != ncclSuccess)
                                        ? std::string("RCCL asynchronous error: ") +
                                              ncclGetErrorString(r != ncclSuccess ? r : ar)
                                        : "RCCL exchange made no progress for " +
                                              std::to_string((int)opt.rccl_timeout_s) + " s";
            ncclCommAbort(comm);
            comm = nullptr;
            comm_aborted = true;
            return fail(CFD_ERCCL, why + " (rank " + std::to_string(rank) +
                                       "); the communicator was aborted");
        }
        if (spin < 256)
            std::this_thread::yield();
        else
            std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

namespace {

// Communicator creation with a deadline.  ncclCommInitRank blocks in its
// bootstrap until every rank has arrived, and RCCL's non-blocking config does
// not change that (measured: ncclCommInitRankConfig with blocking = 0 did not
// return while the peer was missing).  So the blocking call runs on a helper
// thread and the caller waits at most CFD_RCCL_TIMEOUT_S: a rank that never
// arrives makes cfd_create_sharded fail with CFD_ERCCL instead of hanging.
// The stuck bootstrap is abandoned (the detached thread stays blocked; should
// a late peer still complete it, the thread aborts that communicator itself).
struct CommInitJob {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false, abandoned = false;
    ncclComm_t comm = nullptr;
    ncclResult_t r = ncclSuccess;
    hipError_t he = hipSuccess;
};

}  // namespace

namespace cfd {

int comm_init(cfd_model *m, const ncclUniqueId &id, int n_ranks, int rank) {
    auto job = std::make_shared<CommInitJob>();
    const int device = m->device;
    std::thread([job, id, n_ranks, rank, device] {
        ncclComm_t c = nullptr;
        ncclResult_t r = ncclInternalError;
        const hipError_t he = hipSetDevice(device);
        if (he == hipSuccess) r = ncclCommInitRank(&c, n_ranks, id, rank);
        std::lock_guard<std::mutex> lk(job->mu);
        if (job->abandoned) {
            if (r == ncclSuccess && c) ncclCommAbort(c);
            return;
        }
        job->comm = c;
        job->r = r;
        job->he = he;
        job->done = true;
        job->cv.notify_all();
    }).detach();
    std::unique_lock<std::mutex> lk(job->mu);
    const auto limit = std::chrono::duration<double>(m->opt.rccl_timeout_s);
    if (!job->cv.wait_for(lk, limit, [&] { return job->done; })) {
        job->abandoned = true;
        return fail(CFD_ERCCL, "ncclCommInitRank: rank " + std::to_string(rank) + " of " +
                                   std::to_string(n_ranks) + ": not every rank joined within " +
                                   std::to_string((int)m->opt.rccl_timeout_s) +
                                   " s (CFD_RCCL_TIMEOUT_S); creation abandoned");
    }
    if (job->he != hipSuccess)
        return fail(CFD_EHIP, std::string("hipSetDevice (RCCL init thread): ") + hipGetErrorString(job->he));
    if (job->r != ncclSuccess)
        return fail(CFD_ERCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(job->r));
    m->comm = job->comm;
    return 0;
}

}  // namespace cfd

extern "C" {

int cfd_rccl_unique_id(void *out) {
    if (!out) return fail(CFD_EINVAL, "null out");
    ncclUniqueId id;
    RCCL_TRY(ncclGetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
    std::memcpy(out, &id, sizeof(id));
    return 0;
}

void *cfd_local_hub_create(int n_ranks) {
    if (n_ranks < 1) return nullptr;
    LocalHub *h = new LocalHub();
    h->n = n_ranks;
    h->members.assign(n_ranks, nullptr);
    return h;
}

void cfd_local_hub_destroy(void *hub) { delete static_cast<LocalHub *>(hub); }

}  // extern "C"
