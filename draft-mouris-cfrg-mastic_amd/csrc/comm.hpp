// ---- multi-GPU merge over the ctx's own RCCL communicator --
// Its state is mastic_ctx::cm (ctx.hpp CommState); the agreement round's rules are comm_agree.hpp's.
#pragma once
//
// Failure model.  Every collective entry point (mastic_allgather_fold,
// mastic_merge_host, mastic_aggregate_merged) first does all of its
// rank-local work -- argument checks, staging allocations, the local fold --
// and then joins an agreement round: one 32-byte CommStatus per rank (its
// error code, the entry point, n_local, n_elems), all-gathered into buffers
// sized at mastic_comm_init.  A rank whose local work failed still joins it,
// so no peer is left waiting inside a data all-gather: a rank that failed
// returns its own error, every other rank the code of the lowest failing
// rank, and ranks whose calls disagree on the entry point or the share
// geometry all return MASTIC_EINVAL, before any share bytes move.  Only when
// every rank is ready do the data all-gather and the GF(p) fold run.  Every
// wait on the communicator is bounded by the ctx's timeout
// (mastic_comm_init_timeout): a peer that never joins (it crashed, or is stuck
// elsewhere) becomes MASTIC_ETIMEDOUT.  An init that times out is abandoned
// (its thread keeps it; the ctx stays world 1); a collective that times out
// aborts the communicator (ncclCommAbort), and later collective calls then
// fail with MASTIC_EHIP -- never a silent world-1 merge -- until
// mastic_comm_destroy and a new mastic_comm_init.

namespace {
// RCCL is bound on first use of a communicator entry point (dlopen), so a
// single-GPU user of the library has no load-time dependency on librccl; a
// process that already holds it (e.g. PyTorch's copy) shares that one.
struct RcclApi {
    bool ok = false;
    std::string why;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommGetAsyncError) CommGetAsyncError = nullptr;
    decltype(&ncclCommAbort) CommAbort = nullptr;
    decltype(&ncclCommFinalize) CommFinalize = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};

const RcclApi& rccl() {
    static const RcclApi api = [] {
        RcclApi a;
        void* h = nullptr;
        // test hook: MASTIC_RCCL_LIB names the library to bind instead (the
        // shared-memory stand-in of tests/host/fake_rccl.cpp, which lets several
        // processes on one GPU form a communicator); no fallback to RCCL
        const char* hook = getenv("MASTIC_RCCL_LIB");
        if (hook && *hook) {
            h = dlopen(hook, RTLD_NOW | RTLD_LOCAL);
        } else {
            for (const char* name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"})
                if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
        }
        if (!h) {
            const char* e = dlerror();
            a.why = e ? e : "librccl.so.1 not found";
            return a;
        }
        bool all = true;
        auto bind = [&](auto& fn, const char* name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(h, name));
            if (!fn && all) a.why = std::string("librccl lacks ") + name;
            all = all && fn;
        };
        bind(a.GetUniqueId, "ncclGetUniqueId");
        bind(a.CommInitRank, "ncclCommInitRank");
        bind(a.CommGetAsyncError, "ncclCommGetAsyncError");
        bind(a.CommAbort, "ncclCommAbort");
        bind(a.CommFinalize, "ncclCommFinalize");
        bind(a.CommDestroy, "ncclCommDestroy");
        bind(a.AllGather, "ncclAllGather");
        bind(a.GetErrorString, "ncclGetErrorString");
        a.ok = all;
        return a;
    }();
    return api;
}

// One communicator init on its own thread (mastic_comm_init_timeout).
struct CommInitJob {
    std::mutex mu;
    std::condition_variable cv;
    bool done = false, abandoned = false;
    ncclComm_t comm = nullptr;
    ncclResult_t r = ncclSuccess;
    hipError_t dev_err = hipSuccess;
};
}  // namespace

// ctx teardown (stream: the ctx's main stream, still alive): the trace marks,
// then a live communicator -- its queued work is waited for, then it is
// released locally (ncclCommAbort never waits on peers that may be gone) --
// and the pinned status records.  The staging buffers free themselves.
void CommState::release(hipStream_t stream) {
    for (hipEvent_t e : marks)
        if (e) (void)hipEventDestroy(e);
    if (comm) {
        (void)hipStreamSynchronize(stream);
        (void)rccl().CommAbort(comm);
        comm = nullptr;
    }
    if (st_host) (void)hipHostFree(st_host);
}

// Abort the ctx's communicator after a failed or timed-out RCCL step: its
// kernels see the abort flag and exit, the ctx keeps cm.broken so later
// collective calls fail instead of silently folding as world 1.
// MASTIC_TRACE_COMM: mark step i of the agreement round on the ctx's stream;
// a timed-out wait reports which marks the stream has passed.
static void comm_mark(mastic_ctx* c, int i) {
    if (!trace_comm()) return;
    if (!c->cm.marks[i] && hipEventCreateWithFlags(&c->cm.marks[i], hipEventDisableTiming) != hipSuccess) return;
    (void)hipEventRecord(c->cm.marks[i], c->stream);
}
static void comm_marks_report(mastic_ctx* c) {
    if (!trace_comm()) return;
    for (int i = 0; i < 3; i++)
        if (c->cm.marks[i])
            fprintf(stderr, "[mastic comm]   mark %d (%s): %s\n", i,
                    (const char*[]){"status uploaded", "status all-gather queued", "status download queued"}[i],
                    hipEventQuery(c->cm.marks[i]) == hipSuccess ? "passed" : "not passed");
}

static int comm_abort(mastic_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (trace_comm()) fprintf(stderr, "[mastic comm] abort: %s\n", buf);
    if (c->cm.comm) {
        const ncclResult_t r = rccl().CommAbort(c->cm.comm);
        if (trace_comm()) fprintf(stderr, "[mastic comm] ncclCommAbort -> %d\n", (int)r);
    }
    c->cm.comm = nullptr;
    c->cm.broken = true;
    return fail(c, code, "%s; the communicator was aborted", buf);
}

// The result of an RCCL call on the ctx's communicator; a call that reports
// ncclInProgress (a non-blocking communicator's) is polled until it settles,
// within the ctx's timeout.
static int comm_settle(mastic_ctx* c, ncclResult_t r, const char* what) {
    const double t0 = now_ms();
    while (r == ncclInProgress) {
        if (now_ms() - t0 > c->cm.timeout_ms)
            return comm_abort(c, MASTIC_ETIMEDOUT, "RCCL %s did not complete within %d ms", what, c->cm.timeout_ms);
        std::this_thread::yield();
        ncclResult_t st = ncclSuccess;
        const ncclResult_t q = rccl().CommGetAsyncError(c->cm.comm, &st);
        r = q != ncclSuccess ? q : st;
    }
    if (r != ncclSuccess) return comm_abort(c, MASTIC_EHIP, "RCCL %s: %s", what, rccl().GetErrorString(r));
    return 0;
}

// Wait for c->stream, which carries an RCCL collective: bounded by the ctx's
// timeout (a peer that never joins), watching the communicator's own errors.
static int comm_wait(mastic_ctx* c, const char* what) {
    const double t0 = now_ms();
    for (int spin = 0;; spin++) {
        const hipError_t e = hipStreamQuery(c->stream);
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotReady) {
            (void)hipGetLastError();
            return comm_abort(c, MASTIC_EHIP, "%s: %s", what, hipGetErrorString(e));
        }
        ncclResult_t st = ncclSuccess;
        if (rccl().CommGetAsyncError(c->cm.comm, &st) == ncclSuccess && st != ncclSuccess && st != ncclInProgress)
            return comm_abort(c, MASTIC_EHIP, "RCCL %s: %s", what, rccl().GetErrorString(st));
        if (now_ms() - t0 > c->cm.timeout_ms) {
            comm_marks_report(c);
            return comm_abort(c, MASTIC_ETIMEDOUT, "%s: a peer rank did not join within %d ms", what,
                              c->cm.timeout_ms);
        }
        if (spin < 2000)
            std::this_thread::yield();
        else
            std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

// A staging buffer of a collective call (counts against the fail_allocs
// test hook when it must actually allocate).
static bool comm_grow(mastic_ctx* c, DevBuf& b, size_t want) {
    if (want <= b.bytes && b.p) return true;
    if (c->inject_alloc_failure()) return false;
    return b.grow(want);
}

// The agreement round (see the failure model above).  local_rc: the outcome
// of this rank's local work (0, or a code whose text is already in c->err).
// Returns 0 iff every rank is ready for the data exchange.
static int comm_agree(mastic_ctx* c, int local_rc, uint32_t op, size_t n_local, size_t n_elems) {
    if (!c->cm.comm) {
        if (c->cm.broken && !local_rc)
            return fail(c, MASTIC_EHIP, "the ctx's communicator was aborted after an earlier failure "
                                        "(mastic_comm_destroy, then mastic_comm_init)");
        return local_rc;  // world 1
    }
    // this rank's queued work (its prep_init, the local fold) first, unbounded:
    // the timeout below then measures only the wait for the peers
    {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess && !local_rc) {
            (void)hipGetLastError();
            local_rc = fail(c, MASTIC_EHIP, "%s: local work failed: %s", comm_op_name(op), hipGetErrorString(e));
        }
    }
    const std::string local_err = c->err;
    CommStatus* h = (CommStatus*)c->cm.st_host;  // [0]: this rank's record, [1 + r]: rank r's
    h[0] = CommStatus{local_rc, op, (uint64_t)n_local, (uint64_t)n_elems, COMM_MAGIC, 0};
    uint8_t* d = c->cm.st.as<uint8_t>();
    hipError_t e = hipMemcpyAsync(d, h, sizeof(CommStatus), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return comm_abort(c, local_rc ? local_rc : MASTIC_EHIP, "%s: status upload: %s", comm_op_name(op),
                          hipGetErrorString(e));
    }
    comm_mark(c, 0);
    int rc = comm_settle(c, rccl().AllGather(d, d + sizeof(CommStatus), sizeof(CommStatus), ncclUint8, c->cm.comm,
                                             c->stream), "status all-gather");
    if (rc) return local_rc ? local_rc : rc;
    comm_mark(c, 1);
    e = hipMemcpyAsync(h + 1, d + sizeof(CommStatus), sizeof(CommStatus) * (size_t)c->cm.n, hipMemcpyDeviceToHost,
                       c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return comm_abort(c, local_rc ? local_rc : MASTIC_EHIP, "%s: status download: %s", comm_op_name(op),
                          hipGetErrorString(e));
    }
    comm_mark(c, 2);
    rc = comm_wait(c, "status all-gather");
    if (rc) return local_rc ? local_rc : rc;
    const CommVerdict v = comm_decide(h + 1, c->cm.n, op, n_local, n_elems);
    const int rc_all = comm_rank_result(v, local_rc, MASTIC_EINVAL);
    if (local_rc) {
        c->err = local_err;
        return local_rc;
    }
    if (v.first_bad >= 0)
        return fail(c, rc_all, "%s failed on rank %d (code %d); no shares were exchanged", comm_op_name(op),
                    v.first_bad, v.bad_rc);
    if (v.mismatch >= 0) {
        const int mismatch = v.mismatch;
        const CommStatus& s = h[1 + mismatch];
        return fail(c, MASTIC_EINVAL,
                    "ranks disagree on the collective call: rank %d called %s with %llu x %llu elements, this rank "
                    "%s with %zu x %zu; no shares were exchanged",
                    mismatch, comm_op_name(s.op), (unsigned long long)s.n_local, (unsigned long long)s.n_elems,
                    comm_op_name(op), n_local, n_elems);
    }
    return 0;
}

// Staging for the data all-gather of n_local shares of n_elems elements from
// every rank (allocated in the local phase, before the agreement).
static bool comm_stage_gather(mastic_ctx* c, size_t n_local, size_t n_elems) {
    return !c->cm.comm || comm_grow(c, c->cm.gather, std::max<size_t>(n_local * n_elems * c->p.w32 * 4, 4) * c->cm.n);
}

// dev_out = sum mod p of the n_local shares of every rank (n_elems elements
// each), queued on c->stream after a successful agreement: one ncclAllGather
// of this rank's shares into the rank-ordered cm.gather, then
// k_fold_shares over the n_local x nranks shares (RCCL's integer sum is not
// GF(p) addition).  Without a communicator the local shares are folded
// directly (world 1).
static int allgather_fold_impl(mastic_ctx* c, const uint32_t* local, size_t n_local, size_t n_elems, uint32_t* out) {
    const size_t local_bytes = n_local * n_elems * c->p.w32 * 4;
    const uint32_t* src = local;
    size_t n_shares = n_local;
    if (c->cm.comm && local_bytes) {
        int rc = comm_settle(c, rccl().AllGather(local, c->cm.gather.p, local_bytes, ncclUint8, c->cm.comm, c->stream),
                             "share all-gather");
        if (rc) return rc;
        src = c->cm.gather.as<uint32_t>();
        n_shares = n_local * (size_t)c->cm.n;
    }
    return launch_fold_shares(c, src, n_shares, n_elems, out);
}

// The end of a collective call: its queued work (the data all-gather, the
// fold, the copy out) done, bounded by the timeout when RCCL is in it.
static int comm_finish(mastic_ctx* c, uint32_t op) {
    if (c->cm.comm) return comm_wait(c, comm_op_name(op));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// The merged share to the caller's host buffer, AFTER comm_finish: a copy to
// pageable memory is synchronous, so queued behind a data all-gather that a
// dead peer never completes it would block this thread past every bound
// (found by tests/test_gpu_comm_nrank.py: a peer lost between the agreement
// round and the data all-gather).
static int comm_copy_out(mastic_ctx* c, void* host_out, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(host_out, c->cm.out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// Shape limits of the fold kernel (k_fold_shares takes int counts).
static int comm_check_counts(mastic_ctx* c, size_t n_local, size_t n_elems) {
    if (n_local * (size_t)c->cm.n > (size_t)INT32_MAX || n_elems > (size_t)INT32_MAX)
        return fail(c, MASTIC_EINVAL, "too many shares to fold");
    return 0;
}

extern "C" int mastic_comm_unique_id(uint8_t id_out[MASTIC_COMM_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == MASTIC_COMM_ID_BYTES, "ncclUniqueId size");
    if (!id_out) return MASTIC_EINVAL;
    if (!rccl().ok) return MASTIC_ENODEV;
    ncclUniqueId id;
    if (rccl().GetUniqueId(&id) != ncclSuccess) return MASTIC_EHIP;
    std::memcpy(id_out, &id, sizeof(id));
    return 0;
}

extern "C" int mastic_comm_init_timeout(mastic_ctx* c, int nranks, int rank, const uint8_t id[MASTIC_COMM_ID_BYTES],
                                        int timeout_ms) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    if (!id || nranks < 1 || rank < 0 || rank >= nranks) return fail(c, MASTIC_EINVAL, "invalid communicator rank");
    if (c->cm.comm) return fail(c, MASTIC_EINVAL, "the ctx already has a communicator");
    if (!rccl().ok) return fail(c, MASTIC_ENODEV, "RCCL is not available: %s", rccl().why.c_str());
    c->cm.timeout_ms = timeout_ms > 0 ? timeout_ms : MASTIC_COMM_TIMEOUT_MS;
    // the agreement round's buffers, before joining: a rank that cannot
    // allocate them fails here, before any collective
    const size_t st_bytes = sizeof(CommStatus) * ((size_t)nranks + 1);
    if (!c->cm.st.ensure(st_bytes)) return fail(c, MASTIC_ENOMEM, "out of device memory");
    if (c->cm.st_host_n < (size_t)nranks + 1) {
        if (c->cm.st_host) (void)hipHostFree(c->cm.st_host);
        c->cm.st_host = nullptr;
        c->cm.st_host_n = 0;
        HIPCHK(c, hipHostMalloc(&c->cm.st_host, st_bytes, hipHostMallocDefault));
        c->cm.st_host_n = (size_t)nranks + 1;
    }
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    // RCCL's init blocks until every rank has joined -- in its bootstrap,
    // even for a communicator configured non-blocking (measured on RCCL
    // 2.27.7: ncclCommInitRankConfig with blocking = 0 did not return while
    // a peer was missing) -- so it runs on a thread of its own and this call
    // waits for it with the ctx's bound.  An init the caller gave up on stays
    // with its thread, which releases the communicator (ncclCommAbort) if the
    // peers ever arrive; the ctx stays world 1.
    auto job = std::make_shared<CommInitJob>();
    const int dev = c->device;
    try {
        std::thread([job, nranks, uid, rank, dev] {
            ncclComm_t comm = nullptr;
            ncclResult_t r = ncclSystemError;
            const hipError_t e = hipSetDevice(dev);
            if (e == hipSuccess) r = rccl().CommInitRank(&comm, nranks, uid, rank);
            std::unique_lock<std::mutex> lk(job->mu);
            job->comm = comm;
            job->r = r;
            job->dev_err = e;
            job->done = true;
            const bool given_up = job->abandoned;
            lk.unlock();
            job->cv.notify_all();
            if (given_up && comm) (void)rccl().CommAbort(comm);
        }).detach();
    } catch (const std::system_error&) {
        return fail(c, MASTIC_EHIP, "cannot start the RCCL init thread");
    }
    std::unique_lock<std::mutex> lk(job->mu);
    if (!job->cv.wait_for(lk, std::chrono::milliseconds(c->cm.timeout_ms), [&] { return job->done; })) {
        job->abandoned = true;
        if (trace_comm()) fprintf(stderr, "[mastic comm] init of rank %d of %d timed out\n", rank, nranks);
        return fail(c, MASTIC_ETIMEDOUT,
                    "RCCL init: not every rank joined within %d ms (the pending init is abandoned; the ctx stays "
                    "world 1)", c->cm.timeout_ms);
    }
    if (trace_comm()) fprintf(stderr, "[mastic comm] ncclCommInitRank(%d of %d) -> %d\n", rank, nranks, (int)job->r);
    if (job->dev_err != hipSuccess) return fail(c, MASTIC_EHIP, "hipSetDevice: %s", hipGetErrorString(job->dev_err));
    if (job->r != ncclSuccess) {
        if (job->comm) (void)rccl().CommAbort(job->comm);
        return fail(c, MASTIC_EHIP, "RCCL init: %s", rccl().GetErrorString(job->r));
    }
    c->cm.comm = job->comm;
    c->cm.n = nranks;
    c->cm.rank = rank;
    c->cm.broken = false;
    return 0;
}

extern "C" int mastic_comm_init(mastic_ctx* c, int nranks, int rank, const uint8_t id[MASTIC_COMM_ID_BYTES]) {
    return mastic_comm_init_timeout(c, nranks, rank, id, MASTIC_COMM_TIMEOUT_MS);
}

extern "C" int mastic_comm_info(const mastic_ctx* c, int* nranks, int* rank) {
    if (!c) return MASTIC_EINVAL;
    if (nranks) *nranks = c->cm.n;
    if (rank) *rank = c->cm.rank;
    return 0;
}

extern "C" int mastic_comm_destroy(mastic_ctx* c) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    int rc = 0;
    if (c->cm.comm) {
        rc = comm_wait(c, "mastic_comm_destroy");
        if (!rc) rc = comm_settle(c, rccl().CommFinalize(c->cm.comm), "finalize");
        if (!rc) {
            const ncclResult_t r = rccl().CommDestroy(c->cm.comm);
            if (r != ncclSuccess) rc = fail(c, MASTIC_EHIP, "RCCL destroy: %s", rccl().GetErrorString(r));
        }
    }
    c->cm.comm = nullptr;
    c->cm.n = 1;
    c->cm.rank = 0;
    c->cm.broken = false;
    return rc;
}

extern "C" int mastic_allgather_fold(mastic_ctx* c, const void* dev_local, size_t n_local, size_t n_elems,
                                     void* dev_out, void* caller_stream) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    int rc = 0;
    if (n_elems && (!dev_out || (n_local && !dev_local))) rc = fail(c, MASTIC_EINVAL, "null share buffer");
    if (!rc) rc = comm_check_counts(c, n_local, n_elems);
    if (!rc && n_elems && !comm_stage_gather(c, n_local, n_elems)) rc = fail(c, MASTIC_ENOMEM, "out of device memory");
    if (!rc && n_elems) {
        if (!c->fold_ev && hipEventCreateWithFlags(&c->fold_ev, hipEventDisableTiming) != hipSuccess)
            rc = fail(c, MASTIC_EHIP, "hipEventCreateWithFlags failed");
        if (!rc && (hipEventRecord(c->fold_ev, (hipStream_t)caller_stream) != hipSuccess ||
                    hipStreamWaitEvent(c->stream, c->fold_ev, 0) != hipSuccess))
            rc = fail(c, MASTIC_EHIP, "ordering after the caller's stream failed");
    }
    rc = comm_agree(c, rc, COMM_ALLGATHER_FOLD, n_local, n_elems);
    if (rc || n_elems == 0) return rc;
    rc = allgather_fold_impl(c, (const uint32_t*)dev_local, n_local, n_elems, (uint32_t*)dev_out);
    if (rc) return rc;
    return comm_finish(c, COMM_ALLGATHER_FOLD);
}

extern "C" int mastic_merge_host(mastic_ctx* c, const uint8_t* host_local, size_t n_local, size_t n_elems,
                                 uint8_t* host_out) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    const size_t ebytes = (size_t)c->p.w32 * 4;
    int rc = 0;
    if (n_elems && (!host_out || (n_local && !host_local))) rc = fail(c, MASTIC_EINVAL, "null share buffer");
    if (!rc) rc = comm_check_counts(c, n_local, n_elems);
    if (!rc && n_elems &&
        (!comm_grow(c, c->cm.local, std::max<size_t>(n_local, 1) * n_elems * ebytes) ||
         !comm_grow(c, c->cm.out, n_elems * ebytes) || !comm_stage_gather(c, n_local, n_elems)))
        rc = fail(c, MASTIC_ENOMEM, "out of device memory");
    if (!rc && n_elems && n_local &&
        hipMemcpyAsync(c->cm.local.p, host_local, n_local * n_elems * ebytes, hipMemcpyHostToDevice, c->stream) !=
            hipSuccess)
        rc = fail(c, MASTIC_EHIP, "share upload failed");
    rc = comm_agree(c, rc, COMM_MERGE_HOST, n_local, n_elems);
    if (rc || n_elems == 0) return rc;
    rc = allgather_fold_impl(c, c->cm.local.as<uint32_t>(), n_local, n_elems, c->cm.out.as<uint32_t>());
    if (!rc) rc = comm_finish(c, COMM_MERGE_HOST);
    if (rc) return rc;
    return comm_copy_out(c, host_out, n_elems * ebytes);
}

extern "C" int mastic_aggregate_merged(mastic_ctx* c, uint32_t agg_mask, const uint8_t* valid, size_t n_elems,
                                       uint8_t* agg_out) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    const bool zeros = (agg_mask & MASTIC_MERGE_ZEROS) != 0;
    agg_mask &= ~MASTIC_MERGE_ZEROS;
    const size_t ebytes = (size_t)c->p.w32 * 4;
    const size_t n_local = (agg_mask & 1) + ((agg_mask >> 1) & 1);
    int rc = 0;
    if (agg_mask == 0 || agg_mask > 3) rc = fail(c, MASTIC_EINVAL, "invalid aggregator mask");
    if (!rc && n_elems && !agg_out) rc = fail(c, MASTIC_EINVAL, "null agg share buffer");
    if (!rc) rc = comm_check_counts(c, n_local, n_elems);
    for (int a = 0; a < 2 && !rc && n_elems && !zeros; a++) {
        if (!((agg_mask >> a) & 1)) continue;
        const Result& R = c->res[a];
        if (!R.ready)
            rc = fail(c, MASTIC_EINVAL, "no prep_init result for this aggregator");
        else if (agg_rows(c->p, R) != n_elems)
            rc = fail(c, MASTIC_EINVAL, "agg share length does not match the last prep_init");
    }
    if (!rc && n_elems &&
        (!comm_grow(c, c->cm.local, n_local * n_elems * ebytes) || !comm_grow(c, c->cm.out, n_elems * ebytes) ||
         !comm_stage_gather(c, n_local, n_elems)))
        rc = fail(c, MASTIC_ENOMEM, "out of device memory");
    size_t k = 0;
    for (int a = 0; a < 2 && !rc && n_elems; a++) {
        if (!((agg_mask >> a) & 1)) continue;
        uint32_t* dst = (uint32_t*)((uint8_t*)c->cm.local.p + k++ * n_elems * ebytes);
        if (!zeros)
            rc = aggregate_impl(c, a, valid, dst);
        else if (hipMemsetAsync(dst, 0, n_elems * ebytes, c->stream) != hipSuccess)  // no reports here: agg_init's zeros
            rc = fail(c, MASTIC_EHIP, "hipMemsetAsync failed");
    }
    rc = comm_agree(c, rc, COMM_AGGREGATE_MERGED, n_local, n_elems);
    if (rc || n_elems == 0) return rc;
    rc = allgather_fold_impl(c, c->cm.local.as<uint32_t>(), n_local, n_elems, c->cm.out.as<uint32_t>());
    if (!rc) rc = comm_finish(c, COMM_AGGREGATE_MERGED);
    if (rc) return rc;
    return comm_copy_out(c, agg_out, n_elems * ebytes);
}
