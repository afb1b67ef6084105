// The state every subsystem shares (mastic_hip.hip includes this first): buffers, results, the frontier
// cache, resident batches, mastic_ctx, and the helpers more than one subsystem launches or checks through.
#pragma once
namespace {

static bool env_is_1(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '1';
}
// MASTIC_TRACE_ALLOC=1: log every device allocation / free with its duration (stderr)
static bool trace_alloc() {
    static const bool on = env_is_1("MASTIC_TRACE_ALLOC");
    return on;
}
// MASTIC_TRACE_COMM=1: log the communicator's init / agreement / abort steps (stderr)
static bool trace_comm() {
    static const bool on = env_is_1("MASTIC_TRACE_COMM");
    return on;
}
static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool own = true;  // false: a view into another buffer (mastic_reports_view)
    ~DevBuf() { release(); }
    void release() {
        if (p && own) {
            const double t0 = trace_alloc() ? now_ms() : 0;
            (void)hipFree(p);
            if (trace_alloc()) fprintf(stderr, "[mastic] free %.3f GB %.1f ms\n", bytes / 1e9, now_ms() - t0);
        }
        p = nullptr;
        bytes = 0;
        own = true;
    }
    void swap(DevBuf& o) { std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(own, o.own); }
    void view(const DevBuf& b, size_t off, size_t len) {
        release();
        if (!b.p) return;
        p = (uint8_t*)b.p + off;
        bytes = len;
        own = false;
    }
    bool ensure(size_t want) {
        if (want <= bytes && p) return true;
        release();
        if (want == 0) want = 16;
        const double t0 = trace_alloc() ? now_ms() : 0;
        const hipError_t e = hipMalloc(&p, want);
        if (trace_alloc()) fprintf(stderr, "[mastic] malloc %.3f GB %.1f ms%s\n", want / 1e9, now_ms() - t0,
                                   e == hipSuccess ? "" : " FAILED");
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();  // callers handle it; keep it out of later launch checks
            return false;
        }
        bytes = want;
        return true;
    }
    // ensure() with headroom: buffers that follow a growing size (results,
    // staging) are re-allocated rarely (a large hipMalloc costs ~1 s per
    // 50 GB on MI355X)
    bool grow(size_t want) {
        if (want <= bytes && p) return true;
        return ensure(std::max(want, bytes + bytes / 2)) || ensure(want);
    }
    template <class T> T* as() const { return (T*)p; }
};

// The decoded agg param's tree (host_tree.hpp) plus its device copy.
// The device arrays live in one allocation (dev): child_exp, child_pfx,
// child_path, parent_node.
struct Tree : TreeShape {
    DevBuf dev;
    int32_t* d_exp = nullptr;
    int32_t* d_pfx = nullptr;
    uint32_t* d_path = nullptr;
    int32_t* d_parent = nullptr;
};

struct Result {
    bool ready = false;
    size_t n = 0, stride = 0;
    int weight_check = 0;
    int n_prefixes = 0;
    DevBuf out, eval_proof, verifier, jr_part, jr_seed, status;
};

// Frontier cache of one aggregator (mastic_set_frontier_cache; SURVEY.md §8f
// row 1).  In a level sweep (examples.py:37-91) prep_init at level L evaluates
// the whole tree again, but its levels 0..L-1 are usually exactly the previous
// call's tree.  The cache keeps, per report, the two binder sponges' states
// after the cached call's levels (the binder messages are BFS-ordered, so the
// cached message is a prefix of the next one), every node of the last level as
// its convert seed and control bit (5 words: a hit recomputes a parent's seed
// and payload from its convert stream) or, where the call that wrote the slot
// chose the payloads format (mastic_set_frontier_cache_nodes, memplan.hpp
// choose_node_words), as its next seed, control bit and corrected payload
// (5 + VALUE_LEN * w32 words: a hit recomputes nothing), and the root sum; a
// call whose tree extends the cached one by one level evaluates and absorbs
// only that level.
// Planes of all n reports (stride S, independent of the HBM-budget chunks a
// call runs in, so a sweep's chunking may change from level to level).  The
// last level kernel writes its children straight into a spare node slot
// shared by the ctx's aggregators (mastic_ctx::fc_spare; a hit reads its
// parents from this aggregator's slot meanwhile), and the call then swaps the
// two: three node slots in all, no copy of the level into the cache.
// The host metadata (what was cached, the hit test) is memplan.hpp FrontierMeta.

// One node slot: a level's nodes [node][node_words] as planes of stride S.
// Giving it up while queued kernels may still read it is mastic_ctx::retire.
struct NodeSlot {
    DevBuf buf;
    size_t words = 0;  // words per plane row it can hold (nodes x words per node, either format)
    size_t S = 0;      // its plane stride
    bool holds(size_t nodes, size_t node_words) const { return slot_holds(words, nodes, node_words); }
    void swap(NodeSlot& o) { buf.swap(o.buf); std::swap(words, o.words); std::swap(S, o.S); }
    void release() { buf.release(); words = S = 0; }
};

struct LevelCache : FrontierMeta {
    DevBuf sp, rootsum;  // both binder sponges (2 x 50 planes); root sum (wl planes)
    NodeSlot nd;         // last level's nodes (FrontierMeta: the format of the call that wrote them); nd.S == S
    void release() {
        drop();
        sp.release();
        rootsum.release();
        nd.release();
        S = 0;
    }
};

// The staging buffers of the folds (fold.hpp).
struct FoldStage {
    DevBuf valid, out;                  // mastic_aggregate: the validity mask, the agg share
    DevBuf part;                        // per-chunk partial sums of a split fold (aggregate_impl)
    DevBuf grp_ids, grp_part, grp_out;  // mastic_aggregate_grouped: group ids, per-chunk partials, output staging
};

// The library-owned RCCL communicator of a ctx and its staging (comm.hpp; none = world 1).
struct CommState {
    ncclComm_t comm = nullptr;
    int n = 1, rank = 0;
    bool broken = false;  // aborted after a failed / timed-out step: collective calls fail
    int timeout_ms = MASTIC_COMM_TIMEOUT_MS;  // bound of every wait on the communicator
    DevBuf local, gather, out;  // mastic_aggregate_merged / mastic_allgather_fold staging
    DevBuf st;                  // agreement round: this rank's status + every rank's
    void* st_host = nullptr;    // pinned host copy of the same (nranks + 1 records)
    size_t st_host_n = 0;
    hipEvent_t marks[3] = {};   // MASTIC_TRACE_COMM: progress marks of the agreement round
    void release(hipStream_t stream);  // ctx teardown (defined with the RCCL binding)
};

}  // namespace

// Frontier-cache key of a batch: its identity (id, unique per batch or view
// object) and the generation of the HBM it reads.  A batch and its views share
// one generation counter (`gen`), so an upload or shard through any of them
// invalidates cache entries keyed on the others.  Contexts may be driven from
// several threads, so the counters are atomic.
static std::atomic<uint64_t> g_reports_gen{0};
static uint64_t next_reports_gen() { return g_reports_gen.fetch_add(1) + 1; }
struct mastic_reports {
    mastic_ctx* ctx = nullptr;
    size_t n = 0;
    uint64_t id = next_reports_gen();
    std::shared_ptr<std::atomic<uint64_t>> gen = std::make_shared<std::atomic<uint64_t>>(next_reports_gen());
    DevBuf nonces, pub, in0, in1;
    DevBuf wire_flags;  // [n] WIRE_BAD_* of k_validate_wire, refreshed by every upload / shard
    void touch() { gen->store(next_reports_gen()); }
    uint64_t generation() const { return gen->load(); }
};

struct mastic_ctx {
    mastic_params user{};
    McParams p{};
    int device = 0;
    hipStream_t stream = nullptr;   // level evals, setup, finalize, FLP
    hipStream_t stream2 = nullptr;  // binder sponges (overlap the next level's eval)
    hipStream_t stream3 = nullptr;  // binder sponges of the odd chunks of a pipelined prep_init
    hipStream_t stream4 = nullptr;  // FLP randomness + query of a weight-check call, beside its last sponges
    std::vector<hipEvent_t> sync_ev;
    hipEvent_t fold_ev = nullptr;  // order_after: caller's stream -> stream
    CommState cm;
    PrefixState pfx_host[PFX_COUNT];
    std::string err;
    MemKnobs m;      // the knobs the memory plan reads (memplan.hpp)
    DevBuf work;     // per-chunk planes
    DevBuf pfx;      // PrefixState[PFX_COUNT]
    DevBuf pfx_bytes, pfx_meta;
    DevBuf consts;   // alpha^-i table for prove
    FoldStage fold;
    DevBuf stage;              // result encoding / decide staging
    SchedKnobs k;               // the knobs the launch plan reads (schedule.hpp)
    ChunkPlan plans[2];         // the last prep_init's plans (full chunk, last chunk): their vectors are reused
    // the running chunk's sponge ends: per planned sponge launch, and the last
    // piece of the one-hot / payload sponge of each level (run_plan)
    std::vector<hipEvent_t> sp_done, oh_done, pl_done;
    // result-preserving test hooks (mastic_set_test_hooks; nothing in the environment sets them)
    int force_slow_blk = -1;    // exact payload stream from this block on
    int fail_allocs = 0;        // this many result / cache-slot allocations fail first (ENOMEM recovery)
    int sponge_delay_us = 0;    // the next prep_init first holds the sponge stream this long (k_spin)
    int wall_khz = 100000;      // wall_clock64() rate (hipDeviceAttributeWallClockRate)
    bool serial_sponges = false;  // measurement: sponge launches run alone (mastic_set_serial_sponges)
    bool inject_alloc_failure() {
        if (fail_allocs <= 0) return false;
        fail_allocs--;
        return true;
    }
    // Wait for everything queued on the ctx's four streams (explicitly: the
    // recovery paths below free buffers that queued kernels on any of them may
    // still read, so they must not rely on hipFree's implicit device wait).
    // Every stream is waited for, also after a wait failed (mastic_ctx_destroy frees everything next).
    bool idle() {
        bool ok = true;
        for (hipStream_t s : {stream, stream2, stream3, stream4}) ok = hipStreamSynchronize(s) == hipSuccess && ok;
        return ok;
    }
    int pfx_f[PFX_COUNT] = {0};  // fill position of each prefix state (host copy)
    std::vector<uint8_t> pfx_key;  // verify key || ctx of the prefix states in pfx (empty: none)
    std::map<std::vector<uint8_t>, Tree*> trees;
    Result res[2];
    bool frontier_cache = false;  // mastic_set_frontier_cache
    bool last_hit = false;        // the last prep_init evaluated only its last level
    LevelCache lc[2];
    NodeSlot fc_spare;        // the frontier cache's spare node slot
    int fc_nodes = FC_NODES_SEEDS;         // the node format cache-on calls write (mastic_set_frontier_cache_nodes)
    int last_nodes_in = -1, last_nodes_out = -1;  // the last prep_init: format its hit read / it wrote (-1: none)
    std::vector<void*> graveyard;  // replaced cache slots, freed once the streams are idle
    // The AES key schedules in the work arena (k_setup): the reports, ctx and
    // plane geometry they were derived for, so a frontier-cache hit over the
    // same batch skips k_setup (the fixed keys depend on the nonce and ctx only,
    // not on the aggregator or level).  Cleared by anything else that writes
    // the arena's header (a chunked call, the shard's scratch).
    struct {
        bool valid = false;
        uint64_t rep_id = 0, rep_gen = 0;
        size_t n = 0;
        int stride = 0;
        const void* W = nullptr;
        std::vector<uint8_t> pfx_key;
    } rk;
    // pinned staging of the tree uploads (build_tree): one async copy per new
    // tree on the main stream; tree_ev marks when the staging may be reused
    void* tree_stage = nullptr;
    size_t tree_stage_bytes = 0;
    hipEvent_t tree_ev = nullptr;
    void bury() {
        for (void* q : graveyard) (void)hipFree(q);
        graveyard.clear();
    }
    // Give up a buffer that queued kernels may still read: it is freed at the
    // next idle point of the streams (bury), not here, where hipFree would
    // wait for the whole device, i.e. for the other aggregator's queued call.
    void retire(DevBuf& b) {
        if (b.p && b.own) graveyard.push_back(b.p);
        b.p = nullptr;
        b.bytes = 0;
    }
    // The same for a node slot, which is left empty, for planes of stride S.
    void retire(NodeSlot& s, size_t S = 0) { retire(s.buf); s.words = 0; s.S = S; }
    // How reclaim_ensure recovers (memory plan: which differences are deliberate).
    struct Reclaim {
        bool inject;       // the attempt consumes fail_allocs (the test hook covers results and cache slots)
        bool arena;        // the recovery also releases the work arena, and with it the key schedules (rk)
        bool retry_first;  // the retry tries `first` again before `want`
        bool if_buried;    // recover only if the graveyard holds something to free
    };
    // Allocate b: `first` bytes (0: none), else `want`.  If that fails, wait
    // for the streams, free the retired buffers (and what `how` adds), and
    // try once more.
    bool reclaim_ensure(DevBuf& b, size_t first, size_t want, const Reclaim& how) {
        auto attempt = [&](bool with_first) { return (with_first && b.ensure(first)) || b.ensure(want); };
        if (!(how.inject && inject_alloc_failure()) && attempt(first != 0)) return true;
        if ((how.if_buried && graveyard.empty()) || !idle()) return false;
        bury();
        if (how.arena) {
            work.release();
            rk.valid = false;
        }
        return attempt(first != 0 && how.retry_first);
    }
    // timing
    // timing events and results of the last prep_init of each aggregator
    // (both may be queued before either's results are fetched)
    struct Timing {
        std::vector<hipEvent_t> ev;
        double t_eval = 0, t_proof = 0, t_absorb = 0, t_total = 0;
        int n_eval = 0, n_absorb = 0;
    } tm[2];
    int tcur = 0;  // aggregator whose timing mastic_last_timing* report (last prep_init / prep_result)
    ~mastic_ctx() {
        bury();
        for (auto& kv : trees) delete kv.second;
        for (auto& x : tm)
            for (auto e : x.ev) (void)hipEventDestroy(e);
        for (auto e : sync_ev) (void)hipEventDestroy(e);
        if (fold_ev) (void)hipEventDestroy(fold_ev);
        cm.release(stream);
        if (tree_ev) (void)hipEventDestroy(tree_ev);
        if (tree_stage) (void)hipHostFree(tree_stage);
        if (stream) (void)hipStreamDestroy(stream);
        if (stream2) (void)hipStreamDestroy(stream2);
        if (stream3) (void)hipStreamDestroy(stream3);
        if (stream4) (void)hipStreamDestroy(stream4);
    }
};

// Every entry point that touches the GPU runs with the ctx's device current
// (and restores the caller's), so contexts on different GPUs can be driven
// from one thread.
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(const mastic_ctx* c) {
        int cur = -1;
        if (c && hipGetDevice(&cur) == hipSuccess && cur != c->device && hipSetDevice(c->device) == hipSuccess) prev = cur;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

static int fail(mastic_ctx* c, int code, const char* fmt, ...) {
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

#define HIPCHK(c, expr)                                                                  \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess) return fail((c), MASTIC_EHIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

// ---------------------------------------------------------------- shared helpers
// fn(FieldTag<F>{}) with the field of p:
//   with_field(p, [&](auto f) { using F = typename decltype(f)::type; ... });
template <class F> struct FieldTag { typedef F type; };
template <class Fn>
static auto with_field(const McParams& p, Fn&& fn) {
    return p.field == 64 ? fn(FieldTag<F64>{}) : fn(FieldTag<F128>{});
}

// Rows of an agg share of result slot R: one counter and output_len elements per candidate prefix.
static size_t agg_rows(const McParams& p, const Result& R) { return (size_t)R.n_prefixes * (1 + p.output_len); }

// The last prep_init result of agg_id, or null with the ctx's error set (MASTIC_EINVAL).
static Result* ready_result(mastic_ctx* c, int agg_id) {
    if (!c || (agg_id != 0 && agg_id != 1)) return fail(c, MASTIC_EINVAL, "invalid aggregator ID"), nullptr;
    if (!c->res[agg_id].ready) return fail(c, MASTIC_EINVAL, "no prep_init result for this aggregator"), nullptr;
    return &c->res[agg_id];
}

// Order c->stream after the work queued on the caller's stream so far (what allocated, filled or
// all-gathered a buffer the next kernel touches): an event, no device-wide sync.
static int order_after(mastic_ctx* c, void* caller_stream) {
    if (!c->fold_ev) HIPCHK(c, hipEventCreateWithFlags(&c->fold_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->fold_ev, (hipStream_t)caller_stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->fold_ev, 0));
    return 0;
}

// out = sum mod p of n_shares shares of n_elems elements each (k_fold_shares), on c->stream.
static int launch_fold_shares(mastic_ctx* c, const uint32_t* src, size_t n_shares, size_t n_elems, uint32_t* out) {
    with_field(c->p, [&](auto f) {
        using F = typename decltype(f)::type;
        hipLaunchKernelGGL(k_fold_shares<F>, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, c->stream, src,
                           (int)n_shares, (int)n_elems, out);
    });
    HIPCHK(c, hipGetLastError());
    return 0;
}

// k_decide over n pairs of prep-share wire rows (psz bytes each), on c->stream; ver: FLP scratch planes.
static int launch_decide(mastic_ctx* c, size_t n, size_t stride, int weight_check, const uint8_t* ps0,
                         const uint8_t* ps1, size_t psz, uint32_t* ver, uint8_t* msg, uint8_t* code) {
    with_field(c->p, [&](auto f) {
        using F = typename decltype(f)::type;
        hipLaunchKernelGGL(k_decide<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->p, (int)n,
                           (int)stride, weight_check, ps0, ps1, (int)psz, ver, (const PrefixState*)c->pfx.p, msg, code);
    });
    HIPCHK(c, hipGetLastError());
    return 0;
}
