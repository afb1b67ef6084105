// Host side of the MI355X Mastic aggregator: C ABI (include/mastic_hip.h),
// agg-param decoding and tree building, HBM buffer management and the
// level-by-level launch schedule.  No CPU compute path exists: every
// cryptographic operation of prep_init / shard / decide / aggregate runs in
// the kernels of kernels.hpp / shard.hpp.
#include "mastic_hip.h"

#include <dlfcn.h>
#include <rccl/rccl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <type_traits>
#include <vector>

#include "comm_agree.hpp"
#include "compact_plan.hpp"
#include "host_tree.hpp"
#include "kernels.hpp"
#include "memplan.hpp"
#include "nonce_set_kernels.hpp"
#include "rows_kernels.hpp"
#include "schedule.hpp"
#include "shard.hpp"

static_assert(SCHED_EVAL_WAVES == EVAL_WAVES && SCHED_EVAL_PROOF_WAVES == EVAL_PROOF_WAVES &&
                  SCHED_SPONGE_RATE == KECCAK_RATE,
              "schedule.hpp and the kernels disagree on a shared constant");

namespace {

// MASTIC_TRACE_ALLOC=1: log every device allocation / free with its duration (stderr)
static bool trace_alloc() {
    static const bool on = [] {
        const char* e = getenv("MASTIC_TRACE_ALLOC");
        return e && e[0] == '1';
    }();
    return on;
}
// MASTIC_TRACE_COMM=1: log the communicator's init / agreement / abort steps (stderr)
static bool trace_comm() {
    static const bool on = [] {
        const char* e = getenv("MASTIC_TRACE_COMM");
        return e && e[0] == '1';
    }();
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
struct LevelCache : FrontierMeta {
    DevBuf sp, rootsum;    // both binder sponges (2 x 50 planes); root sum (wl planes)
    DevBuf nd;             // last level's nodes [node][node_words] (FrontierMeta: the format of the call that wrote them)
    size_t nd_words = 0;   // words per plane row nd can hold (nodes x words per node, either format)
    void release() {
        drop();
        sp.release();
        rootsum.release();
        nd.release();
        nd_words = 0;
        S = 0;
    }
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
    hipEvent_t fold_ev = nullptr;  // mastic_fold_shares: producer stream -> stream
    hipEvent_t comm_marks[3] = {};  // MASTIC_TRACE_COMM: progress marks of the agreement round
    // library-owned RCCL communicator (mastic_comm_init; none = world 1)
    ncclComm_t comm = nullptr;
    int comm_n = 1, comm_rank = 0;
    bool comm_broken = false;  // aborted after a failed / timed-out step: collective calls fail
    int comm_timeout_ms = MASTIC_COMM_TIMEOUT_MS;  // bound of every wait on the communicator
    DevBuf comm_local, comm_gather, comm_out;  // mastic_aggregate_merged / mastic_allgather_fold staging
    DevBuf comm_st;                            // agreement round: this rank's status + every rank's
    void* comm_st_host = nullptr;              // pinned host copy of the same (nranks + 1 records)
    size_t comm_st_host_n = 0;
    void comm_release();                       // teardown of a live communicator (defined with the RCCL binding)
    PrefixState pfx_host[PFX_COUNT];
    std::string err;
    MemKnobs m;      // the knobs the memory plan reads (memplan.hpp)
    DevBuf work;     // per-chunk planes
    DevBuf pfx;      // PrefixState[PFX_COUNT]
    DevBuf pfx_bytes, pfx_meta;
    DevBuf consts;   // alpha^-i table for prove
    DevBuf agg_valid, agg_out;  // mastic_aggregate staging
    DevBuf agg_part;            // per-chunk partial sums of a split fold (aggregate_impl)
    DevBuf grp_ids, grp_part, grp_out;  // mastic_aggregate_grouped: group ids, per-chunk partials, output staging
    DevBuf stage;               // result encoding / decide staging
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
    // Wait for everything queued on the ctx's three streams (explicitly: the
    // recovery paths below free buffers that queued kernels on any of them may
    // still read, so they must not rely on hipFree's implicit device wait).
    bool idle() {
        return hipStreamSynchronize(stream) == hipSuccess && hipStreamSynchronize(stream2) == hipSuccess &&
               hipStreamSynchronize(stream3) == hipSuccess && hipStreamSynchronize(stream4) == hipSuccess;
    }
    int pfx_f[PFX_COUNT] = {0};  // fill position of each prefix state (host copy)
    std::vector<uint8_t> pfx_key;  // verify key || ctx of the prefix states in pfx (empty: none)
    std::map<std::vector<uint8_t>, Tree*> trees;
    Result res[2];
    bool frontier_cache = false;  // mastic_set_frontier_cache
    bool last_hit = false;        // the last prep_init evaluated only its last level
    LevelCache lc[2];
    DevBuf fc_spare;          // the frontier cache's spare node slot (LevelCache::nd layout)
    size_t spare_words = 0;   // words per plane row it can hold
    int fc_nodes = FC_NODES_SEEDS;         // the node format cache-on calls write (mastic_set_frontier_cache_nodes)
    int last_nodes_in = -1, last_nodes_out = -1;  // the last prep_init: format its hit read / it wrote (-1: none)
    size_t spare_S = 0;       // its plane stride
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
        for (hipEvent_t e : comm_marks)
            if (e) (void)hipEventDestroy(e);
        if (comm) comm_release();
        if (comm_st_host) (void)hipHostFree(comm_st_host);
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
    explicit DeviceScope(const mastic_ctx* c);
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};
DeviceScope::DeviceScope(const mastic_ctx* c) {
    int cur = -1;
    if (c && hipGetDevice(&cur) == hipSuccess && cur != c->device && hipSetDevice(c->device) == hipSuccess) prev = cur;
}

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

// ---------------------------------------------------------------- helpers
static void put_le16(std::vector<uint8_t>& v, uint32_t x) {
    v.push_back((uint8_t)x);
    v.push_back((uint8_t)(x >> 8));
}

// dst (poc/dst.py:30-32) and dst_alg (:35-42)
static std::vector<uint8_t> dst(const uint8_t* ctx, size_t n, int usage) {
    std::vector<uint8_t> d = {'m', 'a', 's', 't', 'i', 'c', 0, (uint8_t)usage};
    d.insert(d.end(), ctx, ctx + n);
    return d;
}
static std::vector<uint8_t> dst_alg(const uint8_t* ctx, size_t n, int usage, uint32_t id) {
    std::vector<uint8_t> d = {'m', 'a', 's', 't', 'i', 'c', 0, (uint8_t)usage,
                              (uint8_t)(id >> 24), (uint8_t)(id >> 16), (uint8_t)(id >> 8), (uint8_t)id};
    d.insert(d.end(), ctx, ctx + n);
    return d;
}

// Compute the sponge prefix states for (ctx, verify_key) on the device.  The
// verify key is XofTurboShake128's seed (u8 length prefix, mastic.py:302-306,
// 499-510), so any length up to 255 bytes is accepted (the reference's own
// driver uses 16, examples.py:38,176; VERIFY_KEY_SIZE is 32, mastic.py:73).
static int build_prefixes(mastic_ctx* c, const uint8_t* app_ctx, size_t ctx_len, const uint8_t* vk, size_t vk_len) {
    if (ctx_len > 65535 - 12) return fail(c, MASTIC_EINVAL, "ctx too long");
    if (vk && vk_len > 255) return fail(c, MASTIC_EINVAL, "verify key too long");
    // callers without a verify key (decide, shard, proof tree) never read the
    // two verify-key states (PFX_EVAL, PFX_QUERY: prep_init only), so any
    // states of the same ctx serve them.  Key layout: u8(len) || vk || ctx || 1.
    if (!vk && !c->pfx_key.empty()) {
        const size_t kl = c->pfx_key[0];
        if (c->pfx_key.size() == 1 + kl + ctx_len + 1 &&
            (ctx_len == 0 || std::equal(app_ctx, app_ctx + ctx_len, c->pfx_key.begin() + 1 + kl)))
            return 0;
    }
    static const uint8_t zero_vk[32] = {0};
    if (!vk) {
        vk = zero_vk;
        vk_len = 32;
    }
    std::vector<uint8_t> key(1, (uint8_t)vk_len);
    key.insert(key.end(), vk, vk + vk_len);
    key.insert(key.end(), app_ctx, app_ctx + ctx_len);
    key.push_back(1);  // never equal to the empty "none" key
    if (key == c->pfx_key) return 0;  // same verify key and ctx as the states already in pfx
    c->pfx_key.clear();
    std::vector<std::vector<uint8_t>> m(PFX_COUNT);
    auto xof_ts = [&](int id, const std::vector<uint8_t>& d, int seed_len, const uint8_t* seed) {
        put_le16(m[id], (uint32_t)d.size());
        m[id].insert(m[id].end(), d.begin(), d.end());
        m[id].push_back((uint8_t)seed_len);
        if (seed) m[id].insert(m[id].end(), seed, seed + seed_len);
    };
    auto xof_aes = [&](int id, const std::vector<uint8_t>& d) {
        put_le16(m[id], (uint32_t)d.size());
        m[id].insert(m[id].end(), d.begin(), d.end());
    };
    const uint32_t ID = c->p.alg_id;
    xof_aes(PFX_EXT, dst(app_ctx, ctx_len, 10));
    xof_aes(PFX_CONV, dst(app_ctx, ctx_len, 11));
    xof_ts(PFX_NODE, dst(app_ctx, ctx_len, 9), 16, nullptr);
    xof_ts(PFX_ONEHOT, dst_alg(app_ctx, ctx_len, 6, ID), 0, nullptr);
    xof_ts(PFX_PAYLOAD, dst_alg(app_ctx, ctx_len, 7, ID), 0, nullptr);
    xof_ts(PFX_EVAL, dst_alg(app_ctx, ctx_len, 8, ID), (int)vk_len, vk);
    xof_ts(PFX_QUERY, dst_alg(app_ctx, ctx_len, 2, ID), (int)vk_len, vk);
    xof_ts(PFX_PROOF_SHARE, dst_alg(app_ctx, ctx_len, 1, ID), 32, nullptr);
    xof_ts(PFX_JR_PART, dst_alg(app_ctx, ctx_len, 4, ID), 32, nullptr);
    xof_ts(PFX_JR_SEED, dst_alg(app_ctx, ctx_len, 3, ID), 0, nullptr);
    xof_ts(PFX_JR, dst_alg(app_ctx, ctx_len, 5, ID), 32, nullptr);
    xof_ts(PFX_PROVE_RAND, dst_alg(app_ctx, ctx_len, 0, ID), 32, nullptr);
    xof_ts(PFX_TREE, dst(app_ctx, ctx_len, 12), 0, nullptr);
    std::vector<uint8_t> all;
    std::vector<int> meta(2 * PFX_COUNT);
    for (int i = 0; i < PFX_COUNT; i++) {
        c->pfx_f[i] = (int)(m[i].size() % KECCAK_RATE);
        meta[i] = (int)all.size();
        meta[PFX_COUNT + i] = (int)m[i].size();
        all.insert(all.end(), m[i].begin(), m[i].end());
    }
    if (!c->pfx.ensure(sizeof(PrefixState) * PFX_COUNT) || !c->pfx_bytes.ensure(all.size()) ||
        !c->pfx_meta.ensure(meta.size() * sizeof(int)))
        return fail(c, MASTIC_ENOMEM, "out of device memory (prefix states)");
    HIPCHK(c, hipMemcpyAsync(c->pfx_bytes.p, all.data(), all.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->pfx_meta.p, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_prefix_states, dim3(1), dim3(64), 0, c->stream, c->pfx_bytes.as<uint8_t>(),
                       c->pfx_meta.as<int>(), c->pfx_meta.as<int>() + PFX_COUNT, (int)PFX_COUNT,
                       c->pfx.as<PrefixState>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->pfx_host, c->pfx.p, sizeof(PrefixState) * PFX_COUNT, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pfx_key = std::move(key);
    return 0;
}

// ---------------------------------------------------------------- tree
// Decode Mastic.encode_agg_param (mastic.py:413-435) and build the evaluated
// prefix tree of eval_with_siblings (vidpf.py:213-261): the children of every
// node on a candidate-prefix path, level by level in BFS (= lexicographic)
// order, which is the binder order of prep_init (mastic.py:263-275).
static int build_tree(mastic_ctx* c, const uint8_t* enc, size_t len, Tree** out) {
    std::vector<uint8_t> keyv(enc, enc + len);
    auto it = c->trees.find(keyv);
    if (it != c->trees.end()) {
        *out = it->second;
        return 0;
    }
    Tree* t = new Tree();
    std::string perr;
    const int prc = tree_parse(c->p.bits, enc, len, t, &perr);
    if (prc != TREE_OK) {
        delete t;
        return fail(c, prc == TREE_ENOMEM ? MASTIC_ENOMEM : MASTIC_EINVAL, "%s", perr.c_str());
    }
    const size_t total = t->nodes;
    const size_t npar = t->parent_node.size();
    // one device allocation and one upload: [child_path | child_exp | child_pfx | parent_node]
    const size_t o_exp = total * 32, o_pfx = o_exp + total * 4, o_par = o_pfx + total * 4;
    const size_t bytes = o_par + std::max<size_t>(npar, 1) * 4;
    if (!t->dev.ensure(bytes)) {
        delete t;
        return fail(c, MASTIC_ENOMEM, "out of device memory (tree)");
    }
    uint8_t* d = t->dev.as<uint8_t>();
    t->d_path = (uint32_t*)d;
    t->d_exp = (int32_t*)(d + o_exp);
    t->d_pfx = (int32_t*)(d + o_pfx);
    t->d_parent = (int32_t*)(d + o_par);
    // staged through a pinned buffer and copied on the main stream (the
    // kernels that read the tree queue behind it); the previous upload must
    // have left the staging buffer first
    bool staged = false;
    if (c->tree_ev || hipEventCreateWithFlags(&c->tree_ev, hipEventDisableTiming) == hipSuccess) {
        if (c->tree_stage_bytes && hipEventSynchronize(c->tree_ev) != hipSuccess) {
            delete t;
            return fail(c, MASTIC_EHIP, "tree upload failed");
        }
        if (c->tree_stage_bytes < bytes) {
            if (c->tree_stage) (void)hipHostFree(c->tree_stage);
            c->tree_stage = nullptr;
            c->tree_stage_bytes = 0;
            const size_t want = std::max(bytes, (size_t)4 << 20);
            if (hipHostMalloc(&c->tree_stage, want, hipHostMallocDefault) == hipSuccess)
                c->tree_stage_bytes = want;
            else
                (void)hipGetLastError();
        }
        if (c->tree_stage_bytes >= bytes) {
            uint8_t* h = (uint8_t*)c->tree_stage;
            std::memcpy(h, t->child_path.data(), total * 32);
            std::memcpy(h + o_exp, t->child_exp.data(), total * 4);
            std::memcpy(h + o_pfx, t->child_pfx.data(), total * 4);
            if (npar) std::memcpy(h + o_par, t->parent_node.data(), npar * 4);
            if (hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                hipEventRecord(c->tree_ev, c->stream) != hipSuccess) {
                delete t;
                return fail(c, MASTIC_EHIP, "tree upload failed");
            }
            staged = true;
        }
    }
    if (!staged) {  // no pinned memory: synchronous uploads from the host vectors
        hipError_t e1 = hipMemcpy(t->d_path, t->child_path.data(), total * 32, hipMemcpyHostToDevice);
        hipError_t e2 = hipMemcpy(t->d_exp, t->child_exp.data(), total * 4, hipMemcpyHostToDevice);
        hipError_t e3 = hipMemcpy(t->d_pfx, t->child_pfx.data(), total * 4, hipMemcpyHostToDevice);
        hipError_t e4 = npar ? hipMemcpy(t->d_parent, t->parent_node.data(), npar * 4, hipMemcpyHostToDevice)
                             : hipSuccess;
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess) {
            delete t;
            return fail(c, MASTIC_EHIP, "tree upload failed");
        }
    }
    if (c->trees.size() > 64) {
        // queued kernels may still read the cached trees: their device
        // buffers are retired (freed at the next idle point of the ctx's
        // streams, mastic_ctx::bury), not freed here
        for (auto& kv : c->trees) {
            c->retire(kv.second->dev);
            delete kv.second;
        }
        c->trees.clear();
    }
    c->trees[keyv] = t;
    *out = t;
    return 0;
}

// ---------------------------------------------------------------- work layout
struct WorkLayout {
    size_t words = 0;  // per report (plane count)
    size_t key, nonce, cw_seed, cw_ctrl, cw_w, cw_proof, lps, seed, peer, rk_ext, rk_conv, sp_onehot, sp_payload,
        rootsum, beta, eval_proof, proof, qr, jr, jr_part, jr_seed, verifier, status, cs[2], fr_w[2], onehot[3],
        payload[3];
};

static WorkLayout work_layout(const McParams& p, const Tree* t) {
    WorkLayout w;
    size_t o = 0;
    auto take = [&](size_t n) {
        size_t r = o;
        o += n;
        return r;
    };
    const size_t wl = (size_t)p.value_len * p.w32;
    w.key = take(4);
    w.nonce = take(4);
    w.cw_seed = take((size_t)p.bits * 4);
    w.cw_ctrl = take(p.bits);
    w.cw_w = take((size_t)p.bits * wl);
    w.cw_proof = take((size_t)p.bits * 8);
    w.lps = take((size_t)p.proof_len * p.w32);
    w.seed = take(8);
    w.peer = take(8);
    w.rk_ext = take(44);
    w.rk_conv = take(44);
    w.sp_onehot = take(50);
    w.sp_payload = take(50);
    w.rootsum = take(wl);
    w.beta = take(wl);
    w.eval_proof = take(8);
    w.proof = take((size_t)p.proof_len * p.w32);
    w.qr = take((size_t)p.query_rand_len * p.w32);
    w.jr = take((size_t)std::max(p.joint_rand_len, 1) * p.w32);
    w.jr_part = take(8);
    w.jr_seed = take(8);
    w.verifier = take((size_t)p.verifier_len * p.w32);
    w.status = take(1);
    for (int s = 0; s < 2; s++) {
        w.cs[s] = take((size_t)t->max_level_nodes * 5);
        w.fr_w[s] = take((size_t)std::max(t->max_exp, 1) * wl);
    }
    for (int k = 0; k < NSLOT; k++) {
        w.onehot[k] = take((size_t)t->max_level_nodes * 8);
        w.payload[k] = take((size_t)t->max_parents * wl);
    }
    w.words = o;
    return w;
}

static Planes make_planes(uint32_t* base, const WorkLayout& w, int n, int stride) {
    Planes pl;
    pl.n = n;
    pl.stride = stride;
    auto P = [&](size_t off) { return base + off * stride; };
    pl.key = P(w.key);
    pl.nonce = P(w.nonce);
    pl.cw_seed = P(w.cw_seed);
    pl.cw_ctrl = P(w.cw_ctrl);
    pl.cw_w = P(w.cw_w);
    pl.cw_proof = P(w.cw_proof);
    pl.lps = P(w.lps);
    pl.seed = P(w.seed);
    pl.peer = P(w.peer);
    pl.rk_ext = P(w.rk_ext);
    pl.rk_conv = P(w.rk_conv);
    pl.sp_onehot = P(w.sp_onehot);
    pl.sp_payload = P(w.sp_payload);
    pl.rootsum = P(w.rootsum);
    pl.beta = P(w.beta);
    pl.eval_proof = P(w.eval_proof);
    pl.proof = P(w.proof);
    pl.qr = P(w.qr);
    pl.jr = P(w.jr);
    pl.jr_part = P(w.jr_part);
    pl.jr_seed = P(w.jr_seed);
    pl.verifier = P(w.verifier);
    pl.status = (int32_t*)P(w.status);
    return pl;
}

// Event i of a pool that grows on demand.
static hipEvent_t event_at(std::vector<hipEvent_t>& pool, size_t i, unsigned flags) {
    while (pool.size() <= i) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, flags) != hipSuccess) return nullptr;
        pool.push_back(e);
    }
    return pool[i];
}
static hipEvent_t get_sync_event(mastic_ctx* c, size_t i) { return event_at(c->sync_ev, i, hipEventDisableTiming); }
static hipEvent_t get_event(mastic_ctx* c, size_t i) { return event_at(c->tm[c->tcur].ev, i, hipEventDefault); }

static int copy_planes(mastic_ctx* c, DevBuf& dst, size_t dst_stride, size_t dst_off, const uint32_t* src,
                       size_t src_stride, size_t n, size_t planes, hipStream_t s) {
    if (planes == 0) return 0;
    HIPCHK(c, hipMemcpy2DAsync(dst.as<uint32_t>() + dst_off, dst_stride * 4, src, src_stride * 4, n * 4, planes,
                               hipMemcpyDeviceToDevice, s));
    return 0;
}

// ---------------------------------------------------------------- prep_init
// The level kernel of each variant (kernels.hpp eval_aes_body; schedule.hpp
// LEVEL_VARIANTS lists the legal ones): the launch path and the LDS attribute
// loop of mastic_ctx_create both go through here.
typedef void (*LevelKernel)(McParams, Planes, AesArgs);
template <class F>
static LevelKernel level_kernel(int variant) {
    switch (variant) {
    case LV_GEN | LV_FC: return k_eval_aes<F, true, true>;
    case LV_FC_PAY: return k_eval_aes<F, true, true, false, true>;
    case 0: return k_eval_aes<F, false, false>;
    case LV_GEN: return k_eval_aes<F, true, false>;
    case LV_SPLIT: return k_eval_aes<F, false, false, true>;
    case LV_GEN | LV_SPLIT: return k_eval_aes<F, true, false, true>;
    case LV_WIDE: return k_eval_aes_wide<F, false>;
    case LV_WIDE | LV_GEN: return k_eval_aes_wide<F, true>;
    case LV_WIDE | LV_SPLIT: return k_eval_aes_wide<F, false, true>;
    case LV_WIDE | LV_GEN | LV_SPLIT: return k_eval_aes_wide<F, true, true>;
    }
    return nullptr;
}

// One chunk of reports [base, base + n) of a prep_init, in work area W, and
// its launch plan (schedule.hpp plan_chunk), which run() executes step by
// step.  lc: the frontier cache (or null); on a hit the parents are read from
// cin (the aggregator's node slot); the last level's nodes go to cout (the
// spare slot).  ss: the chunk's sponge stream.  tail: the stream of the
// chunk's last part (finalize, FLP, result and cache copies): the sponge
// stream when chunks are pipelined (the next chunk's evaluation, in the other
// half of the work arena, then overlaps this chunk's last sponges), else the
// main stream.  sev: next sync event of this chunk (consecutive pipelined
// chunks use disjoint ones); evi: next timing event of the call.
struct Chunk {
    mastic_ctx* c;
    mastic_reports* rep;
    const Tree* t;
    const WorkLayout& wl;
    const ChunkPlan& plan;
    int agg_id, n, stride;
    size_t base;
    uint32_t* W;
    hipStream_t ss, tail;
    LevelCache* lc;
    bool hit;
    const uint32_t* cin;
    uint32_t* cout;
    int in_nw, out_nw;  // words per node of cin / cout (CacheUse)
    size_t& evi;
    size_t sev;
    Planes pl;
    // A single-chunk call with the frontier cache keeps both binder sponges
    // and the root sum in the cache's planes (same stride): a hit resumes and
    // updates them in place, a miss fills them; no copies in or out.
    bool direct;
    // tiled level buffers (kernels.hpp AbsorbArgs): words per report group,
    // and between consecutive words of a report
    int oh_gstride, pay_gstride;
    static constexpr int bin_rstride = 64;
    int groups() const { return (n + 63) / 64; }  // report groups (rows beyond n are padding)
    int wlw() const { return c->p.value_len * c->p.w32; }
    uint32_t* plane(size_t off) const { return W + off * (size_t)stride; }
    // level binder buffers: the ring slots (with the frontier cache too: a
    // hit resumes both sponges from their cached states, so no level's
    // proofs or payload differences outlive the call)
    uint32_t* oh_buf(int lv) const { return plane(wl.onehot[lv % NSLOT]); }
    uint32_t* pay_buf(int lv) const { return plane(wl.payload[lv % NSLOT]); }
    hipStream_t stream(int role) const { return role == ST_MAIN ? c->stream : role == ST_THIRD ? c->stream3 : ss; }

    // Clears the header planes, then k_unpack and the row tiles.
    int unpack() {
        const McParams& p = c->p;
        // Every level plane (child seeds, frontier payloads, proof / payload-
        // difference ring, out shares, staged last-level payloads) is written
        // before it is read: level l reads only level l-1's nodes / expanded
        // nodes, which level l-1 wrote, and each candidate prefix is one child of
        // level L.  So only the per-report header planes (keys, correction words,
        // sponge states, FLP planes, status) are cleared -- 8 KB per report at C2
        // instead of the whole 9.7 MB work area (119 GB of fill per C2 step).  A
        // frontier-cache hit writes every header plane it reads except the
        // status plane: it clears just that.
        if (hit)
            HIPCHK(c, hipMemsetAsync(pl.status, 0, (size_t)stride * 4, c->stream));
        else {
            // Of the header, the keys, nonces and correction words (k_unpack: every
            // report row, every level the call reads) and the AES key schedules and
            // sponge states (k_setup: every row) are written in full before any
            // read, so only their padding rows are cleared; the planes between
            // (leader proof share, seeds: by aggregator and circuit) and from the
            // root sum on (accumulated root sum and FLP, result and status planes)
            // are cleared whole.  C2: 409 of 2,107 header words per report.
            // (work_layout order: key, nonce, cw_* | lps, seed, peer | rk_*, sp_* | rootsum .. status)
            HIPCHK(c, hipMemsetAsync(W + wl.lps * (size_t)stride, 0, (wl.rk_ext - wl.lps) * (size_t)stride * 4, c->stream));
            HIPCHK(c, hipMemsetAsync(W + wl.rootsum * (size_t)stride, 0, (wl.cs[0] - wl.rootsum) * (size_t)stride * 4,
                                     c->stream));
            if (stride > n)
                HIPCHK(c, hipMemset2DAsync(W + n, (size_t)stride * 4, 0, (size_t)(stride - n) * 4, wl.lps, c->stream));
            // level 0 reads its parent (the root) payload from fr_w[1]: zeros
            HIPCHK(c, hipMemsetAsync(W + wl.fr_w[1] * (size_t)stride, 0, (size_t)p.value_len * p.w32 * stride * 4, c->stream));
        }
        const size_t ps = mc_public_share_size(p), is = mc_input_share_size(p, agg_id);
        const uint8_t* pub = rep->pub.as<uint8_t>() + ps * base;
        const uint8_t* in_b = (agg_id == 0 ? rep->in0 : rep->in1).as<uint8_t>() + is * base;
        const int l_lo = hit ? t->L - 1 : 0, l_hi = t->L + 1;  // a hit recomputes level L-1's payloads: its CW
        // Rows of >= 16 KB to unpack per report (C4, C5), 8-byte aligned
        // (BITS a multiple of 32): the correction words and the leader proof
        // share, the bulk of a report's bytes, go through coalesced row tiles;
        // k_unpack keeps the nonce, key, control bits and seeds.  Same-box A/B
        // (profiles/r05_v37_ab_row_tile_unpack.txt): C5 +2.2 %, C4 +0.5 %;
        // the 1M sweep's rows (<= 5.9 KB) gained nothing in wall time (+0.1 %)
        // while its level kernels, started earlier under the previous chunk's
        // sponges, measured 1.3 % longer, so small rows keep one lane per report.
        const size_t nctrl = (2 * (size_t)p.bits + 7) / 8;
        const size_t row_bytes = (size_t)(l_hi - l_lo) * (16 + (size_t)p.value_len * p.enc + 32) +
                                 (agg_id == 0 ? (size_t)p.proof_len * p.enc : 0);
        // (grid y of every row-tile launch below: 64 words per workgroup row)
        const size_t max_words = std::max<size_t>((size_t)p.value_len * p.w32 * (l_hi - l_lo),
                                                  agg_id == 0 ? (size_t)p.proof_len * p.w32 : 0);
        const bool tiles = row_bytes >= 16384 && (((uintptr_t)pub | (uintptr_t)in_b | ps | is | nctrl) & 7) == 0 &&
                           (max_words + 63) / 64 < 65535;
        hipLaunchKernelGGL(k_unpack, dim3((n + 255) / 256), dim3(256), 0, c->stream, p, pl, agg_id,
                           rep->nonces.as<uint8_t>() + 16 * base, pub, in_b, l_lo, l_hi, tiles ? 1 : 0,
                           rep->wire_flags.as<uint8_t>() + base);
        if (tiles) {
            const int wlw_ = wlw(), nl = l_hi - l_lo;
            auto rows = [&](const uint8_t* src, size_t row_bytes, int nwords, uint32_t* dst) {
                if (nwords <= 0) return;
                hipLaunchKernelGGL(k_rows_to_planes, dim3((unsigned)((n + 63) / 64), (unsigned)((nwords + 63) / 64)),
                                   dim3(256), 0, c->stream, src, row_bytes, n, nwords, dst, stride);
            };
            const uint8_t* seg = pub + nctrl;
            rows(seg + 16 * (size_t)l_lo, ps, 4 * nl, pl.cw_seed + (size_t)4 * l_lo * stride);
            seg += 16 * (size_t)p.bits;
            rows(seg + (size_t)l_lo * p.value_len * p.enc, ps, wlw_ * nl, pl.cw_w + (size_t)wlw_ * l_lo * stride);
            seg += (size_t)p.bits * p.value_len * p.enc;
            rows(seg + 32 * (size_t)l_lo, ps, 8 * nl, pl.cw_proof + (size_t)8 * l_lo * stride);
            if (agg_id == 0) rows(in_b + 16, is, p.proof_len * p.w32, pl.lps);
        }
        HIPCHK(c, hipGetLastError());
        return 0;
    }

    // k_setup (AES key schedules, sponge states) unless the arena still holds
    // this batch's (mastic_ctx::rk); a hit's sponge states and root sum from the cache.
    int setup() {
        const bool whole = base == 0 && (size_t)n == rep->n && W == c->work.p;
        const bool rk_ok = hit && whole && c->rk.valid && c->rk.rep_id == rep->id &&
                           c->rk.rep_gen == rep->generation() && c->rk.n == (size_t)n && c->rk.stride == stride &&
                           c->rk.W == (const void*)W && c->rk.pfx_key == c->pfx_key;
        if (!rk_ok) {
            hipLaunchKernelGGL(k_setup, dim3((stride + 255) / 256), dim3(256), 0, c->stream, pl,
                               (const PrefixState*)c->pfx.p, hit ? 0 : 1);
            c->rk = {whole, rep->id, rep->generation(), (size_t)n, stride, (const void*)W, c->pfx_key};
        }
        HIPCHK(c, hipGetLastError());
        if (hit && !direct) {
            // levels 0..L-1 from the cache (its planes' columns base .. base + n).
            // The binder messages are BFS-ordered (mastic.py:263-275), so the
            // cached call's message is a prefix of this one's: both sponges resume
            // from their states at the end of the cached call (mid-block,
            // unpadded; k_finalize pads a register copy); and the root sum of the
            // cached level-0 evaluation (counter check).
            auto from_cache = [&](uint32_t* dst, const uint32_t* src, size_t planes) {
                return hipMemcpy2DAsync(dst, (size_t)stride * 4, src + base, lc->S * 4, (size_t)n * 4, planes,
                                        hipMemcpyDeviceToDevice, c->stream);
            };
            HIPCHK(c, from_cache(pl.sp_onehot, lc->sp.as<uint32_t>(), 50));
            HIPCHK(c, from_cache(pl.sp_payload, lc->sp.as<uint32_t>() + (size_t)50 * lc->S, 50));
            HIPCHK(c, from_cache(pl.rootsum, lc->rootsum.as<uint32_t>(), (size_t)wlw()));
        }
        return 0;
    }

    // One timing sextuple [aes0, aes1, proof0, proof1, absorb0, absorb1] of a
    // step (mastic_last_timing3 decodes strides of six): the first four are
    // recorded here on stream s, with `kernel` launched inside pair `slot`
    // (0 aes, 1 proof; -1: no kernel, both pairs empty); the absorb pair goes to
    // the step's sponge launch.
    template <class Fn>
    int timed_step(hipStream_t s, int slot, Fn&& kernel, hipEvent_t* e4, hipEvent_t* e5) {
        for (int i = 0; i < 4; i++) {
            HIPCHK(c, hipEventRecord(get_event(c, evi++), s));
            if (i == 2 * slot) kernel();
            if (i == 2 * slot + 1) HIPCHK(c, hipGetLastError());
        }
        *e4 = get_event(c, evi++);
        *e5 = get_event(c, evi++);
        return 0;
    }

    // The planned sponges [sp0, sp1) of a step whose end `ready` marks, each on
    // its stream after `ready`; (e4, e5): the absorb pair of the step's timing
    // sextuple.  Their ends are marked in c->sp_done.  The fill positions carry
    // across pieces as across levels (the plan tracks them).
    int launch_sponges(int sp0, int sp1, hipEvent_t ready, hipEvent_t e4, hipEvent_t e5) {
        for (int i = sp0; i < sp1; i++) {
            const SpongeLaunch& s = plan.sponges[i];
            const hipStream_t as = stream(s.stream);
            // the sponge's previous piece ran on another stream
            if (s.prev >= 0) HIPCHK(c, hipStreamWaitEvent(as, c->sp_done[s.prev], 0));
            hipEvent_t m4 = s.marks == MK_STEP ? e4 : nullptr, m5 = s.marks == MK_STEP ? e5 : nullptr;
            // a sponge piece that has no level-kernel launch of its own: an event
            // sextuple whose kernel pairs are empty
            if (s.marks == MK_PIECE && timed_step(as, -1, [] {}, &m4, &m5)) return MASTIC_EHIP;
            AbsorbArgs ab;
            ab.which0 = s.which0;
            ab.seg[0] = oh_buf(s.level) + (size_t)s.piece.node0 * 8 * bin_rstride;
            ab.gstride[0] = oh_gstride;
            ab.nbytes[0] = s.piece.nodes * 32;
            ab.f[0] = s.f_oh;
            ab.seg[1] = pay_buf(s.level) + (size_t)s.piece.parent0 * wlw() * bin_rstride;
            ab.gstride[1] = pay_gstride;
            ab.rstride = bin_rstride;
            ab.nbytes[1] = s.level > 0 ? s.piece.parents * wlw() * 4 : 0;
            ab.f[1] = s.f_pl;
            // The priority and debug arguments of AbsorbArgs and AesArgs were
            // experiment knobs; their A/Bs are settled and the executor pins the
            // values.  The fields stay in kernels.hpp because taking them out
            // moves the kernels' register allocation (DESIGN.md "Retired knobs").
            ab.prio = 3;
            ab.dbg = 0;
            if (as != c->stream) HIPCHK(c, hipStreamWaitEvent(as, ready, 0));
            if (m4) HIPCHK(c, hipEventRecord(m4, as));
            if (plan.pair)
                hipLaunchKernelGGL(k_absorb_pair, dim3((groups() * 64 * 2 + 255) / 256, (unsigned)s.nwh), dim3(256), 0, as,
                                   pl, ab);
            else
                hipLaunchKernelGGL(k_absorb, dim3((groups() * 64 + 255) / 256, (unsigned)s.nwh), dim3(256), 0, as, pl, ab);
            if (m5) HIPCHK(c, hipEventRecord(m5, as));
            HIPCHK(c, hipGetLastError());
            const hipEvent_t done = c->sp_done[i] = get_sync_event(c, sev++);
            HIPCHK(c, hipEventRecord(done, as));
            // measurement schedule (mastic_set_serial_sponges): the main stream waits
            // for this launch, so it runs alone on the chip (standalone sponge rate)
            if (c->serial_sponges && as != c->stream) HIPCHK(c, hipStreamWaitEvent(c->stream, done, 0));
            for (int w = s.which0; w < s.which0 + s.nwh; w++) (w ? c->pl_done : c->oh_done)[s.level] = done;
        }
        if (sp0 == sp1) {
            // no sponge follows (level 0 of a miss, a hit's level kernel): empty marks
            if (c->sponge_delay_us > 0) {
                // test hook: the sponge stream is still busy when these (empty)
                // marks are recorded there; nothing on the main stream waits for them
                const unsigned long long ticks =
                    (unsigned long long)c->sponge_delay_us * (unsigned long long)c->wall_khz / 1000;
                c->sponge_delay_us = 0;
                hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, ss, ticks);
                HIPCHK(c, hipGetLastError());
            }
            HIPCHK(c, hipEventRecord(e4, ss));
            HIPCHK(c, hipEventRecord(e5, ss));
        }
        return 0;
    }

    // One planned level-kernel launch (a whole level, or one parent range of a
    // segmented last level) on the main stream: the pointers of AesArgs from the
    // launch's level, parent range and proof job.
    template <class F>
    void launch_level(const LevelLaunch& v) {
        const int l = v.level, wlw = this->wlw();
        const size_t p0 = (size_t)v.p0;
        uint32_t* cs_level = plane(wl.cs[l & 1]);
        AesArgs a;
        a.level = l;
        a.agg_id = agg_id;
        a.n_parents = v.cnt;
        a.split = v.split;
        a.split_blocks = v.split_blocks;
        a.ppw = v.ppw;
        a.parent_node = t->d_parent + t->poff[l] + p0;
        a.child_exp = t->d_exp + t->off[l] + 2 * p0;
        a.child_pfx = t->d_pfx + t->off[l] + 2 * p0;
        // by child node / parent ordinal of the range: planes of the work
        // buffer, rows of the (tiled) payload-difference buffer
        a.cs_in = hit ? cin + base : plane(wl.cs[(l + 1) & 1]);
        a.cs_out = cs_level + 2 * p0 * 5 * stride;
        a.fr_w_in = plane(wl.fr_w[(l + 1) & 1]) + p0 * wlw * stride;
        a.in_stride = hit ? (int)lc->S : stride;
        a.fr_w_out = plane(wl.fr_w[l & 1]);
        a.payload = pay_buf(l) + p0 * wlw * bin_rstride;
        a.out = c->res[agg_id].out.as<uint32_t>() + base;  // columns base .. base + n of the result planes
        a.out_stride = (int)c->res[agg_id].stride;
        a.force_slow_blk = c->force_slow_blk;
        // frontier cache: stage this level's convert seeds (last level); on a
        // hit recompute the parents' payloads from the cached ones into the
        // (otherwise unused) parent-payload planes
        a.cache_out = (lc && l == t->L) ? cout + base + 2 * p0 * (size_t)out_nw * lc->S : nullptr;
        a.cache_stride = lc ? (int)lc->S : 0;
        a.wp_buf = plane(wl.fr_w[(l + 1) & 1]);
        // a payloads-format slot holds the parents' next seeds and payloads: nothing to recompute
        a.in_nw = hit ? in_nw : SEED_NODE_WORDS;
        a.out_nw = out_nw;
        a.recompute_wp = (hit && in_nw == SEED_NODE_WORDS) ? 1 : 0;
        a.fuse_proofs = v.fuse_proofs;
        a.cur_path_bytes = (l + 1 + 7) / 8;
        a.cur_child_path = t->d_path + (t->off[l] + 2 * p0) * 8;
        a.cur_onehot = oh_buf(l);
        a.aes_waves = v.aes_waves;
        a.par_waves = v.par_waves;
        a.proof_prio = a.aes_prio = a.dbg_skip = 0;  // pinned (launch_sponges)
        // the proof job: level l-1's nodes (seeds in cs_in), or an earlier range
        // of this level's (the previous launch's cs_out)
        const size_t n0 = (size_t)v.pv_node0;
        a.pv_level = v.pv_level;
        a.pv_nodes = v.pv_nodes;
        a.pv_npw = v.pv_npw;
        a.pv_path_bytes = (v.pv_level + 1 + 7) / 8;
        a.pv_child_path = v.pv_level >= 0 ? t->d_path + (t->off[v.pv_level] + n0) * 8 : nullptr;
        a.pv_onehot = v.pv_level >= 0 ? oh_buf(v.pv_level) + n0 * 8 * bin_rstride : nullptr;
        a.pv_cs = v.pv_level == l ? cs_level + n0 * 5 * stride : a.cs_in;
        a.oh_gstride = oh_gstride;
        a.pay_gstride = pay_gstride;
        a.bin_rstride = bin_rstride;
        a.np = (const PrefixState*)c->pfx.p + PFX_NODE;
        a.np_f = c->pfx_f[PFX_NODE];
        // the FC kernel that knows the payloads node format, where a slot of this launch has it
        const bool pay = (v.variant & LV_FC) && (a.in_nw > SEED_NODE_WORDS || (a.cache_out && a.out_nw > SEED_NODE_WORDS));
        hipLaunchKernelGGL(level_kernel<F>(pay ? LV_FC_PAY : v.variant), dim3(groups(), v.gy), dim3(64 * EVAL_WAVES), EVAL_LDS_BYTES,
                           c->stream, c->p, pl, a);
    }

    // The planned launches in order: each level kernel on the main stream, then
    // its sponges; then the final step (the last level's remaining node proofs,
    // or marks only) and its sponges.  Timing: one event sextuple per step.
    template <class F>
    int run_plan() {
        c->sp_done.assign(plan.sponges.size(), nullptr);
        c->oh_done.assign(t->L + 1, nullptr);
        c->pl_done.assign(t->L + 1, nullptr);
        hipEvent_t e4, e5;
        for (const LevelLaunch& v : plan.launches) {
            if (v.wait_level >= 0) {
                // proof / payload ring of NSLOT slots: this launch overwrites that level's
                const hipEvent_t oh = c->oh_done[v.wait_level], pay = c->pl_done[v.wait_level];
                HIPCHK(c, hipStreamWaitEvent(c->stream, oh, 0));
                if (pay && pay != oh) HIPCHK(c, hipStreamWaitEvent(c->stream, pay, 0));
            }
            if (int rc = timed_step(c->stream, 0, [&] { launch_level<F>(v); }, &e4, &e5)) return rc;
            hipEvent_t aes_done = get_sync_event(c, sev++);
            HIPCHK(c, hipEventRecord(aes_done, c->stream));
            if (int rc = launch_sponges(v.sp0, v.sp1, aes_done, e4, e5)) return rc;
        }
        const int l = t->L;
        ProofArgs pa;
        pa.level = l;
        pa.n_nodes = plan.final_nn;
        pa.npw = plan.final_npw;
        pa.path_bytes = (l + 1 + 7) / 8;
        pa.child_path = t->d_path + (t->off[l] + (size_t)plan.final_n0) * 8;
        pa.cs = plane(wl.cs[l & 1]) + (size_t)plan.final_n0 * 5 * stride;
        pa.onehot = oh_buf(l) + (size_t)plan.final_n0 * 8 * bin_rstride;
        pa.oh_gstride = oh_gstride;
        pa.bin_rstride = bin_rstride;
        pa.np = (const PrefixState*)c->pfx.p + PFX_NODE;
        pa.f = c->pfx_f[PFX_NODE];
        auto node_proofs = [&] {
            hipLaunchKernelGGL(k_node_proof, dim3(groups(), (pa.n_nodes + 4 * pa.npw - 1) / (4 * pa.npw)), dim3(256), 0,
                               c->stream, c->p, pl, pa);
        };
        // (a fused last level: its proofs came from the level kernel's AES waves)
        if (int rc = timed_step(c->stream, plan.fuse_last ? -1 : 1, node_proofs, &e4, &e5)) return rc;
        hipEvent_t np_done = get_sync_event(c, sev++);
        HIPCHK(c, hipEventRecord(np_done, c->stream));
        const int n_sponges = (int)plan.sponges.size();  // the last one is the final step's
        return launch_sponges(n_sponges - 1, n_sponges, np_done, e4, e5);
    }

    // FLP side stream, k_finalize, then the cache and result copies on the tail stream.
    template <class F>
    int finish() {
        const McParams& p = c->p;
        const PrefixState* pfx = (const PrefixState*)c->pfx.p;
        hipEvent_t flp_done = nullptr;
        if (t->weight_check) {
            // The FLP randomness and query (mastic.py:234-256) read only header
            // planes and level 0's root sum: on their own stream once the last
            // level kernel is done, beside the last level's sponges (a few
            // latency-bound chains that leave most of the chip idle: C5's last
            // payload chain runs ~34 ms) instead of after them.  (Right after
            // level 0 they slowed the level kernels beside them by as much as
            // they saved: C4 -1.8 %, profiles/r05_v36_ab_flp_side_stream.txt.)
            hipEvent_t lv_done = get_sync_event(c, sev++);
            HIPCHK(c, hipEventRecord(lv_done, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->stream4, lv_done, 0));
            FlpArgs fl{agg_id, t->L};
            hipLaunchKernelGGL(k_flp_rand<F>, dim3((stride + 255) / 256), dim3(256), 0, c->stream4, p, pl, fl, pfx);
            hipLaunchKernelGGL(k_flp_query<F>, dim3((stride + 255) / 256), dim3(256), 0, c->stream4, p, pl,
                               flp_consts<F>(p));
            HIPCHK(c, hipGetLastError());
            flp_done = get_sync_event(c, sev++);
            HIPCHK(c, hipEventRecord(flp_done, c->stream4));
        }
        // the tail follows the last piece of either sponge
        const hipEvent_t oh = c->oh_done[t->L], pay = c->pl_done[t->L];
        if (tail != stream(plan.last_stream)) HIPCHK(c, hipStreamWaitEvent(tail, oh, 0));
        if (pay && pay != oh) HIPCHK(c, hipStreamWaitEvent(tail, pay, 0));  // split schedule, segmented last level
        FinalArgs fa{agg_id, plan.f_oh, plan.f_pl};
        hipLaunchKernelGGL(k_finalize<F>, dim3((stride + 255) / 256), dim3(256), 0, tail, p, pl, fa, pfx);
        HIPCHK(c, hipGetLastError());
        // the status, verifier and joint-rand planes copied below are the FLP's
        if (flp_done) HIPCHK(c, hipStreamWaitEvent(tail, flp_done, 0));
        if (lc && !direct) {
            // work planes of this chunk -> cache planes (columns base .. base + n)
            auto to_cache = [&](uint32_t* dst, const uint32_t* src, size_t planes) {
                return hipMemcpy2DAsync(dst + base, lc->S * 4, src, (size_t)stride * 4, (size_t)n * 4, planes,
                                        hipMemcpyDeviceToDevice, tail);
            };
            // frontier cache for the next level (the last level's nodes are in the
            // spare slot already, written by its level kernel): the root sum
            if (!hit) HIPCHK(c, to_cache(lc->rootsum.as<uint32_t>(), pl.rootsum, (size_t)wlw()));
            // both sponges after levels 0..L (the tail waited for them above)
            HIPCHK(c, to_cache(lc->sp.as<uint32_t>(), pl.sp_onehot, 50));
            HIPCHK(c, to_cache(lc->sp.as<uint32_t>() + (size_t)50 * lc->S, pl.sp_payload, 50));
        }
        // results -> the agg_id slot (plane stride = all reports; the level
        // kernel wrote the out shares there)
        Result& R = c->res[agg_id];
        int rc = 0;
        rc |= copy_planes(c, R.eval_proof, R.stride, base, pl.eval_proof, stride, n, 8, tail);
        rc |= copy_planes(c, R.status, R.stride, base, (const uint32_t*)pl.status, stride, n, 1, tail);
        if (t->weight_check) {
            rc |= copy_planes(c, R.verifier, R.stride, base, pl.verifier, stride, n, (size_t)p.verifier_len * p.w32,
                              tail);
            if (p.joint_rand_len > 0) {
                rc |= copy_planes(c, R.jr_part, R.stride, base, pl.jr_part, stride, n, 8, tail);
                rc |= copy_planes(c, R.jr_seed, R.stride, base, pl.jr_seed, stride, n, 8, tail);
            }
        }
        return rc;
    }

    // Runs one chunk: unpack, key setup, the planned launches, finish.  The plan
    // also says how many sync and timing events the chunk takes: prep_init spaces
    // pipelined chunks' sync events by the former, and mastic_last_timing3
    // decodes the latter in strides of six, so a step that consumed another
    // number than planned is an error here, not a miscount there.  The check
    // is a tripwire for a plan and an executor that have drifted apart: it runs
    // after the chunk's work is queued, so it cannot keep a pipelined chunk
    // that overran its range from sharing sync events with its neighbour, only
    // fail the call (whose results are then never marked ready).  The C ABI has
    // no code for an internal error; MASTIC_EHIP with this text is the nearest.
    template <class F>
    int run() {
        const size_t evi0 = evi, sev0 = sev;
        pl = make_planes(W, wl, n, stride);
        direct = lc && base == 0 && (size_t)n == rep->n && lc->S == (size_t)stride;
        if (direct) {
            pl.sp_onehot = lc->sp.as<uint32_t>();
            pl.sp_payload = lc->sp.as<uint32_t>() + (size_t)50 * lc->S;
            pl.rootsum = lc->rootsum.as<uint32_t>();
        }
        oh_gstride = t->max_level_nodes * 8 * 64;
        pay_gstride = t->max_parents * wlw() * 64;
        int rc = unpack();
        if (rc || (rc = setup()) || (rc = run_plan<F>()) || (rc = finish<F>())) return rc;
        if (evi - evi0 != (size_t)plan.n_timing || sev - sev0 != (size_t)plan.n_sync)
            return fail(c, MASTIC_EHIP, "chunk used %zu timing and %zu sync events, its plan says %d and %d",
                        evi - evi0, sev - sev0, plan.n_timing, plan.n_sync);
        return 0;
    }
};

// Free HBM now (none: the query failed).
static std::optional<size_t> free_hbm() {
    size_t freeb = 0, total = 0;
    if (hipMemGetInfo(&freeb, &total) != hipSuccess) return std::nullopt;
    return freeb;
}

static uint64_t default_budget(mastic_ctx* c) {
    return default_budget(c->m, c->m.budget ? std::nullopt : free_hbm());
}

// Results and cache slots: HBM is held by the work arena (sized to the budget
// when the results were smaller) and by retired buffers, so the recovery frees
// both; the arena is re-allocated afterwards, within what is left (a
// 2M-report sweep's out shares reach 32 GB per aggregator).
static constexpr mastic_ctx::Reclaim RECLAIM_ALL{true, true, false, false};
// The work arena itself: only the retired buffers (cache slots, evicted trees) can make room.
static constexpr mastic_ctx::Reclaim RECLAIM_BURIED{false, false, true, true};

// The result buffers of a call over n reports.  One that must grow retires the
// old buffer (mastic_ctx::retire) and allocates with headroom, like DevBuf::grow.
static int size_results(mastic_ctx* c, Result& R, const Tree* t, size_t n) {
    const McParams& p = c->p;
    R.ready = false;
    R.n = n;
    R.stride = round_up(std::max<size_t>(n, 1), 64);
    R.weight_check = t->weight_check;
    R.n_prefixes = t->n_prefixes;
    const size_t S = R.stride;
    auto rgrow = [&](DevBuf& d, size_t want) {
        if (want <= d.bytes && d.p) return true;
        const size_t old = d.bytes;
        c->retire(d);
        d.own = true;
        return c->reclaim_ensure(d, std::max(want, old + old / 2), want, RECLAIM_ALL);
    };
    if (!rgrow(R.eval_proof, S * 8 * 4) || !rgrow(R.status, S * 4) ||
        !rgrow(R.out, S * 4 * std::max<size_t>(1, (size_t)t->n_prefixes * (1 + p.output_len) * p.w32)) ||
        !rgrow(R.verifier, S * 4 * (size_t)p.verifier_len * p.w32) || !rgrow(R.jr_part, S * 32) ||
        !rgrow(R.jr_seed, S * 32))
        return fail(c, MASTIC_ENOMEM, "out of device memory (results for %zu reports)", n);
    HIPCHK(c, hipMemsetAsync(R.jr_part.p, 0, S * 32, c->stream));
    HIPCHK(c, hipMemsetAsync(R.jr_seed.p, 0, S * 32, c->stream));
    return 0;
}

// What a call does with the frontier cache.
struct CacheUse {
    LevelCache* lc = nullptr;       // null: the call evaluates without the cache
    bool hit = false;               // it evaluates only its last level
    const uint32_t* cin = nullptr;  // a hit's parents: this aggregator's node slot
    uint32_t* cout = nullptr;       // the last level's nodes: the spare node slot
    int in_nw = SEED_NODE_WORDS;    // words per node of cin (the format of the call that wrote it)
    int out_nw = SEED_NODE_WORDS;   // words per node this call writes into cout
};

// Frontier cache: decide hit / miss and size the slots.  Runs before the work
// arena is sized, so the HBM budget sees the cache.
static CacheUse cache_slots(mastic_ctx* c, int agg_id, const Tree* t, const mastic_reports* rep,
                            const std::vector<uint8_t>& lkey) {
    CacheUse u;
    if (!c->frontier_cache) {
        c->lc[agg_id].drop();
        return u;
    }
    LevelCache* lc = &c->lc[agg_id];
    const size_t S1 = round_up(rep->n, 64) + (size_t)c->m.stride_pad;
    u.hit = frontier_hit(*lc, *t, rep->id, rep->generation(), rep->n, S1, lkey);
    if (lc->S != S1) {
        c->retire(lc->sp);
        c->retire(lc->rootsum);
        c->retire(lc->nd);
        lc->nd_words = 0;
        lc->S = S1;
    }
    if (c->spare_S != S1) {
        c->retire(c->fc_spare);
        c->spare_words = 0;
        c->spare_S = S1;
    }
    const size_t wlw = (size_t)c->p.value_len * c->p.w32;
    const size_t nl = (size_t)2 * t->n_parents[t->L];
    bool ok = c->reclaim_ensure(lc->sp, 0, 100 * S1 * 4, RECLAIM_ALL) &&
              c->reclaim_ensure(lc->rootsum, 0, wlw * S1 * 4, RECLAIM_ALL);
    // The format this call writes (memplan.hpp choose_node_words); auto asks for the free HBM.
    std::optional<size_t> free_bytes;
    bool queried = false;
    auto free_now = [&] {
        if (!queried) free_bytes = free_hbm();
        queried = true;
        return free_bytes;
    };
    const size_t held = c->lc[0].nd.bytes + c->lc[1].nd.bytes + c->fc_spare.bytes;
    const bool by_rule = c->fc_nodes == FC_NODES_AUTO;
    size_t nw = (size_t)choose_node_words(c->fc_nodes, nl, wlw, S1, by_rule ? free_now() : std::nullopt, held);
    if (ok && !slot_holds(c->spare_words, nl, nw)) {
        // the spare may be a former slot that queued kernels still read:
        // retire it, and free the retired buffers first
        const size_t old_words = c->spare_words;
        c->retire(c->fc_spare);
        c->spare_words = 0;
        if (c->idle()) c->bury();
        if (nw > SEED_NODE_WORDS) {
            // the wide format is an optimisation: one attempt, no draining of the
            // streams or release of the work arena for it; else seeds width
            const size_t words = spare_slot_words(nl, nw, old_words, free_now(), S1, by_rule, held);
            if (!c->inject_alloc_failure() && c->fc_spare.ensure(words * S1 * 4))
                c->spare_words = words;
            else
                nw = SEED_NODE_WORDS;
        }
        if (nw == SEED_NODE_WORDS) {
            const size_t words = spare_slot_words(nl, nw, old_words, free_now(), S1);
            ok = c->reclaim_ensure(c->fc_spare, 0, words * S1 * 4, RECLAIM_ALL);
            if (ok) c->spare_words = words;
        }
    }
    if (!ok) {  // not enough HBM for the cache: evaluate without it
        lc->release();
        return CacheUse();
    }
    if (!u.hit) lc->drop();  // refilled by this call
    u.lc = lc;
    u.cin = u.hit ? lc->nd.as<uint32_t>() : nullptr;
    u.cout = c->fc_spare.as<uint32_t>();
    u.in_nw = u.hit ? lc->node_words : SEED_NODE_WORDS;
    u.out_nw = (int)nw;
    return u;
}

// The work arena of a call: used as it is, or re-allocated (memplan.hpp
// plan_arena).  *by_budget: the reports per chunk the call's budget allows.
static int size_arena(mastic_ctx* c, size_t n, size_t per_report, bool cache_on, size_t* by_budget) {
    const bool fits = arena_fits(c->m, n, per_report, c->work.bytes);
    const uint64_t budget =
        call_budget(c->m, n, per_report, fits, cache_on, (fits || c->m.budget) ? std::nullopt : free_hbm());
    const ArenaPlan a = plan_arena(c->m, n, per_report, c->work.bytes, budget, cache_on);
    *by_budget = a.by_budget;
    if (a.action == ArenaPlan::TOO_SMALL)
        return fail(c, MASTIC_ENOMEM, "work buffers of 64 reports exceed the memory budget");
    if (a.action == ArenaPlan::USE) return 0;
    c->rk.valid = false;  // the arena may be re-allocated (possibly at the same address)
    if (!c->reclaim_ensure(c->work, a.arena, a.want, RECLAIM_BURIED))
        return fail(c, MASTIC_ENOMEM, "out of device memory (work %zu bytes)", a.want);
    return 0;
}

extern "C" int mastic_prep_init(mastic_ctx* c, mastic_reports* rep, const uint8_t* verify_key, size_t vk_len,
                                const uint8_t* app_ctx, size_t ctx_len, int agg_id, const uint8_t* enc_agg_param,
                                size_t agg_param_len) {
    DeviceScope ds_(c);
    if (!c || !rep || rep->ctx != c) return fail(c, MASTIC_EINVAL, "bad ctx/reports");
    if (agg_id != 0 && agg_id != 1) return fail(c, MASTIC_EINVAL, "invalid aggregator ID");
    if ((agg_id == 0 && !rep->in0.p) || (agg_id == 1 && !rep->in1.p))
        return fail(c, MASTIC_EINVAL, "reports hold no input shares for this aggregator");
    if (!verify_key && vk_len) return fail(c, MASTIC_EINVAL, "verify key required");
    static const uint8_t empty_vk[1] = {0};
    if (!verify_key) verify_key = empty_vk;
    c->tcur = agg_id;
    Tree* t = nullptr;
    int rc = build_tree(c, enc_agg_param, agg_param_len, &t);
    if (rc) return rc;
    if ((rc = build_prefixes(c, app_ctx, ctx_len, verify_key, vk_len))) return rc;
    const McParams& p = c->p;
    WorkLayout wl = work_layout(p, t);
    const size_t n = rep->n;
    Result& R = c->res[agg_id];
    if ((rc = size_results(c, R, t, n))) return rc;
    if (n == 0) {
        R.ready = true;
        return 0;
    }
    const size_t pad = (size_t)c->m.stride_pad;
    std::vector<uint8_t> lkey(1, (uint8_t)vk_len);
    lkey.insert(lkey.end(), verify_key, verify_key + vk_len);
    lkey.insert(lkey.end(), app_ctx, app_ctx + ctx_len);
    const CacheUse cu = cache_slots(c, agg_id, t, rep, lkey);
    LevelCache* const lc = cu.lc;
    const bool hit = cu.hit;
    size_t by_budget = 0;
    if ((rc = size_arena(c, n, wl.words * 4, lc != nullptr, &by_budget))) return rc;
    // the chunks (memplan.hpp), and the launch plans (schedule.hpp) of a full chunk and, if shorter, of the last one
    const ChunkSizes cs = plan_chunks(c->m, n, wl.words * 4, c->work.bytes, by_budget);
    const size_t chunk = cs.chunk;
    const bool pipe = cs.pipe;
    ChunkPlan* plans[2] = {&c->plans[0], &c->plans[cs.n_last != cs.n_full]};
    for (int i = 0; i <= (cs.n_last != cs.n_full); i++)
        plan_chunk(c->k, p, *t, (int)(i ? cs.n_last : cs.n_full), hit, lc != nullptr, pipe, c->pfx_f[PFX_ONEHOT],
                   c->pfx_f[PFX_PAYLOAD], plans[i]);
    // sync events one chunk uses: pipelined chunks alternate between two disjoint ranges of them
    const size_t nsev = (size_t)std::max(plans[0]->n_sync, plans[1]->n_sync);
    size_t evi = 0;
    hipEvent_t t0 = get_event(c, evi++), t1 = get_event(c, evi++);
    HIPCHK(c, hipEventRecord(t0, c->stream));
    hipEvent_t half_free[2] = {get_sync_event(c, 2 * nsev), get_sync_event(c, 2 * nsev + 1)};
    for (size_t b = 0, k = 0; b < n; b += chunk, k++) {
        const int nn = (int)std::min(chunk, n - b), stride = (int)(round_up(nn, 64) + pad);
        const int h = pipe ? (int)(k & 1) : 0;
        if (pipe && k >= 2) HIPCHK(c, hipStreamWaitEvent(c->stream, half_free[h], 0));
        uint32_t* W = c->work.as<uint32_t>() + h * cs.half;
        // pipelined chunks alternate between two sponge streams: a chunk's
        // sponges must not queue behind the previous chunk's trailing ones
        hipStream_t ss = (pipe && h) ? c->stream3 : c->stream2, tail = pipe ? ss : c->stream;
        Chunk ck{c, rep, t, wl, *plans[b + chunk >= n], agg_id, nn, stride, b, W, ss, tail, lc, hit, cu.cin, cu.cout,
                 cu.in_nw, cu.out_nw, evi, h * nsev};
        rc = p.field == 64 ? ck.run<F64>() : ck.run<F128>();
        if (rc) {
            if (lc) lc->drop();
            return rc;
        }
        if (pipe) HIPCHK(c, hipEventRecord(half_free[h], ss));
    }
    if (pipe) {
        // later work on the main stream (results, aggregate, the next call) sees every chunk's tail
        hipEvent_t done = get_sync_event(c, 2 * nsev + 2), done3 = get_sync_event(c, 2 * nsev + 3);
        HIPCHK(c, hipEventRecord(done, c->stream2));
        HIPCHK(c, hipEventRecord(done3, c->stream3));
        HIPCHK(c, hipStreamWaitEvent(c->stream, done, 0));
        HIPCHK(c, hipStreamWaitEvent(c->stream, done3, 0));
    }
    if (lc) {
        // the spare slot now holds this call's last level: it becomes the
        // aggregator's slot, and the old slot (read by this call's hit) the
        // spare, overwritten only by later calls' kernels (stream order)
        std::swap(lc->nd.p, c->fc_spare.p);
        std::swap(lc->nd.bytes, c->fc_spare.bytes);
        std::swap(lc->nd_words, c->spare_words);
        frontier_commit(*lc, *t, rep->id, rep->generation(), n, lkey, cu.out_nw);
    }
    c->last_hit = hit;
    auto fmt = [](int nw) { return nw > SEED_NODE_WORDS ? FC_NODES_PAYLOADS : FC_NODES_SEEDS; };
    c->last_nodes_in = hit ? fmt(cu.in_nw) : -1;
    c->last_nodes_out = lc ? fmt(cu.out_nw) : -1;
    HIPCHK(c, hipEventRecord(t1, c->stream));
    c->tm[c->tcur].n_eval = -(int)evi;  // timing pending (resolved by mastic_last_timing)
    R.ready = true;
    return 0;
}

// Report-major wire rows of plane segments into dst (device), on c->stream.
static int gather_rows(mastic_ctx* c, const RowSegs& sg, size_t n, size_t stride, void* dst) {
    const size_t words = (size_t)sg.words[0] + sg.words[1] + sg.words[2];
    if (n == 0 || words == 0) return 0;
    const size_t total = n * words;
    // grid-stride kernel: at most 2^20 workgroups (2^28 work-items) per launch
    const size_t blocks = std::min<size_t>((total + 255) / 256, (size_t)1 << 20);
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)blocks), dim3(256), 0, c->stream, sg, (int)n, (int)stride,
                       (uint32_t*)dst);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// The prep shares of result slot R as wire rows (mastic.py:543-552):
// eval_proof || [jr_part] || [verifier].
static RowSegs prep_share_segs(const McParams& p, const Result& R) {
    RowSegs sg{};
    sg.seg[0] = R.eval_proof.as<uint32_t>();
    sg.words[0] = 8;
    if (R.weight_check) {
        int k = 1;
        if (p.joint_rand_len > 0) {
            sg.seg[k] = R.jr_part.as<uint32_t>();
            sg.words[k++] = 8;
        }
        sg.seg[k] = R.verifier.as<uint32_t>();
        sg.words[k] = p.verifier_len * p.w32;
    }
    return sg;
}

extern "C" int mastic_prep_result(mastic_ctx* c, int agg_id, uint8_t* prep_shares, uint8_t* jr_seeds,
                                  uint8_t* out_shares, int32_t* status) {
    DeviceScope ds_(c);
    if (!c || (agg_id != 0 && agg_id != 1)) return fail(c, MASTIC_EINVAL, "invalid aggregator ID");
    Result& R = c->res[agg_id];
    if (!R.ready) return fail(c, MASTIC_EINVAL, "no prep_init result for this aggregator");
    c->tcur = agg_id;
    const McParams& p = c->p;
    const size_t n = R.n, S = R.stride;
    // Every output is encoded on the GPU into a staging buffer (planes ->
    // report-major wire bytes) and copied out once: no per-report host loop.
    auto emit = [&](const RowSegs& sg, void* host) -> int {
        const size_t bytes = n * 4 * ((size_t)sg.words[0] + sg.words[1] + sg.words[2]);
        if (!host || bytes == 0) return 0;
        if (!c->stage.grow(bytes)) return fail(c, MASTIC_ENOMEM, "out of device memory (result staging)");
        if (gather_rows(c, sg, n, S, c->stage.p)) return -1;
        HIPCHK(c, hipMemcpyAsync(host, c->stage.p, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    };
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->bury();  // the stream is idle (it joined the sponge stream before k_finalize)
    if (n == 0) return 0;
    if (emit(prep_share_segs(p, R), prep_shares)) return -1;
    if (jr_seeds && !(R.weight_check && p.joint_rand_len > 0)) {
        memset(jr_seeds, 0, 32 * n);  // no joint rand in this call
    } else if (emit(RowSegs{{R.jr_seed.as<uint32_t>(), nullptr, nullptr}, {8, 0, 0}}, jr_seeds)) {
        return -1;
    }
    const int ow = R.n_prefixes * (1 + p.output_len) * p.w32;
    if (emit(RowSegs{{R.out.as<uint32_t>(), nullptr, nullptr}, {ow, 0, 0}}, out_shares)) return -1;
    if (emit(RowSegs{{(const uint32_t*)R.status.p, nullptr, nullptr}, {1, 0, 0}}, status)) return -1;
    return 0;
}

extern "C" int mastic_decide_results(mastic_ctx* c, const uint8_t* app_ctx, size_t ctx_len, uint8_t* accept_out,
                                     uint8_t* decide_out) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    Result &R0 = c->res[0], &R1 = c->res[1];
    if (!R0.ready || !R1.ready) return fail(c, MASTIC_EINVAL, "decide needs both aggregators' prep_init results");
    if (R0.n != R1.n || R0.weight_check != R1.weight_check || R0.n_prefixes != R1.n_prefixes)
        return fail(c, MASTIC_EINVAL, "the two prep_init results are for different batches / agg params");
    const size_t n = R0.n, S = R0.stride;
    if (n == 0) return 0;
    int rc = build_prefixes(c, app_ctx, ctx_len, nullptr, 0);
    if (rc) return rc;
    const McParams& p = c->p;
    const size_t psz = mc_prep_share_size(p, R0.weight_check);
    // both prep shares as wire rows (k_decide's input), decide, accept
    const size_t need = 2 * n * psz + 32 * n + 2 * n + 256 + S * 4 * (size_t)std::max(1, p.verifier_len * p.w32);
    if (!c->stage.grow(need)) return fail(c, MASTIC_ENOMEM, "out of device memory (decide staging)");
    uint8_t* ps0 = c->stage.as<uint8_t>();
    uint8_t* ps1 = ps0 + n * psz;
    uint8_t* msg = ps1 + n * psz;
    uint8_t* code = msg + 32 * n;
    uint8_t* acc = code + n;
    uint32_t* ver = (uint32_t*)(((uintptr_t)(acc + n) + 255) & ~(uintptr_t)255);  // FLP scratch planes
    if (gather_rows(c, prep_share_segs(p, R0), n, S, ps0)) return -1;
    if (gather_rows(c, prep_share_segs(p, R1), n, S, ps1)) return -1;
    HIPCHK(c, hipMemsetAsync(msg, 0, 32 * n, c->stream));
    const dim3 grid((unsigned)((n + 255) / 256));
    if (p.field == 64)
        hipLaunchKernelGGL(k_decide<F64>, grid, dim3(256), 0, c->stream, p, (int)n, (int)S, R0.weight_check, ps0, ps1,
                           (int)psz, ver, (const PrefixState*)c->pfx.p, msg, code);
    else
        hipLaunchKernelGGL(k_decide<F128>, grid, dim3(256), 0, c->stream, p, (int)n, (int)S, R0.weight_check, ps0,
                           ps1, (int)psz, ver, (const PrefixState*)c->pfx.p, msg, code);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(k_accept, grid, dim3(256), 0, c->stream, (int)n, (int)S,
                       (int)(R0.weight_check && p.joint_rand_len > 0), code, (const int32_t*)R0.status.p,
                       (const int32_t*)R1.status.p, msg, R0.jr_seed.as<uint32_t>(), R1.jr_seed.as<uint32_t>(), acc);
    HIPCHK(c, hipGetLastError());
    if (accept_out) HIPCHK(c, hipMemcpyAsync(accept_out, acc, n, hipMemcpyDeviceToHost, c->stream));
    if (decide_out) HIPCHK(c, hipMemcpyAsync(decide_out, code, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->bury();
    return 0;
}

// Fold of the out shares of the last prep_init of agg_id into dagg (device).
static int aggregate_impl(mastic_ctx* c, int agg_id, const uint8_t* valid, uint32_t* dagg) {
    Result& R = c->res[agg_id];
    const McParams& p = c->p;
    const size_t rows = (size_t)R.n_prefixes * (1 + p.output_len);
    const uint8_t* dv = nullptr;
    if (valid && R.n) {
        if (!c->agg_valid.grow(R.n)) return fail(c, MASTIC_ENOMEM, "out of device memory");
        HIPCHK(c, hipMemcpyAsync(c->agg_valid.p, valid, R.n, hipMemcpyHostToDevice, c->stream));
        dv = c->agg_valid.as<uint8_t>();
    }
    if (!rows) return 0;
    // few rows over many reports (a sweep level: ~700 rows x 1M reports):
    // split the reports into chunks so the grid fills the chip, then merge
    // the chunks' partial sums mod p (k_fold_shares)
    const size_t target = (size_t)c->k.n_cus * 16;
    size_t chunks = 1;
    if (rows < target && R.n >= 8192)
        chunks = std::min<size_t>({(target + rows - 1) / rows, R.n / 4096, (size_t)1024});
    // (an empty batch still writes its all-zero agg share: one chunk)
    const size_t chunk = chunks > 1 ? round_up((R.n + chunks - 1) / chunks, 256) : std::max<size_t>(R.n, 1);
    chunks = std::max<size_t>(1, (R.n + chunk - 1) / chunk);
    uint32_t* dst = dagg;
    if (chunks > 1) {
        if (!c->agg_part.ensure(std::max<size_t>(chunks * rows * p.w32 * 4, (size_t)1 << 20)))
            return fail(c, MASTIC_ENOMEM, "out of device memory");
        dst = c->agg_part.as<uint32_t>();
    }
    const dim3 grid((unsigned)rows, (unsigned)chunks);
    if (p.field == 64)
        hipLaunchKernelGGL(k_fold<F64>, grid, dim3(256), 0, c->stream, R.out.as<uint32_t>(), (int)R.n, (int)R.stride,
                           dv, (int)chunk, dst);
    else
        hipLaunchKernelGGL(k_fold<F128>, grid, dim3(256), 0, c->stream, R.out.as<uint32_t>(), (int)R.n, (int)R.stride,
                           dv, (int)chunk, dst);
    HIPCHK(c, hipGetLastError());
    if (chunks > 1) {
        const dim3 g2((unsigned)((rows + 255) / 256));
        if (p.field == 64)
            hipLaunchKernelGGL(k_fold_shares<F64>, g2, dim3(256), 0, c->stream, (const uint32_t*)dst, (int)chunks,
                               (int)rows, dagg);
        else
            hipLaunchKernelGGL(k_fold_shares<F128>, g2, dim3(256), 0, c->stream, (const uint32_t*)dst, (int)chunks,
                               (int)rows, dagg);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

extern "C" int mastic_aggregate(mastic_ctx* c, int agg_id, const uint8_t* valid, uint8_t* agg_share) {
    DeviceScope ds_(c);
    if (!c || (agg_id != 0 && agg_id != 1)) return fail(c, MASTIC_EINVAL, "invalid aggregator ID");
    Result& R = c->res[agg_id];
    if (!R.ready) return fail(c, MASTIC_EINVAL, "no prep_init result for this aggregator");
    const McParams& p = c->p;
    const size_t rows = (size_t)R.n_prefixes * (1 + p.output_len);
    if (!c->agg_out.grow(std::max<size_t>(rows, 1) * p.w32 * 4)) return fail(c, MASTIC_ENOMEM, "out of device memory");
    int rc = aggregate_impl(c, agg_id, valid, c->agg_out.as<uint32_t>());
    if (rc) return rc;
    if (agg_share && rows)
        HIPCHK(c, hipMemcpyAsync(agg_share, c->agg_out.p, rows * p.w32 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// (ABI 6: the only name of this function; mastic_aggregate_device, whose
// argument count changed between ABI 3, 4 and 5, is gone)
extern "C" int mastic_aggregate_device_on_stream(mastic_ctx* c, int agg_id, const uint8_t* valid,
                                                 void* dev_agg_share, void* caller_stream) {
    DeviceScope ds_(c);
    if (!c || (agg_id != 0 && agg_id != 1)) return fail(c, MASTIC_EINVAL, "invalid aggregator ID");
    Result& R = c->res[agg_id];
    if (!R.ready) return fail(c, MASTIC_EINVAL, "no prep_init result for this aggregator");
    const size_t rows = (size_t)R.n_prefixes * (1 + c->p.output_len);
    if (rows && !dev_agg_share) return fail(c, MASTIC_EINVAL, "null agg share buffer");
    // the buffer may have been allocated / filled by work queued on the
    // caller's stream (e.g. a torch allocation's fill): the fold writes it
    // only after that work, ordered by an event (no device-wide sync)
    if (!c->fold_ev) HIPCHK(c, hipEventCreateWithFlags(&c->fold_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->fold_ev, (hipStream_t)caller_stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->fold_ev, 0));
    int rc = aggregate_impl(c, agg_id, valid, (uint32_t*)dev_agg_share);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's stream (e.g. RCCL's) reads it next
    return 0;
}

// One agg share per batch bucket in one pass over the out shares.  Every
// decision (the id check, passes, copies, chunks, sizes) is group_fold.hpp's.
extern "C" int mastic_aggregate_grouped(mastic_ctx* c, int agg_id, const uint32_t* group, size_t n_groups,
                                        const uint8_t* valid, uint8_t* agg_shares, uint64_t* counts) {
    DeviceScope ds_(c);
    if (!c || (agg_id != 0 && agg_id != 1)) return fail(c, MASTIC_EINVAL, "invalid aggregator ID");
    Result& R = c->res[agg_id];
    if (!R.ready) return fail(c, MASTIC_EINVAL, "no prep_init result for this aggregator");
    const McParams& p = c->p;
    const size_t n = R.n;
    const size_t rows = (size_t)R.n_prefixes * (1 + p.output_len);
    if (n_groups == 0 || n_groups > MASTIC_MAX_GROUPS)
        return fail(c, MASTIC_EINVAL, "n_groups must be 1 .. %d", MASTIC_MAX_GROUPS);
    if (n_groups * rows > (size_t)INT_MAX) return fail(c, MASTIC_EINVAL, "n_groups * rows exceeds INT_MAX");
    if (n && !group) return fail(c, MASTIC_EINVAL, "null group ids");
    if (rows && !agg_shares) return fail(c, MASTIC_EINVAL, "null agg shares buffer");
    std::vector<uint64_t> cnt(n_groups);
    const long long bad = check_groups(group, n, n_groups, valid, cnt.data());
    if (bad >= 0)
        return fail(c, MASTIC_EINVAL, "report %lld: group id %u is not below n_groups = %zu", bad, group[bad], n_groups);
    const GroupFoldPlan pl = plan_group_fold(p.w32, n, rows, n_groups, c->k.n_cus, 0, 0);
    const size_t out_bytes = n_groups * rows * p.w32 * 4;
    if (rows) {
        // all device memory first (each allocation takes the fail_allocs hook):
        // nothing is launched before the last of them succeeded
        auto alloc = [&](DevBuf& b, size_t bytes) { return !c->inject_alloc_failure() && b.grow(bytes); };
        if ((n && !alloc(c->grp_ids, n * 4)) || (n && valid && !alloc(c->agg_valid, n)) ||
            (pl.partial_bytes && !alloc(c->grp_part, pl.partial_bytes)) || !alloc(c->grp_out, out_bytes))
            return fail(c, MASTIC_ENOMEM, "out of device memory (grouped fold)");
        uint32_t* stage = c->grp_out.as<uint32_t>();
        if (pl.chunks == 0) {
            HIPCHK(c, hipMemsetAsync(stage, 0, out_bytes, c->stream));
        } else {
            const uint8_t* dv = nullptr;
            HIPCHK(c, hipMemcpyAsync(c->grp_ids.p, group, n * 4, hipMemcpyHostToDevice, c->stream));
            if (valid) {
                HIPCHK(c, hipMemcpyAsync(c->agg_valid.p, valid, n, hipMemcpyHostToDevice, c->stream));
                dv = c->agg_valid.as<uint8_t>();
            }
            const dim3 grid(pl.grid_x, pl.grid_y);
            for (uint32_t k = 0; k < pl.passes; k++) {
                const uint32_t g0 = k * pl.groups_per_pass;
                const uint32_t gpp = std::min<uint32_t>(pl.groups_per_pass, (uint32_t)n_groups - g0);
                uint32_t* dst = stage + (size_t)g0 * rows * p.w32;
                uint32_t* part = pl.chunks > 1 ? c->grp_part.as<uint32_t>() : dst;
                if (p.field == 64)
                    hipLaunchKernelGGL(k_fold_grouped<F64>, grid, dim3(256), pl.lds_bytes, c->stream,
                                       R.out.as<uint32_t>(), (int)n, (int)R.stride, c->grp_ids.as<uint32_t>(), dv,
                                       (int)pl.chunk, g0, (int)gpp, (int)pl.copies, part);
                else
                    hipLaunchKernelGGL(k_fold_grouped<F128>, grid, dim3(256), pl.lds_bytes, c->stream,
                                       R.out.as<uint32_t>(), (int)n, (int)R.stride, c->grp_ids.as<uint32_t>(), dv,
                                       (int)pl.chunk, g0, (int)gpp, (int)pl.copies, part);
                HIPCHK(c, hipGetLastError());
                if (pl.chunks > 1) {
                    const size_t ne = (size_t)gpp * rows;
                    const dim3 g2((unsigned)((ne + 255) / 256));
                    if (p.field == 64)
                        hipLaunchKernelGGL(k_fold_shares<F64>, g2, dim3(256), 0, c->stream, (const uint32_t*)part,
                                           (int)pl.chunks, (int)ne, dst);
                    else
                        hipLaunchKernelGGL(k_fold_shares<F128>, g2, dim3(256), 0, c->stream, (const uint32_t*)part,
                                           (int)pl.chunks, (int)ne, dst);
                    HIPCHK(c, hipGetLastError());
                }
            }
        }
        HIPCHK(c, hipMemcpyAsync(agg_shares, stage, out_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (counts) std::copy(cnt.begin(), cnt.end(), counts);
    return 0;
}

extern "C" int mastic_fold_shares(mastic_ctx* c, const void* dev_shares, size_t n_shares, size_t n_elems,
                                  void* dev_out, void* producer_stream) {
    DeviceScope ds_(c);
    if (!c || (!dev_shares && n_shares) || !dev_out) return MASTIC_EINVAL;
    if (n_elems == 0) return 0;
    // the shares were written on the caller's stream (e.g. an RCCL all-gather):
    // order the fold after that stream's work with an event, not a device sync
    if (!c->fold_ev) HIPCHK(c, hipEventCreateWithFlags(&c->fold_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->fold_ev, (hipStream_t)producer_stream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->fold_ev, 0));
    const dim3 grid((unsigned)((n_elems + 255) / 256));
    if (c->p.field == 64)
        hipLaunchKernelGGL(k_fold_shares<F64>, grid, dim3(256), 0, c->stream, (const uint32_t*)dev_shares,
                           (int)n_shares, (int)n_elems, (uint32_t*)dev_out);
    else
        hipLaunchKernelGGL(k_fold_shares<F128>, grid, dim3(256), 0, c->stream, (const uint32_t*)dev_shares,
                           (int)n_shares, (int)n_elems, (uint32_t*)dev_out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---- multi-GPU merge over the ctx's own RCCL communicator --
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

// ctx teardown: its queued work is waited for, then the communicator is
// released locally (ncclCommAbort never waits on peers that may be gone).
void mastic_ctx::comm_release() {
    (void)hipStreamSynchronize(stream);
    (void)rccl().CommAbort(comm);
    comm = nullptr;
}

// Abort the ctx's communicator after a failed or timed-out RCCL step: its
// kernels see the abort flag and exit, the ctx keeps comm_broken so later
// collective calls fail instead of silently folding as world 1.
// MASTIC_TRACE_COMM: mark step i of the agreement round on the ctx's stream;
// a timed-out wait reports which marks the stream has passed.
static void comm_mark(mastic_ctx* c, int i) {
    if (!trace_comm()) return;
    if (!c->comm_marks[i] && hipEventCreateWithFlags(&c->comm_marks[i], hipEventDisableTiming) != hipSuccess) return;
    (void)hipEventRecord(c->comm_marks[i], c->stream);
}
static void comm_marks_report(mastic_ctx* c) {
    if (!trace_comm()) return;
    for (int i = 0; i < 3; i++)
        if (c->comm_marks[i])
            fprintf(stderr, "[mastic comm]   mark %d (%s): %s\n", i,
                    (const char*[]){"status uploaded", "status all-gather queued", "status download queued"}[i],
                    hipEventQuery(c->comm_marks[i]) == hipSuccess ? "passed" : "not passed");
}

static int comm_abort(mastic_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (trace_comm()) fprintf(stderr, "[mastic comm] abort: %s\n", buf);
    if (c->comm) {
        const ncclResult_t r = rccl().CommAbort(c->comm);
        if (trace_comm()) fprintf(stderr, "[mastic comm] ncclCommAbort -> %d\n", (int)r);
    }
    c->comm = nullptr;
    c->comm_broken = true;
    return fail(c, code, "%s; the communicator was aborted", buf);
}

// The result of an RCCL call on the ctx's communicator; a call that reports
// ncclInProgress (a non-blocking communicator's) is polled until it settles,
// within the ctx's timeout.
static int comm_settle(mastic_ctx* c, ncclResult_t r, const char* what) {
    const double t0 = now_ms();
    while (r == ncclInProgress) {
        if (now_ms() - t0 > c->comm_timeout_ms)
            return comm_abort(c, MASTIC_ETIMEDOUT, "RCCL %s did not complete within %d ms", what, c->comm_timeout_ms);
        std::this_thread::yield();
        ncclResult_t st = ncclSuccess;
        const ncclResult_t q = rccl().CommGetAsyncError(c->comm, &st);
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
        if (rccl().CommGetAsyncError(c->comm, &st) == ncclSuccess && st != ncclSuccess && st != ncclInProgress)
            return comm_abort(c, MASTIC_EHIP, "RCCL %s: %s", what, rccl().GetErrorString(st));
        if (now_ms() - t0 > c->comm_timeout_ms) {
            comm_marks_report(c);
            return comm_abort(c, MASTIC_ETIMEDOUT, "%s: a peer rank did not join within %d ms", what,
                              c->comm_timeout_ms);
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
    if (!c->comm) {
        if (c->comm_broken && !local_rc)
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
    CommStatus* h = (CommStatus*)c->comm_st_host;  // [0]: this rank's record, [1 + r]: rank r's
    h[0] = CommStatus{local_rc, op, (uint64_t)n_local, (uint64_t)n_elems, COMM_MAGIC, 0};
    uint8_t* d = c->comm_st.as<uint8_t>();
    hipError_t e = hipMemcpyAsync(d, h, sizeof(CommStatus), hipMemcpyHostToDevice, c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return comm_abort(c, local_rc ? local_rc : MASTIC_EHIP, "%s: status upload: %s", comm_op_name(op),
                          hipGetErrorString(e));
    }
    comm_mark(c, 0);
    int rc = comm_settle(c, rccl().AllGather(d, d + sizeof(CommStatus), sizeof(CommStatus), ncclUint8, c->comm,
                                             c->stream), "status all-gather");
    if (rc) return local_rc ? local_rc : rc;
    comm_mark(c, 1);
    e = hipMemcpyAsync(h + 1, d + sizeof(CommStatus), sizeof(CommStatus) * (size_t)c->comm_n, hipMemcpyDeviceToHost,
                       c->stream);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return comm_abort(c, local_rc ? local_rc : MASTIC_EHIP, "%s: status download: %s", comm_op_name(op),
                          hipGetErrorString(e));
    }
    comm_mark(c, 2);
    rc = comm_wait(c, "status all-gather");
    if (rc) return local_rc ? local_rc : rc;
    const CommVerdict v = comm_decide(h + 1, c->comm_n, op, n_local, n_elems);
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
    return !c->comm || comm_grow(c, c->comm_gather, std::max<size_t>(n_local * n_elems * c->p.w32 * 4, 4) * c->comm_n);
}

// dev_out = sum mod p of the n_local shares of every rank (n_elems elements
// each), queued on c->stream after a successful agreement: one ncclAllGather
// of this rank's shares into the rank-ordered comm_gather, then
// k_fold_shares over the n_local x nranks shares (RCCL's integer sum is not
// GF(p) addition).  Without a communicator the local shares are folded
// directly (world 1).
static int allgather_fold_impl(mastic_ctx* c, const uint32_t* local, size_t n_local, size_t n_elems, uint32_t* out) {
    const size_t local_bytes = n_local * n_elems * c->p.w32 * 4;
    const uint32_t* src = local;
    size_t n_shares = n_local;
    if (c->comm && local_bytes) {
        int rc = comm_settle(c, rccl().AllGather(local, c->comm_gather.p, local_bytes, ncclUint8, c->comm, c->stream),
                             "share all-gather");
        if (rc) return rc;
        src = c->comm_gather.as<uint32_t>();
        n_shares = n_local * (size_t)c->comm_n;
    }
    const dim3 grid((unsigned)((n_elems + 255) / 256));
    if (c->p.field == 64)
        hipLaunchKernelGGL(k_fold_shares<F64>, grid, dim3(256), 0, c->stream, src, (int)n_shares, (int)n_elems, out);
    else
        hipLaunchKernelGGL(k_fold_shares<F128>, grid, dim3(256), 0, c->stream, src, (int)n_shares, (int)n_elems, out);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// The end of a collective call: its queued work (the data all-gather, the
// fold, the copy out) done, bounded by the timeout when RCCL is in it.
static int comm_finish(mastic_ctx* c, uint32_t op) {
    if (c->comm) return comm_wait(c, comm_op_name(op));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// The merged share to the caller's host buffer, AFTER comm_finish: a copy to
// pageable memory is synchronous, so queued behind a data all-gather that a
// dead peer never completes it would block this thread past every bound
// (found by tests/test_gpu_comm_nrank.py: a peer lost between the agreement
// round and the data all-gather).
static int comm_copy_out(mastic_ctx* c, void* host_out, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(host_out, c->comm_out.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// Shape limits of the fold kernel (k_fold_shares takes int counts).
static int comm_check_counts(mastic_ctx* c, size_t n_local, size_t n_elems) {
    if (n_local * (size_t)c->comm_n > (size_t)INT32_MAX || n_elems > (size_t)INT32_MAX)
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
    if (c->comm) return fail(c, MASTIC_EINVAL, "the ctx already has a communicator");
    if (!rccl().ok) return fail(c, MASTIC_ENODEV, "RCCL is not available: %s", rccl().why.c_str());
    c->comm_timeout_ms = timeout_ms > 0 ? timeout_ms : MASTIC_COMM_TIMEOUT_MS;
    // the agreement round's buffers, before joining: a rank that cannot
    // allocate them fails here, before any collective
    const size_t st_bytes = sizeof(CommStatus) * ((size_t)nranks + 1);
    if (!c->comm_st.ensure(st_bytes)) return fail(c, MASTIC_ENOMEM, "out of device memory");
    if (c->comm_st_host_n < (size_t)nranks + 1) {
        if (c->comm_st_host) (void)hipHostFree(c->comm_st_host);
        c->comm_st_host = nullptr;
        c->comm_st_host_n = 0;
        HIPCHK(c, hipHostMalloc(&c->comm_st_host, st_bytes, hipHostMallocDefault));
        c->comm_st_host_n = (size_t)nranks + 1;
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
    if (!job->cv.wait_for(lk, std::chrono::milliseconds(c->comm_timeout_ms), [&] { return job->done; })) {
        job->abandoned = true;
        if (trace_comm()) fprintf(stderr, "[mastic comm] init of rank %d of %d timed out\n", rank, nranks);
        return fail(c, MASTIC_ETIMEDOUT,
                    "RCCL init: not every rank joined within %d ms (the pending init is abandoned; the ctx stays "
                    "world 1)", c->comm_timeout_ms);
    }
    if (trace_comm()) fprintf(stderr, "[mastic comm] ncclCommInitRank(%d of %d) -> %d\n", rank, nranks, (int)job->r);
    if (job->dev_err != hipSuccess) return fail(c, MASTIC_EHIP, "hipSetDevice: %s", hipGetErrorString(job->dev_err));
    if (job->r != ncclSuccess) {
        if (job->comm) (void)rccl().CommAbort(job->comm);
        return fail(c, MASTIC_EHIP, "RCCL init: %s", rccl().GetErrorString(job->r));
    }
    c->comm = job->comm;
    c->comm_n = nranks;
    c->comm_rank = rank;
    c->comm_broken = false;
    return 0;
}

extern "C" int mastic_comm_init(mastic_ctx* c, int nranks, int rank, const uint8_t id[MASTIC_COMM_ID_BYTES]) {
    return mastic_comm_init_timeout(c, nranks, rank, id, MASTIC_COMM_TIMEOUT_MS);
}

extern "C" int mastic_comm_info(const mastic_ctx* c, int* nranks, int* rank) {
    if (!c) return MASTIC_EINVAL;
    if (nranks) *nranks = c->comm_n;
    if (rank) *rank = c->comm_rank;
    return 0;
}

extern "C" int mastic_comm_destroy(mastic_ctx* c) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    int rc = 0;
    if (c->comm) {
        rc = comm_wait(c, "mastic_comm_destroy");
        if (!rc) rc = comm_settle(c, rccl().CommFinalize(c->comm), "finalize");
        if (!rc) {
            const ncclResult_t r = rccl().CommDestroy(c->comm);
            if (r != ncclSuccess) rc = fail(c, MASTIC_EHIP, "RCCL destroy: %s", rccl().GetErrorString(r));
        }
    }
    c->comm = nullptr;
    c->comm_n = 1;
    c->comm_rank = 0;
    c->comm_broken = false;
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
        (!comm_grow(c, c->comm_local, std::max<size_t>(n_local, 1) * n_elems * ebytes) ||
         !comm_grow(c, c->comm_out, n_elems * ebytes) || !comm_stage_gather(c, n_local, n_elems)))
        rc = fail(c, MASTIC_ENOMEM, "out of device memory");
    if (!rc && n_elems && n_local &&
        hipMemcpyAsync(c->comm_local.p, host_local, n_local * n_elems * ebytes, hipMemcpyHostToDevice, c->stream) !=
            hipSuccess)
        rc = fail(c, MASTIC_EHIP, "share upload failed");
    rc = comm_agree(c, rc, COMM_MERGE_HOST, n_local, n_elems);
    if (rc || n_elems == 0) return rc;
    rc = allgather_fold_impl(c, c->comm_local.as<uint32_t>(), n_local, n_elems, c->comm_out.as<uint32_t>());
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
        else if ((size_t)R.n_prefixes * (1 + c->p.output_len) != n_elems)
            rc = fail(c, MASTIC_EINVAL, "agg share length does not match the last prep_init");
    }
    if (!rc && n_elems &&
        (!comm_grow(c, c->comm_local, n_local * n_elems * ebytes) || !comm_grow(c, c->comm_out, n_elems * ebytes) ||
         !comm_stage_gather(c, n_local, n_elems)))
        rc = fail(c, MASTIC_ENOMEM, "out of device memory");
    size_t k = 0;
    for (int a = 0; a < 2 && !rc && n_elems; a++) {
        if (!((agg_mask >> a) & 1)) continue;
        uint32_t* dst = (uint32_t*)((uint8_t*)c->comm_local.p + k++ * n_elems * ebytes);
        if (!zeros)
            rc = aggregate_impl(c, a, valid, dst);
        else if (hipMemsetAsync(dst, 0, n_elems * ebytes, c->stream) != hipSuccess)  // no reports here: agg_init's zeros
            rc = fail(c, MASTIC_EHIP, "hipMemsetAsync failed");
    }
    rc = comm_agree(c, rc, COMM_AGGREGATE_MERGED, n_local, n_elems);
    if (rc || n_elems == 0) return rc;
    rc = allgather_fold_impl(c, c->comm_local.as<uint32_t>(), n_local, n_elems, c->comm_out.as<uint32_t>());
    if (!rc) rc = comm_finish(c, COMM_AGGREGATE_MERGED);
    if (rc) return rc;
    return comm_copy_out(c, agg_out, n_elems * ebytes);
}

// Eval-proof Merkle tree (proof-aggregation mode, kernels.hpp k_proof_tree_*)
// over the last prep_init result of agg_id.
extern "C" int mastic_proof_tree(mastic_ctx* c, int agg_id, const uint8_t* app_ctx, size_t ctx_len,
                                 uint8_t* nodes_out, size_t n_nodes) {
    DeviceScope ds_(c);
    if (!c || (agg_id != 0 && agg_id != 1)) return fail(c, MASTIC_EINVAL, "invalid aggregator ID");
    Result& R = c->res[agg_id];
    if (!R.ready) return fail(c, MASTIC_EINVAL, "no prep_init result for this aggregator");
    const size_t n = R.n;
    size_t total = 0;
    for (size_t m = n; m > 0; m = (m == 1) ? 0 : (m + 1) / 2) total += m;
    if (n_nodes != total) return fail(c, MASTIC_EINVAL, "proof tree has incorrect size");
    if (n == 0) return 0;
    if (n > (size_t)INT32_MAX / 2) return fail(c, MASTIC_EINVAL, "batch too large for a proof tree");
    int rc = build_prefixes(c, app_ctx, ctx_len, nullptr, 0);
    if (rc) return rc;
    DevBuf nodes;
    if (!nodes.ensure(total * 32)) return fail(c, MASTIC_ENOMEM, "out of device memory (proof tree)");
    uint32_t* d = nodes.as<uint32_t>();
    hipLaunchKernelGGL(k_proof_tree_leaves, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       R.eval_proof.as<uint32_t>(), (int)n, (int)R.stride, d);
    size_t off = 0;
    for (size_t m = n; m > 1; m = (m + 1) / 2) {
        const size_t mo = (m + 1) / 2;
        hipLaunchKernelGGL(k_proof_tree_level, dim3((unsigned)((mo + 255) / 256)), dim3(256), 0, c->stream,
                           (const PrefixState*)c->pfx.p, d + off * 8, (int)m, d + (off + m) * 8);
        off += m;
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(nodes_out, d, total * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int mastic_synchronize(mastic_ctx* c) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->bury();
    return 0;
}

extern "C" int mastic_last_timing(mastic_ctx* c, double* eval_ms, int* eval_launches, double* absorb_ms,
                                  int* absorb_launches, double* total_ms) {
    return mastic_last_timing3(c, eval_ms, eval_launches, nullptr, nullptr, absorb_ms, absorb_launches, total_ms);
}

extern "C" int mastic_last_timing3(mastic_ctx* c, double* aes_ms, int* aes_launches, double* proof_ms,
                                   int* proof_launches, double* absorb_ms, int* absorb_launches, double* total_ms) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->tm[c->tcur].n_eval < 0) {
        // some timing marks sit on the sponge streams without the main stream
        // waiting for them (a single-chunk hit's empty sponge marks, recorded
        // on the sponge stream while its sponges run on the main stream):
        // wait for the marks themselves (an unwaited mark gave "device not
        // ready" in a 4-rank run sharing one GPU)
        for (int i = 0; i < -c->tm[c->tcur].n_eval; i++) HIPCHK(c, hipEventSynchronize(c->tm[c->tcur].ev[i]));
        // events: [t0, t1] then per level [aes0, aes1, proof0, proof1, absorb0, absorb1]
        const size_t evi = (size_t)(-c->tm[c->tcur].n_eval);
        double ta = 0, tp = 0, tb = 0;
        int n = 0;
        float ms = 0;
        for (size_t i = 2; i + 6 <= evi; i += 6) {
            HIPCHK(c, hipEventElapsedTime(&ms, c->tm[c->tcur].ev[i], c->tm[c->tcur].ev[i + 1]));
            ta += ms;
            HIPCHK(c, hipEventElapsedTime(&ms, c->tm[c->tcur].ev[i + 2], c->tm[c->tcur].ev[i + 3]));
            tp += ms;
            HIPCHK(c, hipEventElapsedTime(&ms, c->tm[c->tcur].ev[i + 4], c->tm[c->tcur].ev[i + 5]));
            tb += ms;
            n++;
        }
        HIPCHK(c, hipEventElapsedTime(&ms, c->tm[c->tcur].ev[0], c->tm[c->tcur].ev[1]));
        c->tm[c->tcur].t_total = ms;
        c->tm[c->tcur].t_eval = ta;
        c->tm[c->tcur].t_proof = tp;
        c->tm[c->tcur].t_absorb = tb;
        c->tm[c->tcur].n_eval = n;
        c->tm[c->tcur].n_absorb = n;
    }
    if (aes_ms) *aes_ms = c->tm[c->tcur].t_eval;
    if (aes_launches) *aes_launches = c->tm[c->tcur].n_eval;
    if (proof_ms) *proof_ms = c->tm[c->tcur].t_proof;
    if (proof_launches) *proof_launches = c->tm[c->tcur].n_absorb;
    if (absorb_ms) *absorb_ms = c->tm[c->tcur].t_absorb;
    if (absorb_launches) *absorb_launches = c->tm[c->tcur].n_absorb;
    if (total_ms) *total_ms = c->tm[c->tcur].t_total;
    return 0;
}

extern "C" int mastic_tree_stats(mastic_ctx* c, const uint8_t* enc, size_t len, uint64_t* nodes, uint64_t* interior,
                                 uint64_t* max_level_nodes) {
    DeviceScope ds_(c);
    Tree* t = nullptr;
    int rc = build_tree(c, enc, len, &t);
    if (rc) return rc;
    if (nodes) *nodes = t->nodes;
    if (interior) *interior = t->interior;
    if (max_level_nodes) *max_level_nodes = (uint64_t)t->max_level_nodes;
    return 0;
}

extern "C" int mastic_work_bytes(mastic_ctx* c, const uint8_t* enc, size_t len, uint64_t* per_report) {
    DeviceScope ds_(c);
    Tree* t = nullptr;
    int rc = build_tree(c, enc, len, &t);
    if (rc) return rc;
    if (per_report) *per_report = (uint64_t)work_layout(c->p, t).words * 4;
    return 0;
}

extern "C" int mastic_prep_init_batch(mastic_ctx* c, const uint8_t* verify_key, size_t vk_len, const uint8_t* app_ctx,
                                      size_t ctx_len, int agg_id, const uint8_t* enc_agg_param, size_t agg_param_len,
                                      size_t n, const uint8_t* nonces, const uint8_t* public_shares,
                                      const uint8_t* input_shares, uint8_t* prep_shares_out, uint8_t* jr_seeds_out,
                                      uint8_t* out_shares_out, int32_t* status_out) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    if (agg_id != 0 && agg_id != 1) return fail(c, MASTIC_EINVAL, "invalid aggregator ID");
    mastic_reports* rep = nullptr;
    int rc = mastic_reports_create(c, n, &rep);
    if (rc) return rc;
    rc = mastic_reports_upload(rep, nonces, public_shares, agg_id == 0 ? input_shares : nullptr,
                               agg_id == 1 ? input_shares : nullptr);
    if (!rc) rc = mastic_prep_init(c, rep, verify_key, vk_len, app_ctx, ctx_len, agg_id, enc_agg_param, agg_param_len);
    if (!rc) rc = mastic_prep_result(c, agg_id, prep_shares_out, jr_seeds_out, out_shares_out, status_out);
    mastic_reports_destroy(rep);
    return rc;
}

// ---------------------------------------------------------------- decide
extern "C" int mastic_decide_batch(mastic_ctx* c, const uint8_t* app_ctx, size_t ctx_len, const uint8_t* enc,
                                   size_t len, size_t n, const uint8_t* ps0, const uint8_t* ps1, uint8_t* msgs_out,
                                   uint8_t* valid_out) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    Tree* t = nullptr;
    int rc = build_tree(c, enc, len, &t);
    if (rc) return rc;
    if (n == 0) return 0;
    if ((rc = build_prefixes(c, app_ctx, ctx_len, nullptr, 0))) return rc;
    const McParams& p = c->p;
    const size_t psz = mc_prep_share_size(p, t->weight_check);
    const size_t stride = round_up(n, 64);
    DevBuf a, b, ver, msg, st;
    if (!a.ensure(psz * n) || !b.ensure(psz * n) || !ver.ensure(stride * 4 * (size_t)p.verifier_len * p.w32) ||
        !msg.ensure(32 * n) || !st.ensure(n))
        return fail(c, MASTIC_ENOMEM, "out of device memory (decide)");
    HIPCHK(c, hipMemcpyAsync(a.p, ps0, psz * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.p, ps1, psz * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(msg.p, 0, 32 * n, c->stream));
    if (p.field == 64)
        hipLaunchKernelGGL(k_decide<F64>, dim3((n + 255) / 256), dim3(256), 0, c->stream, p, (int)n, (int)stride,
                           (int)t->weight_check, a.as<uint8_t>(), b.as<uint8_t>(), (int)psz, ver.as<uint32_t>(),
                           (const PrefixState*)c->pfx.p, msg.as<uint8_t>(), st.as<uint8_t>());
    else
        hipLaunchKernelGGL(k_decide<F128>, dim3((n + 255) / 256), dim3(256), 0, c->stream, p, (int)n, (int)stride,
                           (int)t->weight_check, a.as<uint8_t>(), b.as<uint8_t>(), (int)psz, ver.as<uint32_t>(),
                           (const PrefixState*)c->pfx.p, msg.as<uint8_t>(), st.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    if (msgs_out && t->weight_check && p.joint_rand_len > 0)
        HIPCHK(c, hipMemcpyAsync(msgs_out, msg.p, 32 * n, hipMemcpyDeviceToHost, c->stream));
    if (valid_out) HIPCHK(c, hipMemcpyAsync(valid_out, st.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// ---------------------------------------------------------------- reports
extern "C" int mastic_reports_create(mastic_ctx* c, size_t n, mastic_reports** out) {
    DeviceScope ds_(c);
    if (!c || !out) return MASTIC_EINVAL;
    mastic_reports* r = new mastic_reports();
    r->ctx = c;
    r->n = n;
    const McParams& p = c->p;
    if (!r->nonces.ensure(16 * n) || !r->pub.ensure((size_t)mc_public_share_size(p) * n) || !r->wire_flags.ensure(n)) {
        delete r;
        return fail(c, MASTIC_ENOMEM, "out of device memory (reports)");
    }
    // (null stream, like the blocking copies of upload / shard that follow it there and are done before
    // the first kernel that touches the flags is queued on the ctx's stream)
    if (hipMemset(r->wire_flags.p, 0, r->wire_flags.bytes) != hipSuccess) {
        delete r;
        return fail(c, MASTIC_EHIP, "reports: clearing the wire flags failed");
    }
    *out = r;
    return 0;
}

extern "C" int mastic_reports_view(mastic_reports* rep, size_t first, size_t count, mastic_reports** out) {
    DeviceScope ds_(rep ? rep->ctx : nullptr);
    if (!rep || !out) return MASTIC_EINVAL;
    mastic_ctx* c = rep->ctx;
    if (first > rep->n || count > rep->n - first) return fail(c, MASTIC_EINVAL, "view out of range");
    const McParams& p = c->p;
    mastic_reports* r = new mastic_reports();
    r->ctx = c;
    r->n = count;
    r->gen = rep->gen;  // one contents generation for the batch and all its views
    const size_t ps = mc_public_share_size(p), i0 = mc_input_share_size(p, 0), i1 = mc_input_share_size(p, 1);
    r->nonces.view(rep->nonces, 16 * first, 16 * count);
    r->pub.view(rep->pub, ps * first, ps * count);
    r->in0.view(rep->in0, i0 * first, i0 * count);
    r->in1.view(rep->in1, i1 * first, i1 * count);
    r->wire_flags.view(rep->wire_flags, first, count);
    *out = r;
    return 0;
}

extern "C" void mastic_reports_destroy(mastic_reports* r) {
    DeviceScope ds_(r ? r->ctx : nullptr);
    delete r;
}
extern "C" size_t mastic_reports_count(const mastic_reports* r) { return r ? r->n : 0; }

// Range check of the wire field elements of the segments just written (pub:
// the public shares, in0: the leader input shares), queued on the ctx's
// stream ahead of any prep_init over the batch.
static int validate_wire(mastic_ctx* c, mastic_reports* r, bool pub, bool in0) {
    if (r->n == 0 || (!pub && !in0)) return 0;
    const dim3 grid((unsigned)((r->n + 3) / 4));
    const uint8_t* dp = pub ? r->pub.as<uint8_t>() : nullptr;
    const uint8_t* di = in0 ? r->in0.as<uint8_t>() : nullptr;
    if (c->p.field == 64)
        hipLaunchKernelGGL(k_validate_wire<F64>, grid, dim3(256), 0, c->stream, c->p, (int)r->n, dp, di,
                           r->wire_flags.as<uint8_t>());
    else
        hipLaunchKernelGGL(k_validate_wire<F128>, grid, dim3(256), 0, c->stream, c->p, (int)r->n, dp, di,
                           r->wire_flags.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int mastic_reports_upload(mastic_reports* r, const uint8_t* nonces, const uint8_t* pub,
                                     const uint8_t* in0, const uint8_t* in1) {
    DeviceScope ds_(r ? r->ctx : nullptr);
    if (!r) return MASTIC_EINVAL;
    mastic_ctx* c = r->ctx;
    const McParams& p = c->p;
    const size_t n = r->n;
    r->touch();
    if (nonces) HIPCHK(c, hipMemcpy(r->nonces.p, nonces, 16 * n, hipMemcpyHostToDevice));
    if (pub) HIPCHK(c, hipMemcpy(r->pub.p, pub, (size_t)mc_public_share_size(p) * n, hipMemcpyHostToDevice));
    if (in0) {
        if (!r->in0.ensure((size_t)mc_input_share_size(p, 0) * n)) return fail(c, MASTIC_ENOMEM, "out of device memory");
        HIPCHK(c, hipMemcpy(r->in0.p, in0, (size_t)mc_input_share_size(p, 0) * n, hipMemcpyHostToDevice));
    }
    if (in1) {
        if (!r->in1.ensure((size_t)mc_input_share_size(p, 1) * n)) return fail(c, MASTIC_ENOMEM, "out of device memory");
        HIPCHK(c, hipMemcpy(r->in1.p, in1, (size_t)mc_input_share_size(p, 1) * n, hipMemcpyHostToDevice));
    }
    return validate_wire(c, r, pub != nullptr, in0 != nullptr);
}

extern "C" int mastic_reports_download(mastic_reports* r, uint8_t* nonces, uint8_t* pub, uint8_t* in0, uint8_t* in1) {
    DeviceScope ds_(r ? r->ctx : nullptr);
    if (!r) return MASTIC_EINVAL;
    mastic_ctx* c = r->ctx;
    const McParams& p = c->p;
    const size_t n = r->n;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nonces) HIPCHK(c, hipMemcpy(nonces, r->nonces.p, 16 * n, hipMemcpyDeviceToHost));
    if (pub) HIPCHK(c, hipMemcpy(pub, r->pub.p, (size_t)mc_public_share_size(p) * n, hipMemcpyDeviceToHost));
    if (in0) {
        if (!r->in0.p) return fail(c, MASTIC_EINVAL, "no leader input shares");
        HIPCHK(c, hipMemcpy(in0, r->in0.p, (size_t)mc_input_share_size(p, 0) * n, hipMemcpyDeviceToHost));
    }
    if (in1) {
        if (!r->in1.p) return fail(c, MASTIC_EINVAL, "no helper input shares");
        HIPCHK(c, hipMemcpy(in1, r->in1.p, (size_t)mc_input_share_size(p, 1) * n, hipMemcpyDeviceToHost));
    }
    return 0;
}

template <class F>
static int shard_impl(mastic_ctx* c, mastic_reports* rep, const uint8_t* alphas, const uint8_t* betas,
                      const uint8_t* nonces, const uint8_t* rands) {
    typedef typename F::E E;
    const McParams& p = c->p;
    const size_t n = rep->n;
    const size_t ab = (p.bits + 7) / 8, bsz = (size_t)p.meas_len * p.enc, rs = mc_rand_size(p);
    if (!rep->in0.ensure((size_t)mc_input_share_size(p, 0) * n) || !rep->in1.ensure((size_t)mc_input_share_size(p, 1) * n))
        return fail(c, MASTIC_ENOMEM, "out of device memory (input shares)");
    DevBuf da, db, dr, tab;
    if (!da.ensure(ab * n) || !db.ensure(bsz * n) || !dr.ensure(rs * n) || !tab.ensure(sizeof(E) * p.P))
        return fail(c, MASTIC_ENOMEM, "out of device memory (shard inputs)");
    HIPCHK(c, hipMemcpy(da.p, alphas, ab * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(db.p, betas, bsz * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dr.p, rands, rs * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(rep->nonces.p, nonces, 16 * n, hipMemcpyHostToDevice));
    FlpConsts<F> fc = flp_consts<F>(p);
    const std::vector<E> pows = flp_alpha_inv_pows<F>(fc, p.P);
    HIPCHK(c, hipMemcpy(tab.p, pows.data(), sizeof(E) * p.P, hipMemcpyHostToDevice));
    // scratch planes per report
    const size_t wl = (size_t)p.value_len * p.w32;
    const size_t words = wl + 88 + 2 * wl + (size_t)std::max(1, p.joint_rand_len) * p.w32 + (size_t)p.arity * p.w32 +
                         2 * (size_t)p.arity * p.P * p.w32 + 2 * (size_t)p.proof_len * p.w32 + 32;
    const uint64_t budget = default_budget(c);
    size_t chunk = std::min<size_t>(round_up(n, 64), std::max<size_t>(64, (budget / (words * 4)) / 64 * 64));
    // the scratch is the ctx's work arena (kept across calls, stream-ordered
    // after earlier prep_inits): sharding a large batch leaves the arena that
    // its prep_inits then reuse instead of freeing it and allocating again
    // (large hipMallocs / hipFrees cost ~1 s per 50-100 GB on MI355X)
    DevBuf& scratch = c->work;
    c->rk.valid = false;  // the scratch overwrites the arena's key-schedule planes
    if (!scratch.ensure(words * 4 * chunk)) return fail(c, MASTIC_ENOMEM, "out of device memory (shard scratch)");
    for (size_t b = 0; b < n; b += chunk) {
        const int nn = (int)std::min(chunk, n - b);
        const int S = (int)round_up(nn, 64);
        ShardArgs a;
        a.n = nn;
        a.stride = S;
        a.alphas = da.as<uint8_t>() + ab * b;
        a.betas = db.as<uint8_t>() + bsz * b;
        a.nonces = rep->nonces.as<uint8_t>() + 16 * b;
        a.rands = dr.as<uint8_t>() + rs * b;
        a.pub = rep->pub.as<uint8_t>() + (size_t)mc_public_share_size(p) * b;
        a.in0 = rep->in0.as<uint8_t>() + (size_t)mc_input_share_size(p, 0) * b;
        a.in1 = rep->in1.as<uint8_t>() + (size_t)mc_input_share_size(p, 1) * b;
        uint32_t* w = scratch.as<uint32_t>();
        size_t o = 0;
        auto take = [&](size_t k) {
            uint32_t* r = w + o * S;
            o += k;
            return r;
        };
        a.beta = take(wl);
        a.rke = take(44);
        a.rkc = take(44);
        a.bs = take(2 * wl);
        a.jr = take((size_t)std::max(1, p.joint_rand_len) * p.w32);
        a.prand = take((size_t)p.arity * p.w32);
        a.vals = take((size_t)p.arity * p.P * p.w32);
        a.coef = take((size_t)p.arity * p.P * p.w32);
        a.proof = take((size_t)p.proof_len * p.w32);
        a.hps = take((size_t)p.proof_len * p.w32);
        a.misc = take(32);
        hipLaunchKernelGGL(k_shard<F>, dim3((nn + 255) / 256), dim3(256), 0, c->stream, p, a,
                           (const PrefixState*)c->pfx.p, fc, tab.as<E>());
        HIPCHK(c, hipGetLastError());
    }
    if (int rc = validate_wire(c, rep, true, true)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int mastic_reports_shard(mastic_reports* rep, const uint8_t* app_ctx, size_t ctx_len,
                                    const uint8_t* alphas, const uint8_t* betas, const uint8_t* nonces,
                                    const uint8_t* rands) {
    DeviceScope ds_(rep ? rep->ctx : nullptr);
    if (!rep) return MASTIC_EINVAL;
    mastic_ctx* c = rep->ctx;
    rep->touch();
    if (rep->n == 0) {
        // an empty batch holds both aggregators' (zero) input shares, so that
        // prep_init accepts it and its views (e.g. a rank of a split job that
        // gets no reports)
        if (!rep->in0.ensure(0) || !rep->in1.ensure(0)) return fail(c, MASTIC_ENOMEM, "out of device memory");
        return 0;
    }
    if (!alphas || !nonces || !rands || (!betas && c->p.meas_len > 0)) return fail(c, MASTIC_EINVAL, "null input");
    int rc = build_prefixes(c, app_ctx, ctx_len, nullptr, 0);
    if (rc) return rc;
    return c->p.field == 64 ? shard_impl<F64>(c, rep, alphas, betas, nonces, rands)
                            : shard_impl<F128>(c, rep, alphas, betas, nonces, rands);
}

extern "C" int mastic_shard_batch(mastic_ctx* c, const uint8_t* app_ctx, size_t ctx_len, size_t n,
                                  const uint8_t* alphas, const uint8_t* betas, const uint8_t* nonces,
                                  const uint8_t* rands, uint8_t* pub_out, uint8_t* in0_out, uint8_t* in1_out) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    mastic_reports* rep = nullptr;
    int rc = mastic_reports_create(c, n, &rep);
    if (rc) return rc;
    rc = mastic_reports_shard(rep, app_ctx, ctx_len, alphas, betas, nonces, rands);
    if (!rc) rc = mastic_reports_download(rep, nullptr, pub_out, in0_out, in1_out);
    mastic_reports_destroy(rep);
    return rc;
}

// ---------------------------------------------------------------- compaction
// mastic_reports_compact: the plan is compact_plan.hpp, the kernel
// rows_kernels.hpp.  Everything runs on the ctx's main stream.  That orders it
// after every queued reader of the batch's buffers, because all of them run
// there: k_unpack, k_rows_to_planes and k_validate_wire (Chunk::unpack and
// validate_wire launch on c->stream whatever stream the chunk's sponges use),
// k_shard and the replay set's kernels.  Streams 2 to 4 run binder sponges and
// the FLP query, which read the work arena only, so no event is needed.
static int compact_segment(mastic_ctx* c, uint8_t* seg, size_t rb, const CompactIndex& ix, const uint32_t* d_idx,
                           uint8_t* stage, size_t stage_bytes) {
    const size_t S = compact_stage_rows(stage_bytes, rb);
    for (const CompactLaunch& l : compact_launches(ix, S)) {
        if (l.op == CP_COPY_BACK) {
            HIPCHK(c, hipMemcpyAsync(seg + l.first * rb, stage, l.count * rb, hipMemcpyDeviceToDevice, c->stream));
            continue;
        }
        uint8_t* dst = l.op == CP_GATHER_STAGE ? stage : seg + l.first * rb;
        // (one launch's grid.x is bounded; a tile above it goes out in pieces, in order)
        const size_t piece = std::max<size_t>(1, (size_t)(ROWS_MAX_GRID * ROWS_THREADS / rows_slots_per_row(rb)));
        for (size_t o = 0; o < l.count; o += piece) {
            const size_t cnt = std::min(piece, l.count - o);
            hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)rows_grid(rb, cnt)), dim3(ROWS_THREADS), 0, c->stream,
                               (const uint8_t*)seg, dst + o * rb, rb, d_idx, l.first + o, cnt, rows_slots_per_row(rb));
            HIPCHK(c, hipGetLastError());
        }
    }
    return 0;
}

extern "C" int mastic_reports_compact(mastic_reports* rep, const uint8_t* keep, size_t staging_bytes, size_t* n_kept) {
    DeviceScope ds_(rep ? rep->ctx : nullptr);
    if (!rep) return MASTIC_EINVAL;
    mastic_ctx* c = rep->ctx;
    if (!rep->nonces.own || !rep->pub.own || !rep->wire_flags.own)
        return fail(c, MASTIC_EINVAL, "compact: the batch is a view (compact the batch that owns the memory)");
    if (!keep) return fail(c, MASTIC_EINVAL, "compact: null keep mask");
    if (rep->n > 0xffffffffull) return fail(c, MASTIC_EINVAL, "compact: too many reports");
    const CompactIndex ix = compact_index(keep, rep->n);
    if (n_kept) *n_kept = ix.n_kept;
    if (ix.n_kept == rep->n) return 0;  // nothing dropped: same contents, same generation
    if (ix.moved() > 0) {
        const McParams& p = c->p;
        struct Seg {
            DevBuf* b;
            size_t rb;
        } segs[5] = {{&rep->nonces, 16},
                     {&rep->pub, (size_t)mc_public_share_size(p)},
                     {&rep->in0, (size_t)mc_input_share_size(p, 0)},
                     {&rep->in1, (size_t)mc_input_share_size(p, 1)},
                     {&rep->wire_flags, 1}};
        size_t widest = 0;
        for (const Seg& s : segs)
            if (s.b->p) widest = std::max(widest, s.rb);
        const size_t sb = compact_staging_bytes(staging_bytes, widest, ix.moved());
        // both allocations before any row moves: MASTIC_ENOMEM leaves the batch as it was
        DevBuf d_idx, stage;
        if (c->inject_alloc_failure() || !d_idx.ensure(4 * ix.n_kept) || !stage.ensure(sb))
            return fail(c, MASTIC_ENOMEM, "out of device memory (compact: %zu B staging, %zu B index)", sb,
                        4 * ix.n_kept);
        int rc = 0;
        if (hipMemcpyAsync(d_idx.p, ix.src.data(), 4 * ix.n_kept, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            rc = fail(c, MASTIC_EHIP, "compact: the index upload failed");
        for (const Seg& s : segs)
            if (!rc && s.b->p)
                rc = compact_segment(c, s.b->as<uint8_t>(), s.rb, ix, d_idx.as<uint32_t>(), stage.as<uint8_t>(), sb);
        // (also on failure: the index and the staging buffer are freed on return)
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc)
            rc = fail(c, MASTIC_EHIP, "compact: the row moves failed; the batch must be uploaded again");
        if (rc) {
            rep->touch();
            return rc;
        }
    }
    rep->touch();
    rep->n = ix.n_kept;
    return 0;
}

// ---------------------------------------------------------------- replay set
// The nonces an aggregator has admitted, in HBM (nonce_set.hpp: layout, hash
// and sizing rules; nonce_set_kernels.hpp: the kernels).  Every call blocks,
// runs on the ctx's main stream and leaves the table holding arena ids only.
struct mastic_nonce_set {
    mastic_ctx* ctx = nullptr;
    NsHashKey hk{};
    uint64_t count = 0;       // keys in the arena
    uint64_t slots = 0;       // of `table`
    uint64_t arena_keys = 0;  // capacity of `arena`
    bool broken = false;      // a probe came full circle or a launch failed mid-admit: every later call fails
    DevBuf table, arena;
    DevBuf words;             // NS_WORDS words: error flag, fresh counter
    DevBuf stage;             // the host nonces of an admit / query
    DevBuf fresh, slot_of;    // per nonce of the batch (resolve -> commit)
    NsTable dev(const DevBuf& t, const DevBuf& a, uint64_t nslots) const {
        return NsTable{t.as<uint32_t>(), a.as<uint4>(), (uint32_t)nslots, (uint32_t)count, hk};
    }
};

// Every allocation of a set takes the ctx's allocation-failure hook
// (mastic_set_test_hooks); one that is large enough already is none.
static bool ns_alloc(mastic_ctx* c, DevBuf& b, size_t want) {
    if (want <= b.bytes && b.p) return true;
    return !c->inject_alloc_failure() && b.ensure(want);
}

static int ns_broken(mastic_nonce_set* s, const char* what) {
    s->broken = true;
    (void)hipStreamSynchronize(s->ctx->stream);
    return fail(s->ctx, MASTIC_EHIP, "nonce set: %s; the set is unusable", what);
}

// Make the table and the arena fit `keys` keys (the growth rules of
// nonce_set.hpp).  Both new buffers are allocated before anything is touched,
// so MASTIC_ENOMEM leaves the set as it was; the old ones are dropped once the
// copy and the rehash that read them are done.
static int ns_reserve(mastic_nonce_set* s, uint64_t keys) {
    mastic_ctx* c = s->ctx;
    const uint64_t slots = ns_grown_slots(s->slots, keys);
    const uint64_t cap = ns_grown_arena(s->arena_keys, slots, keys);
    if (slots == s->slots && cap == s->arena_keys) return 0;
    DevBuf table, arena;
    if ((slots != s->slots && !ns_alloc(c, table, 4 * slots)) || (cap != s->arena_keys && !ns_alloc(c, arena, 16 * cap)))
        return fail(c, MASTIC_ENOMEM, "out of device memory (nonce set of %llu keys)", (unsigned long long)keys);
    uint32_t w[NS_WORDS] = {};
    if (arena.p && s->count)
        HIPCHK(c, hipMemcpyAsync(arena.p, s->arena.p, 16 * s->count, hipMemcpyDeviceToDevice, c->stream));
    if (table.p) {
        HIPCHK(c, hipMemsetAsync(table.p, 0, 4 * slots, c->stream));
        if (s->count) {
            HIPCHK(c, hipMemsetAsync(s->words.p, 0, 4 * NS_WORDS, c->stream));
            hipLaunchKernelGGL(k_ns_rehash, dim3((unsigned)((s->count + 255) / 256)), dim3(256), 0, c->stream,
                               s->dev(table, arena.p ? arena : s->arena, slots), (uint32_t)s->count,
                               s->words.as<uint32_t>());
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(w, s->words.p, sizeof w, hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (w[NS_ERR]) return ns_broken(s, "a rehash probe came full circle");
    if (table.p) {
        std::swap(s->table.p, table.p);
        std::swap(s->table.bytes, table.bytes);
        s->slots = slots;
    }
    if (arena.p) {
        std::swap(s->arena.p, arena.p);
        std::swap(s->arena.bytes, arena.bytes);
        s->arena_keys = cap;
    }
    return 0;
}

// Admit the n nonces at d_batch (device memory, 16-byte aligned).
static int ns_admit(mastic_nonce_set* s, const uint4* d_batch, size_t n, uint8_t* fresh_out, size_t* n_fresh) {
    mastic_ctx* c = s->ctx;
    if (n_fresh) *n_fresh = 0;
    if (n == 0) return 0;
    if (n > NS_MAX_KEYS || s->count + n > NS_MAX_KEYS) return fail(c, MASTIC_EINVAL, "nonce set: too many nonces");
    // all growth (table, arena, rehash, scratch) before the first insert: a failure
    // here leaves the set's contents as they were (at most its buffers larger)
    int rc = ns_reserve(s, s->count + n);
    if (rc) return rc;
    if (!ns_alloc(c, s->fresh, n) || !ns_alloc(c, s->slot_of, 4 * n))
        return fail(c, MASTIC_ENOMEM, "out of device memory (nonce set scratch for %zu nonces)", n);
    const dim3 grid((unsigned)((n + 255) / 256));
    const NsTable t = s->dev(s->table, s->arena, s->slots);
    uint32_t* words = s->words.as<uint32_t>();
    uint32_t w[NS_WORDS] = {};
    HIPCHK(c, hipMemsetAsync(words, 0, 4 * NS_WORDS, c->stream));
    hipLaunchKernelGGL(k_ns_insert, grid, dim3(256), 0, c->stream, t, d_batch, (uint32_t)n, words);
    hipLaunchKernelGGL(k_ns_resolve, grid, dim3(256), 0, c->stream, t, d_batch, (const uint4*)nullptr, (uint32_t)n,
                       s->fresh.as<uint8_t>(), s->slot_of.as<uint32_t>(), words);
    hipLaunchKernelGGL(k_ns_commit, grid, dim3(256), 0, c->stream, s->table.as<uint32_t>(), s->arena.as<uint4>(),
                       (uint32_t)s->count, d_batch, (uint32_t)n, s->fresh.as<uint8_t>(), s->slot_of.as<uint32_t>(),
                       words);
    // from the first launch on the table may hold batch ids: a failure leaves no usable set
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(w, words, sizeof w, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        (fresh_out && hipMemcpyAsync(fresh_out, s->fresh.p, n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return ns_broken(s, "an admit's launches failed");
    if (w[NS_ERR] || w[NS_FRESH] > n) return ns_broken(s, "an admit's probe came full circle");
    s->count += w[NS_FRESH];
    if (n_fresh) *n_fresh = w[NS_FRESH];
    return 0;
}

// The host nonces of an admit / query, copied to the set's staging buffer.
static int ns_stage(mastic_nonce_set* s, const uint8_t* nonces, size_t n) {
    mastic_ctx* c = s->ctx;
    if (!nonces) return fail(c, MASTIC_EINVAL, "nonce set: null nonces");
    if (n > NS_MAX_KEYS) return fail(c, MASTIC_EINVAL, "nonce set: too many nonces");
    if (!ns_alloc(c, s->stage, 16 * n)) return fail(c, MASTIC_ENOMEM, "out of device memory (nonce staging)");
    HIPCHK(c, hipMemcpy(s->stage.p, nonces, 16 * n, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int mastic_nonce_set_create(mastic_ctx* c, size_t capacity_hint, const uint8_t hash_key[16],
                                       mastic_nonce_set** out) {
    DeviceScope ds_(c);
    if (!c || !out) return MASTIC_EINVAL;
    *out = nullptr;
    if (capacity_hint > NS_MAX_KEYS) return fail(c, MASTIC_EINVAL, "nonce set: capacity hint too large");
    uint8_t key[16];
    if (hash_key)
        memcpy(key, hash_key, 16);
    else if (getentropy(key, sizeof key) != 0)
        return fail(c, MASTIC_EHIP, "nonce set: no entropy for the hash key");
    std::unique_ptr<mastic_nonce_set> s(new mastic_nonce_set());
    s->ctx = c;
    memcpy(&s->hk.k0, key, 8);
    memcpy(&s->hk.k1, key + 8, 8);
    if (!ns_alloc(c, s->words, 4 * NS_WORDS)) return fail(c, MASTIC_ENOMEM, "out of device memory (nonce set)");
    const int rc = ns_reserve(s.get(), capacity_hint);
    if (rc) return rc;
    *out = s.release();
    return 0;
}

extern "C" void mastic_nonce_set_destroy(mastic_nonce_set* s) {
    DeviceScope ds_(s ? s->ctx : nullptr);
    if (!s) return;
    (void)hipStreamSynchronize(s->ctx->stream);
    delete s;
}

extern "C" size_t mastic_nonce_set_count(const mastic_nonce_set* s) { return s ? (size_t)s->count : 0; }

#define NS_USABLE(s)                                                                                      \
    do {                                                                                                  \
        if (!(s)) return MASTIC_EINVAL;                                                                   \
        if ((s)->broken) return fail((s)->ctx, MASTIC_EHIP, "nonce set: unusable after an earlier failure"); \
    } while (0)

extern "C" int mastic_nonce_set_admit(mastic_nonce_set* s, const uint8_t* nonces, size_t n, uint8_t* fresh_out,
                                      size_t* n_fresh) {
    DeviceScope ds_(s ? s->ctx : nullptr);
    NS_USABLE(s);
    if (n == 0) return ns_admit(s, nullptr, 0, fresh_out, n_fresh);
    const int rc = ns_stage(s, nonces, n);
    return rc ? rc : ns_admit(s, s->stage.as<uint4>(), n, fresh_out, n_fresh);
}

extern "C" int mastic_nonce_set_admit_reports(mastic_nonce_set* s, mastic_reports* rep, uint8_t* fresh_out,
                                              size_t* n_fresh) {
    DeviceScope ds_(s ? s->ctx : nullptr);
    NS_USABLE(s);
    if (!rep || rep->ctx != s->ctx) return fail(s->ctx, MASTIC_EINVAL, "nonce set: the reports belong to another ctx");
    return ns_admit(s, rep->nonces.as<uint4>(), rep->n, fresh_out, n_fresh);
}

extern "C" int mastic_nonce_set_contains(mastic_nonce_set* s, const uint8_t* nonces, size_t n, uint8_t* found_out) {
    DeviceScope ds_(s ? s->ctx : nullptr);
    NS_USABLE(s);
    if (n == 0) return 0;
    mastic_ctx* c = s->ctx;
    if (!found_out) return fail(c, MASTIC_EINVAL, "nonce set: null output");
    int rc = ns_stage(s, nonces, n);
    if (rc) return rc;
    if (!ns_alloc(c, s->fresh, n)) return fail(c, MASTIC_ENOMEM, "out of device memory (nonce set scratch)");
    uint32_t w[NS_WORDS] = {};
    HIPCHK(c, hipMemsetAsync(s->words.p, 0, 4 * NS_WORDS, c->stream));
    hipLaunchKernelGGL(k_ns_resolve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       s->dev(s->table, s->arena, s->slots), (const uint4*)nullptr, s->stage.as<uint4>(), (uint32_t)n,
                       s->fresh.as<uint8_t>(), (uint32_t*)nullptr, s->words.as<uint32_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(w, s->words.p, sizeof w, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(found_out, s->fresh.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (w[NS_ERR]) return ns_broken(s, "a query's probe came full circle");
    return 0;
}

extern "C" int mastic_nonce_set_export(mastic_nonce_set* s, uint8_t* nonces_out, size_t capacity, size_t* n_out) {
    DeviceScope ds_(s ? s->ctx : nullptr);
    NS_USABLE(s);
    mastic_ctx* c = s->ctx;
    if (n_out) *n_out = (size_t)s->count;
    if (capacity < s->count) return fail(c, MASTIC_EINVAL, "nonce set: export buffer too small");
    if (s->count == 0) return 0;
    if (!nonces_out) return fail(c, MASTIC_EINVAL, "nonce set: null output");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(nonces_out, s->arena.p, 16 * s->count, hipMemcpyDeviceToHost));
    return 0;
}

// ---------------------------------------------------------------- ctx
extern "C" int mastic_ctx_create(const mastic_params* up, mastic_ctx** out) {
    if (!up || !out) return MASTIC_EINVAL;
    *out = nullptr;
    McParams p;
    if (mc_derive((int)up->circuit, (int)up->bits, (int)up->length, (int)up->sum_vec_bits, up->max_measurement,
                  (int)up->chunk_length, &p))
        return MASTIC_EINVAL;
    if (p.bits > TREE_MAX_BITS) return MASTIC_EINVAL;  // node paths are at most 256 bits (host_tree.hpp)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MASTIC_ENODEV;
    if (up->device < 0 || up->device >= ndev) return MASTIC_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, up->device) != hipSuccess) return MASTIC_ENODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return MASTIC_ENODEV;
    if (hipSetDevice(up->device) != hipSuccess) return MASTIC_ENODEV;
    mastic_ctx* c = new mastic_ctx();
    c->user = *up;
    c->p = p;
    c->device = up->device;
    c->k.n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, up->device) == hipSuccess && khz > 0)
            c->wall_khz = khz;
    }
#ifdef MASTIC_EXPERIMENT_KNOBS
    // A/B and timing experiments only (tools/ab_*.sh build the library with
    // -DMASTIC_EXPERIMENT_KNOBS; the shipped library reads none of these):
    // the knobs that are still open and have no mastic_set_* entry point.
    {
        const char* e = getenv("MASTIC_ABSORB_SINGLE");
        if (e) c->k.absorb_mode = e[0] == '1' ? 1 : (e[0] == '2' ? 2 : 0);
        const char* esm = getenv("MASTIC_ABSORB_SINGLE_MIN");
        if (esm) c->k.absorb_single_min = (size_t)std::max(0, atoi(esm));
        const char* spd = getenv("MASTIC_STRIDE_PAD");
        if (spd) c->m.stride_pad = std::max(0, std::min(1 << 20, atoi(spd))) / 64 * 64;
        const char* wa = getenv("MASTIC_WORK_ARENA_GB");
        if (wa) c->m.work_arena = c->m.work_arena_fc = (size_t)std::max(0, atoi(wa)) << 30;
        const char* cp = getenv("MASTIC_CHUNK_PIPELINE");
        if (cp) c->m.chunk_pipeline = cp[0] != '0';
        const char* fp = getenv("MASTIC_FUSE_PROOFS");
        if (fp) c->k.fuse_proofs = atoi(fp) > 0;
        const char* cr = getenv("MASTIC_CHUNK_REPORTS");
        if (cr) c->m.chunk_max = (size_t)std::max(0, atoi(cr));
        const char* spl = getenv("MASTIC_SPLIT_SPONGES");
        if (spl) c->k.split_sponges = spl[0] == '1' ? 1 : 0;
        const char* sgb = getenv("MASTIC_SEG_BALANCE");
        if (sgb) c->k.seg_balance = sgb[0] != '0';
    }
#endif
    // the level kernel's LDS (table + key schedules) is dynamic, above the
    // 64 KiB default: every variant the plan may launch, of both fields
    auto lds = [](const void* fn, int bytes) {
        return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
    };
    bool attrs = true;
    for (int v : LEVEL_VARIANTS)
        attrs = attrs && lds((const void*)level_kernel<F64>(v), EVAL_LDS_BYTES) &&
                lds((const void*)level_kernel<F128>(v), EVAL_LDS_BYTES);
    attrs = attrs && lds((const void*)level_kernel<F64>(LV_FC_PAY), EVAL_LDS_BYTES) &&
            lds((const void*)level_kernel<F128>(LV_FC_PAY), EVAL_LDS_BYTES);
    // the binder sponges are the latency-critical chain: their stream gets the
    // highest priority so their workgroups are dispatched first
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (!attrs || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipStreamCreateWithPriority(&c->stream3, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream4, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return MASTIC_EHIP;
    }
    *out = c;
    return 0;
}

extern "C" void mastic_ctx_destroy(mastic_ctx* c) {
    DeviceScope ds_(c);
    if (!c) return;
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->stream2);
    (void)hipStreamSynchronize(c->stream3);
    (void)hipStreamSynchronize(c->stream4);
    delete c;
}

extern "C" const char* mastic_last_error(const mastic_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

extern "C" int mastic_set_frontier_cache(mastic_ctx* c, int on, int* last_hit) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    if (on >= 0) {
        c->frontier_cache = on != 0;
        if (!on) {
            // queued kernels may still read the cache slots: retire them (freed
            // at the next idle point of the ctx's streams), no synchronisation
            for (auto& x : c->lc) {
                for (DevBuf* b : {&x.sp, &x.rootsum, &x.nd}) c->retire(*b);
                x.release();
            }
            c->retire(c->fc_spare);
            c->spare_words = 0;
            c->spare_S = 0;
        }
    }
    if (last_hit) *last_hit = c->last_hit ? 1 : 0;
    return 0;
}

extern "C" int mastic_set_frontier_cache_nodes(mastic_ctx* c, int mode, int* last_in, int* last_out) {
    if (!c || mode > FC_NODES_AUTO) return MASTIC_EINVAL;
    const int prev = c->fc_nodes;
    // the slots keep their formats (a hit reads either), so the cache stays as it is
    if (mode >= 0) c->fc_nodes = mode;
    if (last_in) *last_in = c->last_nodes_in;
    if (last_out) *last_out = c->last_nodes_out;
    return prev;
}

extern "C" int mastic_set_test_hooks(mastic_ctx* c, int force_slow_blk, int fail_allocs) {
    if (!c) return MASTIC_EINVAL;
    const int pending = c->fail_allocs;
    c->force_slow_blk = force_slow_blk < 0 ? -1 : force_slow_blk;
    c->fail_allocs = std::max(0, fail_allocs);
    return pending;
}

extern "C" int mastic_set_serial_sponges(mastic_ctx* c, int on) {
    if (!c) return MASTIC_EINVAL;
    const int prev = c->serial_sponges ? 1 : 0;
    if (on >= 0) c->serial_sponges = on != 0;
    return prev;
}

extern "C" int mastic_set_last_level_segments(mastic_ctx* c, int k) {
    if (!c || k < 0) return MASTIC_EINVAL;
    const int prev = c->k.last_level_segments;
    c->k.last_level_segments = k;
    return prev;
}

extern "C" int mastic_set_test_sponge_delay(mastic_ctx* c, int delay_us) {
    if (!c || delay_us < 0 || delay_us > 10000000) return MASTIC_EINVAL;
    c->sponge_delay_us = delay_us;
    return 0;
}

extern "C" int mastic_abi_version(void) { return MASTIC_ABI_VERSION; }

extern "C" int mastic_set_memory_budget(mastic_ctx* c, uint64_t bytes) {
    if (!c) return MASTIC_EINVAL;
    c->m.budget = bytes;
    return 0;
}

extern "C" int mastic_get_sizes(const mastic_ctx* c, mastic_sizes* s) {
    if (!c || !s) return MASTIC_EINVAL;
    const McParams& p = c->p;
    s->field_bytes = p.enc;
    s->value_len = p.value_len;
    s->meas_len = p.meas_len;
    s->output_len = p.output_len;
    s->proof_len = p.proof_len;
    s->verifier_len = p.verifier_len;
    s->joint_rand_len = p.joint_rand_len;
    s->query_rand_len = p.query_rand_len;
    s->prove_rand_len = p.prove_rand_len;
    s->rand_size = mc_rand_size(p);
    s->public_share_size = mc_public_share_size(p);
    s->input_share_size[0] = mc_input_share_size(p, 0);
    s->input_share_size[1] = mc_input_share_size(p, 1);
    s->prep_share_size[0] = mc_prep_share_size(p, false);
    s->prep_share_size[1] = mc_prep_share_size(p, true);
    s->algorithm_id = p.alg_id;
    return 0;
}
