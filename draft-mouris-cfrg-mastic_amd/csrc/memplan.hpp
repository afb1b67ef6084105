// Host-only memory plan of a prep_init: the frontier cache's hit test and
// bookkeeping, the growth rule of its spare node slot, and how a call's
// reports are cut into chunks of the work arena.  Plain C++17, no HIP:
// mastic_hip.hip executes it (mastic_prep_init and its helpers own every
// hipMalloc and the free-memory queries), and tests/host/memplan_host.cpp
// checks it on a CPU under ASan / UBSan.
#pragma once
#include <algorithm>
#include <cstdint>
#include <optional>
#include <vector>

#include "host_tree.hpp"

inline size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

// ------------------------------------------------------------------ the knobs
// The fields of mastic_ctx that the memory decisions read (mastic_ctx::m;
// MASTIC_EXPERIMENT_KNOBS builds and mastic_set_memory_budget write them).
struct MemKnobs {
    uint64_t budget = 0;                   // bytes a call may plan with (mastic_set_memory_budget; 0 = by free HBM)
    int stride_pad = 64;                   // words of padding per plane row (MASTIC_STRIDE_PAD)
    size_t work_arena = (size_t)48 << 30;  // minimum size of a new work buffer (MASTIC_WORK_ARENA_GB)
    // ... with the frontier cache on (level sweeps, whose trees grow from level to level): large
    // enough that a 1M-report C2 sweep's cache misses run as one chunk (r02 v58: -4 % sweep time)
    size_t work_arena_fc = (size_t)128 << 30;
    size_t chunk_max = 0;        // reports per chunk cap (0 = what fits; MASTIC_CHUNK_REPORTS)
    bool chunk_pipeline = true;  // several chunks: two halves of the work arena (MASTIC_CHUNK_PIPELINE=0: off)
};

// ------------------------------------------------------------- frontier cache
// Host metadata of one aggregator's frontier cache (mastic_hip.hip LevelCache
// adds the device slots): what the cached call evaluated, and over which batch.
struct FrontierMeta {
    bool valid = false;
    uint64_t rep_id = 0, rep_gen = 0;  // the batch (mastic_reports::id) and its contents generation
    size_t n = 0;
    size_t S = 0;                 // plane stride (n rounded up to 64, plus padding)
    std::vector<uint8_t> key;     // u8(len) || verify key || ctx
    int L = -1;                   // level of the cached call
    std::vector<int> n_parents;   // per level 0..L
    std::vector<uint32_t> paths;  // child paths of level L (8 words per node)
    int node_words = 5;           // words per node of the aggregator's slot (the format of the call that wrote it)
    void drop() { valid = false; }
};

// The two formats of a cached node (mastic_set_frontier_cache_nodes).  seeds:
// [convert seed 4][ctrl], 5 words; a hit recomputes the parent's next seed and
// payload from its convert stream.  payloads: [next seed 4][ctrl][payload], the
// payload as the level kernel's emit corrected it, wlw = VALUE_LEN * w32 words.
// A slot's format is that of the call that wrote it (FrontierMeta::node_words);
// a hit reads either, whatever it writes itself.
enum NodeMode { FC_NODES_SEEDS = 0, FC_NODES_PAYLOADS = 1, FC_NODES_AUTO = 2 };
constexpr int SEED_NODE_WORDS = 5;
inline int payload_node_words(size_t wlw) { return SEED_NODE_WORDS + (int)wlw; }

// A call over tree t extends the cached call by exactly one level, over the
// same batch contents, plane stride S1 and key: it evaluates only level L.
// The slot's node format (lc.node_words) is not compared: either format hits.
inline bool frontier_hit(const FrontierMeta& lc, const TreeShape& t, uint64_t rep_id, uint64_t rep_gen, size_t n,
                         size_t S1, const std::vector<uint8_t>& key) {
    const int L = t.L;
    return lc.valid && lc.rep_id == rep_id && lc.rep_gen == rep_gen && lc.n == n && lc.S == S1 && lc.key == key &&
           !t.weight_check && L == lc.L + 1 && (size_t)L <= lc.n_parents.size() &&
           std::equal(t.n_parents.begin(), t.n_parents.begin() + L, lc.n_parents.begin()) &&
           // level L-1's node paths fix every level above (each level's
           // parents are the truncations of the next level's nodes), so
           // they and the node counts decide that the trees agree there
           lc.paths.size() == (t.off[L] - t.off[L - 1]) * 8 &&
           std::equal(lc.paths.begin(), lc.paths.end(), t.child_path.begin() + t.off[L - 1] * 8);
}

// The call over tree t has filled the cache (S was set when its slots were sized).
inline void frontier_commit(FrontierMeta& lc, const TreeShape& t, uint64_t rep_id, uint64_t rep_gen, size_t n,
                            const std::vector<uint8_t>& key, int node_words = SEED_NODE_WORDS) {
    lc.valid = true;
    lc.node_words = node_words;
    lc.rep_id = rep_id;
    lc.rep_gen = rep_gen;
    lc.n = n;
    lc.key = key;
    lc.L = t.L;
    lc.n_parents.assign(t.n_parents.begin(), t.n_parents.begin() + t.L + 1);
    lc.paths.assign(t.child_path.begin() + t.off[t.L] * 8,
                    t.child_path.begin() + (t.off[t.L] + 2 * t.n_parents[t.L]) * 8);
}

// Nodes of a new spare slot that must hold nl > spare_cap nodes of stride S1.
// Grow geometrically (a sweep's frontier widens over several levels), and
// while HBM is plentiful (free_bytes: none if the query failed) straight to up
// to 4x the need within a fifth of the free memory: each large hipMalloc costs
// ~1 s per 50 GB, so a 1M-report sweep should grow its slots a couple of
// times, not at every level.
// node_words: the node format the slot is sized for.
inline size_t spare_capacity(size_t nl, size_t spare_cap, std::optional<size_t> free_bytes, size_t S1,
                             size_t node_words = SEED_NODE_WORDS) {
    size_t cap = std::max(nl, spare_cap + spare_cap / 4);
    if (free_bytes) {
        const size_t per_node = node_words * S1 * 4;
        cap = std::max(cap, std::min(4 * nl, *free_bytes / 5 / per_node));
    }
    return cap;
}

// Slots are sized and tracked in words per plane row, not in nodes: a slot of
// slot_words holds nl nodes of node_words each if they fit, whichever format
// it was allocated for (a payload-width slot of c nodes holds c * NW / 5
// seeds-format nodes of a later, wider level without growing).
inline bool slot_holds(size_t slot_words, size_t nl, size_t node_words) { return nl * node_words <= slot_words; }

// The cache's share of the HBM: with the cache on, call_budget plans the work
// arena with half of the free memory where default_budget takes three
// quarters, so a quarter is the cache's.  held_bytes: what the three node
// slots hold now (free memory the cache has already taken).
inline size_t cache_quarter(size_t free_bytes, size_t held_bytes) { return (free_bytes + held_bytes) / 4; }

// Bytes of the three node slots (both aggregators' and the spare) of nl nodes each.
inline size_t node_slots_bytes(size_t nl, size_t node_words, size_t S1) { return 3 * nl * node_words * S1 * 4; }

// The node format a cache-on call writes.  seeds / payloads: as asked,
// whatever the memory.  auto: payloads if and only if all three slots, at
// payload width and at the capacity this level's nl nodes need, fit the
// cache's quarter of (free HBM + what the slots hold now); seeds if the
// free-memory query failed.  More free memory never turns payloads into
// seeds, more reports (S1) or nodes never seeds into payloads.
inline int choose_node_words(int mode, size_t nl, size_t wlw, size_t S1, std::optional<size_t> free_bytes,
                             size_t held_bytes) {
    const int nw = payload_node_words(wlw);
    if (mode == FC_NODES_PAYLOADS) return nw;
    if (mode != FC_NODES_AUTO || !free_bytes) return SEED_NODE_WORDS;
    return node_slots_bytes(nl, (size_t)nw, S1) <= cache_quarter(*free_bytes, held_bytes) ? nw : SEED_NODE_WORDS;
}

// Words per plane row of a new spare slot that must hold nl nodes of
// node_words (slot_holds(spare_words, ...) is false): spare_capacity's growth
// at that width.  bounded (auto chose payloads): the growth beyond the need
// stops where three such slots would leave the cache's quarter.
inline size_t spare_slot_words(size_t nl, size_t node_words, size_t spare_words, std::optional<size_t> free_bytes,
                               size_t S1, bool bounded = false, size_t held_bytes = 0) {
    size_t cap = spare_capacity(nl, spare_words / node_words, free_bytes, S1, node_words);
    if (bounded && free_bytes)
        cap = std::min(cap, std::max(nl, cache_quarter(*free_bytes, held_bytes) / 3 / (node_words * S1 * 4)));
    return cap * node_words;
}

// -------------------------------------------------------------------- chunking
// The HBM a call plans with when nothing narrows it: the explicit budget, else
// three quarters of the free memory (work buffers are the only large
// allocation, C2: ~8.6 MB per report; one chunk per batch keeps one
// binder-sponge chain per prep_init), 1 GiB if the query failed.
inline uint64_t default_budget(const MemKnobs& k, std::optional<size_t> free_bytes) {
    if (k.budget) return k.budget;
    if (!free_bytes) return 1ull << 30;
    return (uint64_t)(*free_bytes * 0.75);
}

// An arena of have_bytes that already holds the whole batch needs no budget
// (the caller then skips the free-memory query, ~tens of us per call).
inline bool arena_fits(const MemKnobs& k, size_t n, size_t per_report, size_t have_bytes) {
    return !k.budget && have_bytes / per_report >= round_up(n, 64) + (size_t)k.stride_pad;
}

// A prep_init's budget.  With the cache on, half of the free HBM (two thirds
// of the default): the other aggregator's slot may still grow at this level.
inline uint64_t call_budget(const MemKnobs& k, size_t n, size_t per_report, bool fits, bool cache_on,
                            std::optional<size_t> free_bytes) {
    if (fits) return (uint64_t)per_report * (round_up(n, 64) + (size_t)k.stride_pad);
    return (cache_on && !k.budget) ? default_budget(k, free_bytes) * 2 / 3 : default_budget(k, free_bytes);
}

struct ArenaPlan {
    enum Action { USE, ALLOC, TOO_SMALL } action = USE;  // TOO_SMALL: 64 reports do not fit the budget
    size_t arena = 0, want = 0;  // ALLOC: the bytes to try first, and what the chunk needs at least
    size_t by_budget = 0;        // reports per chunk the budget allows
};

// Whether the work arena (have_bytes now) serves the call as it is.
inline ArenaPlan plan_arena(const MemKnobs& k, size_t n, size_t per_report, size_t have_bytes, uint64_t budget,
                            bool cache_on) {
    ArenaPlan a;
    // Plane rows are padded by stride_pad words: with a power-of-two row
    // length every word of a report sits at the same address bits modulo a
    // large power of two, and the 42-plane block loads of the binder sponges
    // all land on the same memory channels.
    const size_t pad = (size_t)k.stride_pad;
    a.by_budget = (budget / per_report) / 64 * 64;
    if (a.by_budget > pad + 64) a.by_budget -= pad;  // the padded rows count against the budget too
    const size_t chunk = std::min<size_t>(round_up(n, 64), a.by_budget);
    // The work buffer is an arena kept across calls: a call uses all of its
    // capacity (even past the budget: it is allocated already), and a new
    // one is at least work_arena bytes (within the budget), so a level
    // sweep whose trees grow from level to level does not re-allocate it at
    // every level.
    const size_t have = have_bytes / per_report;
    // An arena that holds half the batch in chunks of >= 64k reports is used
    // as it is (pipelined chunks of that size keep the GPU full and hide each
    // other's sponge tails) rather than re-allocated for a single chunk.
    const size_t need = std::min(chunk, round_up(n, 64)) + pad;
    if (have >= need || (2 * have >= need && have >= pad + 2 * 65536)) return a;
    if (chunk < 64) {
        a.action = ArenaPlan::TOO_SMALL;
        return a;
    }
    a.action = ArenaPlan::ALLOC;
    a.want = per_report * (chunk + pad);
    a.arena = std::max(a.want, std::min<size_t>(cache_on ? k.work_arena_fc : k.work_arena, budget));
    return a;
}

struct ChunkSizes {
    size_t chunk = 0;  // reports per chunk (a multiple of 64)
    bool pipe = false;  // chunks alternate between the two halves of the arena
    size_t half = 0;   // words: the second half's offset
    size_t n_full = 0, n_last = 0, count = 0;  // reports of a full chunk and of the last one; chunks
};

// The chunks of a call over an arena of work_bytes (after plan_arena's allocation, if any).
inline ChunkSizes plan_chunks(const MemKnobs& k, size_t n, size_t per_report, size_t work_bytes, size_t by_budget) {
    ChunkSizes s;
    const size_t pad = (size_t)k.stride_pad;
    s.chunk = std::min<size_t>(round_up(n, 64), (work_bytes / per_report - pad) / 64 * 64);
    if (k.budget) s.chunk = std::min(s.chunk, std::max<size_t>(by_budget, 64));  // an explicit budget caps chunks
    // MASTIC_CHUNK_REPORTS caps a chunk below what fits, so a large batch runs
    // as several pipelined chunks (the trailing sponges of one overlap the
    // evaluation of the next) instead of one chunk with an exposed tail
    const bool capped = k.chunk_max > 0 && round_up(k.chunk_max, 64) < s.chunk;
    if (capped) s.chunk = round_up(k.chunk_max, 64);
    // Several chunks: pipeline them through the two halves of the work arena
    // (chunk k+1 evaluates in one half while chunk k's last sponges, finalize
    // and copies run on the sponge stream over the other).
    const size_t half_cap = work_bytes / 2 / per_report;  // reports (padding rows included) per half
    s.pipe = k.chunk_pipeline && n > s.chunk && s.chunk >= 128 && half_cap >= pad + 64;
    if (s.pipe) s.chunk = std::min(capped ? s.chunk : s.chunk / 2, half_cap - pad) / 64 * 64;
    s.half = work_bytes / 2 / 4 / 64 * 64;
    s.n_full = std::min(s.chunk, n);
    s.n_last = n - (n - 1) / s.chunk * s.chunk;
    s.count = (n - 1) / s.chunk + 1;
    return s;
}
