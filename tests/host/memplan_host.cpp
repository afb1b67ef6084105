// Host harness for the memory plan of a prep_init
// (draft-mouris-cfrg-mastic_amd/csrc/memplan.hpp, executed by prep.hpp
// mastic_prep_init).  Two parts:
//   (a) frontier_hit, spare_capacity and the chunking (arena_fits, call_budget,
//       plan_arena, plan_chunks) over a grid of inputs, against values recorded
//       from the text of mastic_prep_init before it moved into memplan.hpp: the
//       three run_* functions below then held that text, with the work arena's
//       ensure() replaced by a stub whose outcome is a parameter.  The chunk
//       grid has ~10^5 rows, so what is recorded is one FNV-1a hash per
//       (n, per_report) slice plus a few whole rows; `memplan_host --dump`
//       prints every row, which is how two versions are compared in full;
//   (b) invariants of every chunk plan of the same grid, and of the spare-slot
//       growth rule.
// Prints the number of cases and "memplan_host: OK" and returns 0, or one line
// per failure and 1.  Run under ASan/UBSan by tests/test_memplan_host.py.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../draft-mouris-cfrg-mastic_amd/csrc/memplan.hpp"

static int g_failures = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (g_failures++ < 40) {              \
                printf("FAIL %s: ", #cond);       \
                printf(__VA_ARGS__);              \
                printf("\n");                     \
            }                                     \
        }                                         \
    } while (0)

typedef unsigned long long u64;

// ---- what runs under the grids (the parent's text stood here when the values were recorded)
struct ChunkCase {
    size_t n, per_report, have_bytes;
    MemKnobs k;
    size_t free_bytes;  // what the free-memory query would return
    bool cache_on;
    int outcome;  // of the arena's allocation: 0 `arena` succeeds, 1 `arena` fails and `want` succeeds, 2 both fail
};
enum { RC, QUERIED, BUDGET, BY_BUDGET, ALLOCATED, WORK_BYTES, CHUNK, PIPE, HALF, N_FULL, N_LAST, COUNT, ROW_LEN };
struct ChunkRow {
    u64 v[ROW_LEN] = {};  // RC: 0 planned, 1 64 reports exceed the budget, 2 out of memory
};

static ChunkRow run_chunk_case(const ChunkCase& q) {
    ChunkRow r;
    const bool fits = arena_fits(q.k, q.n, q.per_report, q.have_bytes);
    std::optional<size_t> free_bytes;
    if (!fits && !q.k.budget) {
        free_bytes = q.free_bytes;
        r.v[QUERIED] = 1;
    }
    const uint64_t budget = call_budget(q.k, q.n, q.per_report, fits, q.cache_on, free_bytes);
    const ArenaPlan a = plan_arena(q.k, q.n, q.per_report, q.have_bytes, budget, q.cache_on);
    r.v[BUDGET] = budget;
    r.v[BY_BUDGET] = a.by_budget;
    size_t work_bytes = q.have_bytes;
    if (a.action == ArenaPlan::TOO_SMALL) {
        r.v[RC] = 1;
        return r;
    }
    if (a.action == ArenaPlan::ALLOC) {
        r.v[ALLOCATED] = 1;
        if (q.outcome == 2) {
            r.v[RC] = 2;
            return r;
        }
        work_bytes = q.outcome == 0 ? a.arena : a.want;
    }
    const ChunkSizes s = plan_chunks(q.k, q.n, q.per_report, work_bytes, a.by_budget);
    r.v[WORK_BYTES] = work_bytes;
    r.v[CHUNK] = s.chunk;
    r.v[PIPE] = s.pipe;
    r.v[HALF] = s.half;
    r.v[N_FULL] = s.n_full;
    r.v[N_LAST] = s.n_last;
    r.v[COUNT] = s.count;
    return r;
}

static bool run_hit(const FrontierMeta& lc, const TreeShape& t, uint64_t rep_id, uint64_t rep_gen, size_t n, size_t S1,
                    const std::vector<uint8_t>& key) {
    return frontier_hit(lc, t, rep_id, rep_gen, n, S1, key);
}

static size_t run_spare(size_t nl, size_t spare_cap, bool query_ok, size_t free_bytes, size_t S1) {
    return spare_capacity(nl, spare_cap, query_ok ? std::optional<size_t>(free_bytes) : std::nullopt, S1);
}

// ---- the chunk grid
static const size_t NS[] = {1,    63,    64,    65,     127,    128,     129,    200,
                            8192, 16384, 65536, 131072, 400000, 1 << 20, 2 << 20};
// bytes per report: C2-like (~8.6 MB), Count-like, a small tree
static const size_t PERS[] = {8601236, 48340, 1900};
static const size_t GB = (size_t)1 << 30;

static u64 fnv(u64 h, u64 x) {
    for (int i = 0; i < 8; i++) h = (h ^ ((x >> (8 * i)) & 0xff)) * 0x100000001b3ull;
    return h;
}

// the grid's own estimate of the reports a budget allows (it only places the arena states)
static size_t grid_by_budget(uint64_t budget, size_t free_bytes, bool cache_on, size_t per, size_t pad) {
    const uint64_t b = budget ? budget : (uint64_t)(free_bytes * 0.75) * (cache_on ? 2 : 3) / 3;
    const size_t by = b / per / 64 * 64;
    return by > pad + 64 ? by - pad : by;
}

// (b) what every planned row must satisfy
static void check_row(const ChunkCase& q, const ChunkRow& r) {
    if (r.v[RC] != 0) return;
    const size_t pad = (size_t)q.k.stride_pad, chunk = r.v[CHUNK], bytes = r.v[WORK_BYTES], per = q.per_report;
    const bool pipe = r.v[PIPE] != 0;
    CHECK(chunk >= 64 && chunk % 64 == 0, "n %zu per %zu: chunk %zu", q.n, per, chunk);
    if (chunk == 0) return;
    CHECK((chunk + pad) * per <= (pipe ? bytes / 2 : bytes), "n %zu per %zu: chunk %zu of %zu bytes, pipe %d", q.n,
          per, chunk, bytes, (int)pipe);
    const size_t count = r.v[COUNT], n_last = r.v[N_LAST], n_full = r.v[N_FULL];
    CHECK(count >= 1 && (count - 1) * chunk + n_last == q.n, "n %zu: %zu chunks of %zu, last %zu", q.n, count, chunk,
          n_last);
    CHECK(0 < n_last && n_last <= chunk, "n %zu: chunk %zu, last %zu", q.n, chunk, n_last);
    CHECK(n_full == std::min(chunk, q.n) && (count == 1 ? n_last == n_full : n_full == chunk), "n %zu: full %zu", q.n,
          n_full);
    if (q.k.budget)
        CHECK(chunk <= std::max<size_t>(r.v[BY_BUDGET], 64), "n %zu: chunk %zu over the budget's %llu", q.n, chunk,
              r.v[BY_BUDGET]);
    if (q.k.chunk_max) CHECK(chunk <= round_up(q.k.chunk_max, 64), "n %zu: chunk %zu over chunk_max", q.n, chunk);
    if (pipe) {
        const size_t half = r.v[HALF];
        CHECK(q.k.chunk_pipeline && count >= 2, "n %zu: pipelined, %zu chunks", q.n, count);
        CHECK(half % 64 == 0 && (chunk + pad) * per <= half * 4 && half * 4 + (chunk + pad) * per <= bytes,
              "n %zu per %zu: halves of %zu rows at word %zu of %zu bytes", q.n, per, chunk + pad, half, bytes);
    }
}

static size_t g_chunk_cases = 0;

// One (n, per_report) slice of the grid: hashes every row (and dumps it on request).
static u64 chunk_slice(size_t n, size_t per, bool dump) {
    u64 h = 0xcbf29ce484222325ull;
    const size_t rn = round_up(n, 64);
    for (int pad : {0, 64}) {
        // budgets: unset with 16 / 64 / 256 GB free, the GPU tests' explicit ones, and one of 63 rows
        struct { uint64_t budget; size_t free_bytes; } const budgets[] = {
            {0, 16 * GB}, {0, 64 * GB}, {0, 256 * GB},
            {(64 * 1 + 64) * per + 1000, 0}, {(64 * 2 + 64) * per + 1000, 0}, {(64 * 4 + 64) * per + 1000, 0},
            {(192 + 64) * per + 1000, 0}, {63 * per, 0}};
        for (const auto& bg : budgets)
            for (int cache_on = 0; cache_on < 2; cache_on++) {
                // the arena's states are relative to what the call needs when the arena is empty
                MemKnobs k0;
                k0.budget = bg.budget;
                k0.stride_pad = pad;
                const size_t by0 = grid_by_budget(bg.budget, bg.free_bytes, cache_on != 0, per, (size_t)pad);
                const size_t need = std::min(by0, rn) + (size_t)pad;
                const size_t big = std::max((need + 1) / 2, (size_t)pad + 2 * 65536);
                std::vector<size_t> haves = {0, need, 4 * need};
                if (need >= 64) haves.push_back(need - 64);
                if (big < need) {
                    haves.push_back(big);
                    haves.push_back(big - 1);
                }
                for (size_t have : haves) {
                    // the parent divides by zero when a budget below 64 reports meets an arena of
                    // pad .. pad + 63 rows (left as it is: DESIGN.md, memory plan)
                    if (by0 < 64 && have >= (size_t)pad && have < (size_t)pad + 64) continue;
                    for (size_t chunk_max : {0, 64, 100, 65536})
                        for (int pipeline = 0; pipeline < 2; pipeline++)
                            for (int outcome = 0; outcome < 3; outcome++) {
                                ChunkCase q{n, per, have * per + (have ? 12 : 0), k0, bg.free_bytes, cache_on != 0,
                                            outcome};
                                q.k.chunk_max = chunk_max;
                                q.k.chunk_pipeline = pipeline != 0;
                                const ChunkRow r = run_chunk_case(q);
                                if (outcome && !r.v[ALLOCATED]) continue;  // no allocation that could fail
                                g_chunk_cases++;
                                check_row(q, r);
                                for (u64 x : r.v) h = fnv(h, x);
                                if (dump) {
                                    printf("n %zu per %zu pad %d budget %llu free %zu cache %d have %zu max %zu pipe %d "
                                           "outcome %d:",
                                           n, per, pad, (u64)bg.budget, bg.free_bytes, cache_on, q.have_bytes,
                                           chunk_max, pipeline, outcome);
                                    for (u64 x : r.v) printf(" %llu", x);
                                    printf("\n");
                                }
                            }
                }
            }
    }
    return h;
}

// WANT-BEGIN (recorded from the parent's text)
static const u64 WANT_SLICES[15][3] = {
    {0x9010739d27f675c5ull, 0x3eca5989da097ce5ull, 0xae69b20a3c8bd345ull},
    {0xd96499d7f37a4cc5ull, 0xb48729ff38758a65ull, 0xb10d6bee412900c5ull},
    {0xecca4cb95aa1dd45ull, 0x888db8912f1e2265ull, 0x4fea26e5403bc445ull},
    {0xb3c8608b394f4155ull, 0x37db78cf15401805ull, 0x2ce354d79661e485ull},
    {0xe463533384a1a575ull, 0xb8418bc2aeeba555ull, 0x876b57343da9b855ull},
    {0xa8bbd8295989160dull, 0x6cd6363c9472056dull, 0x1a04e94d48652a85ull},
    {0x084dc298ddd5b67dull, 0xad8c1d5304c80c45ull, 0x0b854843b7e2a63dull},
    {0xdfbdafc5a323febdull, 0x379fce50dc8d7f65ull, 0x8280ec78e22a87bdull},
    {0x7abdc4673df30425ull, 0x637a33f153196485ull, 0x14099fb907e4457dull},
    {0xe28cebfd7ace61d5ull, 0xeebdb2d889af9825ull, 0x7e624969c3ee910dull},
    {0x6c06b97b244c7571ull, 0x601a176d8580b19dull, 0x78ff0ceb8e4fc16dull},
    {0x813ed621595c86b9ull, 0x633af2fa8727553dull, 0x7f721cdbbaf3102dull},
    {0xf6a3c7abfa595d56ull, 0x7edb2f38a92e3ff5ull, 0x9ae122ddd7dd894dull},
    {0x403c1b6ee8fdd4b3ull, 0x5eb3cacc8ba3bb40ull, 0xad750f45b79461adull},
    {0xb1cfa3f5cb68765eull, 0x0c3a4c073ad2fcf1ull, 0x2e23acf3d0f0b5e5ull},
};
static const u64 WANT_ROWS[8][ROW_LEN] = {
    {0, 0, 6188520, 128, 1, 9281280, 128, 0, 1160128, 128, 72, 2},
    {0, 0, 9282280, 128, 1, 9282280, 128, 0, 1160256, 128, 72, 2},
    {0, 0, 15469800, 256, 1, 15469800, 256, 0, 1933696, 200, 200, 1},
    {0, 0, 12376040, 192, 1, 12376040, 64, 1, 1546944, 64, 8, 4},
    {0, 0, 6188520, 128, 1, 9281280, 128, 0, 1160128, 128, 128, 64},
    {0, 0, 9282280, 128, 1, 9282280, 128, 0, 1160256, 128, 128, 64},
    {0, 0, 15469800, 256, 1, 15469800, 64, 1, 1933696, 64, 64, 128},
    {0, 0, 12376040, 192, 1, 12376040, 64, 1, 1546944, 64, 64, 128},
};
static const int WANT_HITS[] = {1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
static const u64 WANT_SPARE[] = {
    2, 2, 8, 8, 8, 8, 2, 2, 8, 8, 8, 8,
    2, 2, 8, 8, 8, 8, 2, 2, 8, 8, 8, 8,
    2, 2, 8, 8, 8, 8, 2, 2, 8, 8, 8, 8,
    2, 2, 8, 8, 8, 8, 2, 2, 8, 8, 8, 8,
    2, 2, 8, 8, 8, 8, 2, 2, 8, 8, 8, 8,
    2, 2, 8, 8, 8, 8, 2, 2, 8, 8, 8, 8,
    10, 10, 40, 40, 40, 40, 10, 10, 40, 40, 40, 40,
    10, 10, 10, 40, 40, 40, 10, 10, 40, 40, 40, 40,
    10, 10, 40, 40, 40, 40, 10, 10, 10, 40, 40, 40,
    10, 10, 40, 40, 40, 40, 10, 10, 40, 40, 40, 40,
    10, 10, 10, 40, 40, 40, 10, 10, 40, 40, 40, 40,
    10, 10, 40, 40, 40, 40, 10, 10, 10, 40, 40, 40,
    11, 11, 40, 40, 40, 40, 11, 11, 40, 40, 40, 40,
    11, 11, 11, 40, 40, 40, 1000, 1000, 4000, 4000, 4000, 4000,
    1000, 1000, 1300, 4000, 4000, 4000, 1000, 1000, 1000, 1000, 1000, 2621,
    1000, 1000, 4000, 4000, 4000, 4000, 1000, 1000, 1300, 4000, 4000, 4000,
    1000, 1000, 1000, 1000, 1000, 2621, 1000, 1000, 4000, 4000, 4000, 4000,
    1000, 1000, 1300, 4000, 4000, 4000, 1000, 1000, 1000, 1000, 1000, 2621,
    1000, 1000, 4000, 4000, 4000, 4000, 1000, 1000, 1300, 4000, 4000, 4000,
    1000, 1000, 1000, 1000, 1000, 2621, 1248, 1248, 4000, 4000, 4000, 4000,
    1248, 1248, 1300, 4000, 4000, 4000, 1248, 1248, 1248, 1248, 1248, 2621,
    100000, 100000, 100000, 400000, 400000, 400000, 100000, 100000, 100000, 100000, 100000, 332943,
    100000, 100000, 100000, 100000, 100000, 100000, 100000, 100000, 100000, 400000, 400000, 400000,
    100000, 100000, 100000, 100000, 100000, 332943, 100000, 100000, 100000, 100000, 100000, 100000,
    100000, 100000, 100000, 400000, 400000, 400000, 100000, 100000, 100000, 100000, 100000, 332943,
    100000, 100000, 100000, 100000, 100000, 100000, 100000, 100000, 100000, 400000, 400000, 400000,
    100000, 100000, 100000, 100000, 100000, 332943, 100000, 100000, 100000, 100000, 100000, 100000,
    124998, 124998, 124998, 400000, 400000, 400000, 124998, 124998, 124998, 124998, 124998, 332943,
    124998, 124998, 124998, 124998, 124998, 124998, 2097152, 2097152, 2097152, 2097152, 5368709, 8388608,
    2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152,
    2097152, 2097152, 2097152, 2097152, 5368709, 8388608, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152,
    2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 5368709, 8388608,
    2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152,
    2097152, 2097152, 2097152, 2097152, 5368709, 8388608, 2097152, 2097152, 2097152, 2097152, 2097152, 2097152,
    2097152, 2097152, 2097152, 2097152, 2097152, 2097152, 2621438, 2621438, 2621438, 2621438, 5368709, 8388608,
    2621438, 2621438, 2621438, 2621438, 2621438, 2621438, 2621438, 2621438, 2621438, 2621438, 2621438, 2621438,
};
// WANT-END

static void check_chunks(bool dump) {
    for (size_t i = 0; i < sizeof NS / sizeof NS[0]; i++)
        for (size_t j = 0; j < sizeof PERS / sizeof PERS[0]; j++) {
            const u64 h = chunk_slice(NS[i], PERS[j], dump);
            if (dump) printf("slice %zu %zu: 0x%016llxull\n", i, j, h);
            CHECK(h == WANT_SLICES[i][j], "slice n %zu per %zu hashes to 0x%016llx, recorded 0x%016llx", NS[i], PERS[j],
                  h, WANT_SLICES[i][j]);
        }
    // whole rows: the GPU tests' explicit budgets over a Count-like layout, empty arena
    int row = 0;
    for (size_t n : {200, 8192})
        for (size_t rows : {64 * 1 + 64, 64 * 2 + 64, 64 * 4 + 64, 192 + 64}) {
            ChunkCase q{n, PERS[1], 0, MemKnobs(), 0, false, 0};
            q.k.budget = rows * PERS[1] + 1000;
            const ChunkRow r = run_chunk_case(q);
            if (dump) {
                printf("row %d:", row);
                for (u64 x : r.v) printf(" %llu,", x);
                printf("\n");
            }
            for (int i = 0; i < ROW_LEN; i++)
                CHECK(r.v[i] == WANT_ROWS[row][i], "row %d value %d is %llu, recorded %llu", row, i, r.v[i],
                      WANT_ROWS[row][i]);
            row++;
        }
}

// ---- frontier_hit: a base hit, every clause falsified on its own, the near-misses
static TreeShape tree_of(const std::vector<int>& n_parents, uint32_t salt) {
    TreeShape t;
    t.n_parents = n_parents;
    t.L = (int)n_parents.size() - 1;
    size_t o = 0;
    for (int np : n_parents) {
        t.off.push_back(o);
        o += 2 * (size_t)np;
    }
    t.off.push_back(o);
    t.nodes = o;
    t.child_path.resize(o * 8);
    for (size_t i = 0; i < t.child_path.size(); i++) t.child_path[i] = (uint32_t)(i * 2654435761u) ^ salt;
    return t;
}

static TreeShape truncated(const TreeShape& t, int L) {
    TreeShape c = t;
    c.L = L;
    c.n_parents.resize(L + 1);
    c.off.resize(L + 2);
    c.child_path.resize(c.off[L + 1] * 8);
    c.child_path.shrink_to_fit();
    return c;
}

static void check_hits(bool dump) {
    const std::vector<uint8_t> key = {2, 7, 9, 1, 2, 3};
    const size_t n = 180, S1 = 256;
    const TreeShape t = tree_of({1, 2, 3, 5, 6}, 0);  // the call: level 4
    FrontierMeta base;
    frontier_commit(base, truncated(t, 3), 11, 22, n, key);
    base.S = S1;
    CHECK(base.valid && base.L == 3 && base.n_parents.size() == 4 && base.paths.size() == 2 * 5 * 8, "commit");
    std::vector<int> got;
    auto run = [&](const FrontierMeta& lc, const TreeShape& tt, uint64_t id, uint64_t gen, size_t nn, size_t S,
                   const std::vector<uint8_t>& kk) { got.push_back(run_hit(lc, tt, id, gen, nn, S, kk)); };
    run(base, t, 11, 22, n, S1, key);  // the base hit
    FrontierMeta m = base;
    m.valid = false;
    run(m, t, 11, 22, n, S1, key);
    run(base, t, 12, 22, n, S1, key);      // another batch
    run(base, t, 11, 23, n, S1, key);      // its contents changed
    run(base, t, 11, 22, n + 1, S1, key);  // n
    run(base, t, 11, 22, n, S1 + 64, key);  // stride
    std::vector<uint8_t> key2 = key;
    key2.back() ^= 1;
    run(base, t, 11, 22, n, S1, key2);
    TreeShape tw = t;
    tw.weight_check = true;
    run(base, tw, 11, 22, n, S1, key);
    run(base, truncated(t, 3), 11, 22, n, S1, key);  // the same level again
    FrontierMeta two;  // a cache two levels behind
    frontier_commit(two, truncated(t, 2), 11, 22, n, key);
    two.S = S1;
    run(two, t, 11, 22, n, S1, key);
    TreeShape tn = tree_of({1, 2, 4, 5, 6}, 0);  // a node count differs above level L - 1
    run(base, tn, 11, 22, n, S1, key);
    TreeShape tl = tree_of({1, 2, 3, 4, 6}, 0);  // level L - 1 has another width
    run(base, tl, 11, 22, n, S1, key);
    m = base;  // the cached paths are not level L - 1's nodes
    m.paths.resize(m.paths.size() - 8);
    run(m, t, 11, 22, n, S1, key);
    // near-miss: the node counts agree, one path word of level L - 1 differs
    TreeShape tp = t;
    tp.child_path[(tp.off[3] + 7) * 8 + 5] ^= 0x80;
    run(base, tp, 11, 22, n, S1, key);
    // near-miss: L == lc.L + 1, but the call has more levels than the cached vector holds
    m = base;
    m.n_parents.resize(2);
    m.n_parents.shrink_to_fit();
    run(m, t, 11, 22, n, S1, key);
    // a wider last level alone is still a hit
    TreeShape tw2 = tree_of({1, 2, 3, 5, 9}, 0);
    run(base, tw2, 11, 22, n, S1, key);
    if (dump) {
        printf("hits:");
        for (int g : got) printf(" %d,", g);
        printf("\n");
    }
    const size_t want_n = sizeof WANT_HITS / sizeof WANT_HITS[0];
    CHECK(got.size() == want_n, "%zu hit cases, recorded %zu", got.size(), want_n);
    for (size_t i = 0; i < got.size() && i < want_n; i++)
        CHECK(got[i] == WANT_HITS[i], "hit case %zu is %d, recorded %d", i, got[i], WANT_HITS[i]);
    CHECK(got[0] == 1 && got.back() == 1, "the base hits");
    for (size_t i = 1; i + 1 < got.size(); i++) CHECK(got[i] == 0, "hit case %zu must miss", i);
}

// ---- spare_capacity
static size_t g_spare_cases = 0;
static void check_spare(bool dump) {
    std::vector<u64> got;
    for (size_t nl : {2, 10, 1000, 100000, 2 << 20})
        for (size_t cap : {(size_t)0, (size_t)1, (size_t)8, nl / 2, nl - 1})
            for (size_t S1 : {128, 8256, (1 << 20) + 64})
                for (size_t free_gb : {(size_t)0, (size_t)1, (size_t)16, (size_t)64, (size_t)256})
                    for (int query_ok = 0; query_ok < 2; query_ok++) {
                        if (cap >= nl || (!query_ok && free_gb)) continue;
                        const size_t c = run_spare(nl, cap, query_ok != 0, free_gb * GB, S1);
                        got.push_back(c);
                        g_spare_cases++;
                        CHECK(c >= nl && c > cap, "spare of %zu nodes for %zu, was %zu", c, nl, cap);
                        CHECK(c <= std::max(std::max(nl, cap + cap / 4), 4 * nl), "spare of %zu nodes for %zu", c, nl);
                    }
    if (dump) {
        printf("spare:");
        for (u64 g : got) printf(" %llu,", g);
        printf("\n");
    }
    const size_t want_n = sizeof WANT_SPARE / sizeof WANT_SPARE[0];
    CHECK(got.size() == want_n, "%zu spare cases, recorded %zu", got.size(), want_n);
    for (size_t i = 0; i < got.size() && i < want_n; i++)
        CHECK(got[i] == WANT_SPARE[i], "spare case %zu is %llu, recorded %llu", i, got[i], WANT_SPARE[i]);
}

int main(int argc, char** argv) {
    const bool dump = argc > 1 && !strcmp(argv[1], "--dump");
    check_chunks(dump);
    check_hits(dump);
    check_spare(dump);
    printf("chunk cases checked: %zu\n", g_chunk_cases);
    printf("spare cases checked: %zu\n", g_spare_cases);
    if (g_failures) {
        printf("memplan_host: %d FAILURES\n", g_failures);
        return 1;
    }
    printf("memplan_host: OK\n");
    return 0;
}
