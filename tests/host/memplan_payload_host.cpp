// Host harness for the frontier cache's node formats in the memory plan
// (draft-mouris-cfrg-mastic_amd/csrc/memplan.hpp: FrontierMeta::node_words,
// slot_holds, spare_slot_words, choose_node_words; executed by prep.hpp
// cache_slots).  Checks
//   (a) frontier_hit accepts a cached level of either node width and
//       frontier_commit records the width;
//   (b) slot capacity in words: a payload-width slot of c nodes holds
//       c * NW / 5 seeds-format nodes without growing, and spare_capacity with
//       the defaulted width is the 5-word rule it was before it took a width;
//   (c) the auto policy at DESIGN.md §7's two anchors (the north_star C2 sweep
//       at 1M reports on one GPU: seeds; at the 8-GPU split's 125k reports per
//       rank: payloads);
//   (d) the policy's properties over a grid of reports, nodes, value widths,
//       free and held bytes.
// Prints the number of cases and "memplan_payload_host: OK" and returns 0, or
// one line per failure and 1.  Run under ASan/UBSan by
// tests/test_memplan_payload_host.py.
#include <cstdio>
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

static const size_t GB = 1000000000ull;   // DESIGN.md's figures are decimal
static const size_t GiB = (size_t)1 << 30;

// ---- (a) hit and commit
static TreeShape tree_of(const std::vector<int>& n_parents) {
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
    for (size_t i = 0; i < t.child_path.size(); i++) t.child_path[i] = (uint32_t)(i * 2654435761u);
    return t;
}

static TreeShape truncated(const TreeShape& t, int L) {
    TreeShape c = t;
    c.L = L;
    c.n_parents.resize(L + 1);
    c.off.resize(L + 2);
    c.child_path.resize(c.off[L + 1] * 8);
    return c;
}

static void check_hits() {
    const std::vector<uint8_t> key = {2, 7, 9, 1, 2, 3};
    const size_t n = 180, S1 = 256;
    const TreeShape t = tree_of({1, 2, 3, 5, 6});
    FrontierMeta fresh;
    CHECK(fresh.node_words == SEED_NODE_WORDS, "a new meta is seeds-format, %d words", fresh.node_words);
    for (int nw : {SEED_NODE_WORDS, payload_node_words(4), payload_node_words(34), payload_node_words(20)}) {
        FrontierMeta lc;
        frontier_commit(lc, truncated(t, 3), 11, 22, n, key, nw);
        lc.S = S1;
        CHECK(lc.valid && lc.node_words == nw, "commit records %d words, has %d", nw, lc.node_words);
        CHECK(frontier_hit(lc, t, 11, 22, n, S1, key), "a %d-word slot hits", nw);
        CHECK(!frontier_hit(lc, t, 11, 23, n, S1, key), "a %d-word slot of other contents misses", nw);
        // the next call overwrites the width with its own
        frontier_commit(lc, t, 11, 22, n, key);
        CHECK(lc.node_words == SEED_NODE_WORDS && lc.L == 4, "the defaulted commit is seeds-format");
    }
    CHECK(payload_node_words(34) == 39 && payload_node_words(4) == 9, "C2: 39 words (156 B), C3: 9 words (36 B)");
}

// ---- (b) capacity in words
static size_t old_spare_capacity(size_t nl, size_t spare_cap, std::optional<size_t> free_bytes, size_t S1) {
    // the rule before it took a node width (5-word nodes)
    size_t cap = std::max(nl, spare_cap + spare_cap / 4);
    if (free_bytes) {
        const size_t per_node = 5 * S1 * 4;
        cap = std::max(cap, std::min(4 * nl, *free_bytes / 5 / per_node));
    }
    return cap;
}

static size_t g_cap_cases = 0;
static void check_capacity() {
    for (size_t nw : {(size_t)9, (size_t)25, (size_t)39})
        for (size_t c : {(size_t)1, (size_t)2, (size_t)7, (size_t)366, (size_t)100000}) {
            const size_t words = c * nw, seeds = words / 5;
            CHECK(slot_holds(words, c, nw) && !slot_holds(words, c + 1, nw), "%zu nodes of %zu words", c, nw);
            CHECK(slot_holds(words, seeds, 5), "a slot of %zu x %zu words holds %zu seeds-format nodes", c, nw, seeds);
            CHECK(!slot_holds(words, seeds + 1, 5), "... and not %zu", seeds + 1);
            g_cap_cases++;
        }
    CHECK(!slot_holds(0, 2, 5), "an empty slot holds nothing");
    // the grid of tests/host/memplan_host.cpp check_spare
    const size_t GiBs[] = {0, 1, 16, 64, 256};
    for (size_t nl : {(size_t)2, (size_t)10, (size_t)1000, (size_t)100000, (size_t)2 << 20})
        for (size_t cap : {(size_t)0, (size_t)1, (size_t)8, nl / 2, nl - 1})
            for (size_t S1 : {(size_t)128, (size_t)8256, ((size_t)1 << 20) + 64})
                for (size_t free_gb : GiBs)
                    for (int query_ok = 0; query_ok < 2; query_ok++) {
                        if (cap >= nl || (!query_ok && free_gb)) continue;
                        const std::optional<size_t> fr =
                            query_ok ? std::optional<size_t>(free_gb * GiB) : std::nullopt;
                        const size_t want = old_spare_capacity(nl, cap, fr, S1);
                        CHECK(spare_capacity(nl, cap, fr, S1) == want, "defaulted width: nl %zu cap %zu", nl, cap);
                        CHECK(spare_capacity(nl, cap, fr, S1, 5) == want, "width 5: nl %zu cap %zu", nl, cap);
                        CHECK(spare_slot_words(nl, 5, cap * 5, fr, S1) == 5 * want, "words: nl %zu cap %zu", nl, cap);
                        // a wider node grows no further than the same bytes allow, and holds the need
                        const size_t w39 = spare_slot_words(nl, 39, cap * 39, fr, S1);
                        CHECK(slot_holds(w39, nl, 39) && w39 % 39 == 0 && w39 / 39 <= std::max(want, 4 * nl),
                              "39-word slot of %zu words for %zu nodes", w39, nl);
                        g_cap_cases++;
                    }
}

// ---- (c) DESIGN.md §7 ("Caching payloads instead of recomputing them on a hit"; memory plan, §0b)
static void check_anchors() {
    // C2 (Sum, Field64, VALUE_LEN 17): a payloads-format node is 39 words = 156 B; ~366 cached nodes
    // per report and slot at the north_star sweep's hit levels; the work arena's floor with the cache
    // on is 128 GiB (137 GB; MemKnobs::work_arena_fc), the sweep's misses need ~130 KB per report;
    // a GPU has 288 GB; reports, results and the rest are ~50 GB at 1M reports.
    const size_t wlw = 17 * 2, nl = 366, hbm = 288 * GB, arena = MemKnobs().work_arena_fc;
    CHECK(payload_node_words(wlw) * 4 == 156 && arena == 128 * GiB, "the anchors' constants");
    struct { size_t n; bool payloads; double slots_gb, free_gb; } const rows[] = {
        {1000000, false, 171, 79},  // one GPU: 171 GB of payload slots beside ~79 GB free
        {125000, true, 21, 142},    // the 8-GPU split: ~21 GB beside ~142 GB free
    };
    for (const auto& row : rows) {
        const size_t S1 = round_up(row.n, 64) + 64;
        const size_t resident = 50 * GB / 1000000 * row.n;
        CHECK(row.n * 130000 <= arena, "%zu reports' misses fit the arena floor", row.n);
        const size_t held = node_slots_bytes(nl, SEED_NODE_WORDS, S1);  // the sweep so far wrote seeds
        const size_t free_bytes = hbm - resident - arena - held;
        const size_t pay = node_slots_bytes(nl, (size_t)payload_node_words(wlw), S1);
        printf("anchor %zu reports: free %.1f GB, seeds slots %.1f GB, payload slots %.1f GB, quarter %.1f GB\n", row.n,
               free_bytes / 1e9, held / 1e9, pay / 1e9, cache_quarter(free_bytes, held) / 1e9);
        CHECK(pay / 1e9 > row.slots_gb - 1 && pay / 1e9 < row.slots_gb + 1, "payload slots %.1f GB", pay / 1e9);
        CHECK(free_bytes / 1e9 > row.free_gb - 1 && free_bytes / 1e9 < row.free_gb + 1, "free %.1f GB", free_bytes / 1e9);
        const int nw = choose_node_words(FC_NODES_AUTO, nl, wlw, S1, free_bytes, held);
        CHECK((nw > SEED_NODE_WORDS) == row.payloads, "%zu reports: auto chose %d words", row.n, nw);
        // the same once the slots hold what auto chose (no flapping from level to level)
        const size_t held2 = row.payloads ? pay : held;
        const int nw2 = choose_node_words(FC_NODES_AUTO, nl, wlw, S1, free_bytes + held - held2, held2);
        CHECK(nw2 == nw, "%zu reports: auto chose %d words, then %d", row.n, nw, nw2);
    }
}

// ---- (d) properties
static size_t g_policy_cases = 0;
static void check_policy() {
    const size_t ns[] = {64, 1000, 16384, 125000, 1000000, 2000000};
    const size_t nls[] = {2, 10, 366, 1000, 5000, 100000};
    const size_t wlws[] = {4, 20, 34, 400};
    const size_t frees[] = {0, 1 * GB, 8 * GB, 36 * GB, 79 * GB, 142 * GB, 256 * GB};
    const size_t helds[] = {0, 3 * GB, 22 * GB};
    const size_t NN = sizeof ns / sizeof ns[0], NL = sizeof nls / sizeof nls[0], NF = sizeof frees / sizeof frees[0];
    int n_pay = 0, n_seed = 0;
    for (size_t wlw : wlws)
        for (size_t held : helds) {
            const int nwp = payload_node_words(wlw);
            // choice[i][j][f]
            std::vector<int> choice(NN * NL * NF);
            for (size_t i = 0; i < NN; i++)
                for (size_t j = 0; j < NL; j++)
                    for (size_t f = 0; f < NF; f++) {
                        const size_t S1 = round_up(ns[i], 64) + 64, nl = nls[j];
                        const int nw = choose_node_words(FC_NODES_AUTO, nl, wlw, S1, frees[f], held);
                        CHECK(nw == SEED_NODE_WORDS || nw == nwp, "auto chose %d words", nw);
                        choice[(i * NL + j) * NF + f] = nw;
                        (nw > SEED_NODE_WORDS ? n_pay : n_seed)++;
                        g_policy_cases++;
                        const size_t quarter = cache_quarter(frees[f], held);
                        if (nw > SEED_NODE_WORDS) {
                            // the chosen slots fit the quarter the rule grants: at the need ...
                            CHECK(node_slots_bytes(nl, (size_t)nw, S1) <= quarter, "n %zu nl %zu: slots over the quarter",
                                  ns[i], nl);
                            // ... and at the capacity a new slot gets (from empty, and from a smaller one)
                            for (size_t have : {(size_t)0, nl * (size_t)nw / 2}) {
                                const size_t words = spare_slot_words(nl, (size_t)nw, have, frees[f], S1, true, held);
                                CHECK(slot_holds(words, nl, (size_t)nw) && 3 * words * S1 * 4 <= quarter,
                                      "n %zu nl %zu: a slot of %zu words, quarter %zu", ns[i], nl, words, quarter);
                            }
                        }
                        // the fixed modes ignore memory; a failed query gives seeds
                        CHECK(choose_node_words(FC_NODES_SEEDS, nl, wlw, S1, frees[f], held) == SEED_NODE_WORDS, "seeds");
                        CHECK(choose_node_words(FC_NODES_PAYLOADS, nl, wlw, S1, frees[f], held) == nwp, "payloads");
                        CHECK(choose_node_words(FC_NODES_SEEDS, nl, wlw, S1, std::nullopt, held) == SEED_NODE_WORDS,
                              "seeds, no query");
                        CHECK(choose_node_words(FC_NODES_PAYLOADS, nl, wlw, S1, std::nullopt, held) == nwp,
                              "payloads, no query");
                        CHECK(choose_node_words(FC_NODES_AUTO, nl, wlw, S1, std::nullopt, held) == SEED_NODE_WORDS,
                              "auto with a failed query");
                    }
            auto at = [&](size_t i, size_t j, size_t f) { return choice[(i * NL + j) * NF + f] > SEED_NODE_WORDS; };
            for (size_t i = 0; i < NN; i++)
                for (size_t j = 0; j < NL; j++)
                    for (size_t f = 0; f < NF; f++) {
                        // more free memory never turns payloads into seeds
                        if (f + 1 < NF) CHECK(!at(i, j, f) || at(i, j, f + 1), "free: n %zu nl %zu", ns[i], nls[j]);
                        // more reports or nodes never turn seeds into payloads
                        if (i + 1 < NN) CHECK(at(i, j, f) || !at(i + 1, j, f), "reports: n %zu nl %zu", ns[i], nls[j]);
                        if (j + 1 < NL) CHECK(at(i, j, f) || !at(i, j + 1, f), "nodes: n %zu nl %zu", ns[i], nls[j]);
                    }
        }
    CHECK(n_pay > 1000 && n_seed > 1000, "the grid covers both answers: %d payloads, %d seeds", n_pay, n_seed);
}

int main() {
    check_hits();
    check_capacity();
    check_anchors();
    check_policy();
    printf("capacity cases checked: %zu\n", g_cap_cases);
    printf("policy cases checked: %zu\n", g_policy_cases);
    if (g_failures) {
        printf("memplan_payload_host: %d FAILURES\n", g_failures);
        return 1;
    }
    printf("memplan_payload_host: OK\n");
    return 0;
}
