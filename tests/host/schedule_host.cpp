// Host harness for the launch plan of a prep_init chunk
// (draft-mouris-cfrg-mastic_amd/csrc/schedule.hpp, executed by prep.hpp
// struct Chunk).  Two parts:
//   (a) the level-geometry helpers over a grid of inputs, against values
//       recorded from the helpers' text before it moved into schedule.hpp
//       (WANT_GRID below), and the rows the move's issue listed, one by one;
//   (b) plan_chunk over a grid of trees, fields, modes and knobs: every plan
//       covers each level, proof and sponge byte exactly once, in an order
//       the streams and waits enforce.  The grid spans the whole knob space:
//       every SchedKnobs field that can change a plan is swept
//       (last_level_segments, split_sponges, fuse_proofs, absorb_mode,
//       seg_balance; absorb_single_min through n on either side of it).
// Prints "schedule_host: OK" and returns 0, or one line per failure and 1.
// Run under ASan/UBSan by tests/test_schedule_host.py.
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../draft-mouris-cfrg-mastic_amd/csrc/schedule.hpp"

typedef TreeShape TreeT;

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

static McParams params(int field, int value_len) {
    McParams p{};
    p.field = field;
    p.w32 = field / 32;
    p.enc = field / 8;
    p.value_len = value_len;
    return p;
}

static TreeT tree_of(const std::vector<int>& n_parents) {
    TreeT t;
    t.n_parents = n_parents;
    t.L = (int)n_parents.size() - 1;
    return t;
}

// ---- (a) the helpers' grid (GRID-BEGIN .. GRID-END is what was run over the old text)
// GRID-BEGIN
static std::vector<long> helper_grid() {
    std::vector<long> g;
    SchedKnobs K;
    for (int field : {64, 128})
        for (int vl : {1, 2, 3, 5, 9, 18, 33, 64}) g.push_back(hit_proof_waves(params(field, vl)));
    const int prevs[5][3] = {{0, 1, 0}, {64, 128, 1}, {5000, 10000, 1}, {1, 2, 1}, {100, 101, 1}};
    for (int field : {64, 128})
        for (int vl : {1, 2, 18, 64})
            for (const int* q : prevs) g.push_back(miss_proof_waves(params(field, vl), q[0], q[1], q[2] != 0));
    for (int np : {1, 2, 3, 5, 8, 16, 17, 32})
        for (int nblk : {1, 2, 3, 9, 17, 64}) {
            int split = 0, blocks = 0;
            choose_split(np, np / 2, 8, nblk, &split, &blocks);
            g.push_back(split);
            g.push_back(blocks);
        }
    for (int np : {1, 10, 100, 1000, 10000, 100000})
        for (int groups : {1, 2, 4, 256, 6000}) {
            g.push_back(choose_ppw(np, groups));
            for (int aw : {8, 12}) g.push_back(choose_eval_ppw(np, groups, aw, 256));
        }
    TreeT small = tree_of({1, 2, 4, 8, 16, 24}), big = tree_of(std::vector<int>(32, 1));
    big.n_parents[30] = 5000;
    big.n_parents[31] = 10000;
    for (const TreeT* t : {&small, &big})
        for (int balance = 1; balance >= 0; balance--)
            for (int k = 1; k <= 5; k++) {
                K.seg_balance = balance != 0;
                for (int b : segment_ranges(K, *t, k)) g.push_back(b);
            }
    K.seg_balance = true;
    for (const TreeT* t : {&small, &big})
        for (int forced : {0, 1, 3, 100000})
            for (int groups : {2, 256, 1024}) {
                K.last_level_segments = forced;
                g.push_back(last_level_segments(K, *t, groups, 8));
            }
    return g;
}
// GRID-END

static const long WANT_GRID[] = {
    7, 7, 6, 5, 4, 3, 2, 1, 7, 6, 5, 4, 3, 1, 1, 1, 8, 10, 10, 10, 11, 8, 10, 10,
    10, 11, 3, 5, 5, 5, 6, 1, 2, 2, 2, 2, 8, 10, 10, 10, 11, 7, 8, 8, 8, 10, 2, 3,
    3, 3, 4, 1, 1, 1, 1, 1, 1, 1, 2, 1, 3, 1, 9, 1, 9, 2, 16, 4, 1, 1, 2, 1,
    3, 1, 5, 2, 6, 3, 7, 10, 1, 1, 2, 1, 3, 1, 3, 3, 4, 5, 5, 13, 1, 1, 2, 1,
    2, 2, 2, 5, 2, 9, 3, 22, 1, 1, 1, 2, 1, 3, 3, 3, 3, 6, 5, 13, 1, 1, 1, 2,
    1, 3, 3, 3, 3, 6, 8, 8, 1, 1, 1, 2, 1, 3, 3, 3, 3, 6, 8, 8, 1, 1, 1, 2,
    1, 3, 3, 3, 3, 6, 4, 16, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
    1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 3, 8, 8, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
    13, 9, 36, 13, 9, 1, 1, 1, 1, 1, 1, 1, 1, 1, 15, 25, 42, 64, 63, 42, 1, 1, 1, 1,
    10, 2, 2, 20, 14, 64, 50, 60, 64, 50, 44, 6, 49, 33, 12, 49, 33, 24, 49, 44, 64, 64, 60, 64,
    64, 60, 0, 24, 0, 13, 24, 0, 11, 19, 24, 0, 10, 17, 21, 24, 0, 10, 16, 20, 22, 24, 0, 24,
    0, 12, 24, 0, 8, 16, 24, 0, 6, 12, 18, 24, 0, 5, 10, 14, 19, 24, 0, 10000, 0, 5000, 10000, 0,
    4053, 7338, 10000, 0, 3706, 6454, 8490, 10000, 0, 3545, 6059, 7841, 9104, 10000, 0, 10000, 0, 5000, 10000, 0, 3333, 6667, 10000, 0,
    2500, 5000, 7500, 10000, 0, 2000, 4000, 6000, 8000, 10000, 1, 2, 4, 1, 1, 1, 3, 3, 3, 24, 24, 24, 2, 4,
    4, 1, 1, 1, 3, 3, 3, 10000, 10000, 10000
};

static void check_helpers() {
    const std::vector<long> g = helper_grid();
    const size_t want_n = sizeof WANT_GRID / sizeof WANT_GRID[0];
    CHECK(g.size() == want_n, "grid has %zu values, recorded %zu", g.size(), want_n);
    for (size_t i = 0; i < g.size() && i < want_n; i++)
        CHECK(g[i] == WANT_GRID[i], "grid value %zu is %ld, recorded %ld", i, g[i], WANT_GRID[i]);
    // the rows listed when the helpers moved
    SchedKnobs K;
    CHECK(hit_proof_waves(params(64, 2)) == 7, "-");
    CHECK(hit_proof_waves(params(64, 18)) == 3, "-");
    CHECK(hit_proof_waves(params(128, 64)) == 1, "-");
    CHECK(miss_proof_waves(params(64, 18), 5000, 10000, true) == 5, "-");
    CHECK(miss_proof_waves(params(64, 2), 64, 128, true) == 10, "-");
    CHECK(miss_proof_waves(params(64, 2), 0, 1, false) == 8, "-");
    const int splits[][4] = {{1, 9, 9, 1},   {1, 64, 16, 4}, {2, 9, 5, 2},  {2, 64, 7, 10}, {16, 64, 8, 8},
                             {32, 64, 4, 16}, {32, 9, 3, 3},  {1, 1, 1, 1}, {7, 1, 1, 1},   {32, 1, 1, 1}};
    for (const int* r : splits) {
        int split = 0, blocks = 0;
        choose_split(r[0], r[0] / 2, 8, r[1], &split, &blocks);
        CHECK(split == r[2] && blocks == r[3], "choose_split(%d, nblk %d) = %d x %d", r[0], r[1], split, blocks);
    }
    CHECK(choose_eval_ppw(1000, 256, 8, 256) == 25, "-");
    CHECK(choose_eval_ppw(1000, 256, 12, 256) == 42, "-");
    CHECK(choose_eval_ppw(10000, 256, 8, 256) == 50, "-");
    CHECK(choose_eval_ppw(10000, 256, 12, 256) == 60, "-");
    CHECK(choose_eval_ppw(10000, 4, 8, 256) == 20, "-");
    CHECK(choose_eval_ppw(10000, 4, 12, 256) == 14, "-");
    CHECK(choose_ppw(10000, 256) == 64, "-");
    CHECK(choose_ppw(1000, 256) == 15, "-");
    const TreeT small = tree_of({1, 2, 4, 8, 16, 24});
    TreeT big = tree_of(std::vector<int>(32, 1));
    big.n_parents[30] = 5000;
    big.n_parents[31] = 10000;
    CHECK(segment_ranges(K, small, 2) == (std::vector<int>{0, 13, 24}), "-");
    CHECK(segment_ranges(K, small, 3) == (std::vector<int>{0, 11, 19, 24}), "-");
    CHECK(segment_ranges(K, small, 4) == (std::vector<int>{0, 10, 17, 21, 24}), "-");
    CHECK(segment_ranges(K, big, 4) == (std::vector<int>{0, 3706, 6454, 8490, 10000}), "-");
    K.seg_balance = false;
    CHECK(segment_ranges(K, small, 3) == (std::vector<int>{0, 8, 16, 24}), "-");
}

// ---- (b) plan invariants
struct Case {
    SchedKnobs K;
    McParams p;
    TreeT t;
    int n;
    bool hit, cache, pipelined;
    std::string name;
};

static bool legal_variant(int v) {
    for (int w : LEVEL_VARIANTS)
        if (v == w) return true;
    return false;
}

static void check_plan(const Case& c) {
    const int F_OH = 37, F_PL = 101;  // fill positions after the prefixes (any values below the rate)
    ChunkPlan P;
    plan_chunk(c.K, c.p, c.t, c.n, c.hit, c.cache, c.pipelined, F_OH, F_PL, &P);
    const char* nm = c.name.c_str();
    const int L = c.t.L, lo = c.hit ? L : 0, wlw = c.p.value_len * c.p.w32;
    const std::vector<int>& np = c.t.n_parents;
    const int n_launch = (int)P.launches.size(), n_sponge = (int)P.sponges.size();

    // levels: the launches' parent ranges partition each evaluated level once, in order
    std::vector<std::vector<int>> made(L + 1);   // per level and parent: the launch that evaluates it
    {
        int level = lo, next = 0;
        for (int j = 0; j < n_launch; j++) {
            const LevelLaunch& a = P.launches[j];
            if (next == np[level] && level < L) level++, next = 0;
            CHECK(a.level == level && a.p0 == next && a.cnt > 0, "%s: launch %d is level %d [%d, +%d)", nm, j, a.level,
                  a.p0, a.cnt);
            next = a.p0 + a.cnt;
            if (a.level >= lo && a.level <= L) made[a.level].resize(std::max(0, std::min(next, np[a.level])), j);
            CHECK(legal_variant(a.variant), "%s: launch %d variant %d", nm, j, a.variant);
            const bool fc = (c.cache && (c.hit || a.level == L)) || a.fuse_proofs > 0;
            CHECK(((a.variant & LV_FC) != 0) == fc, "%s: launch %d FC", nm, j);
            if (!fc) {
                CHECK(((a.variant & LV_WIDE) != 0) == P.wide, "%s: launch %d WIDE", nm, j);
                CHECK(((a.variant & LV_SPLIT) != 0) == (a.split > 1), "%s: launch %d SPLIT", nm, j);
                CHECK(((a.variant & LV_GEN) != 0) == (a.level == 0 || a.level == L), "%s: launch %d GEN", nm, j);
            }
            CHECK(a.split == 1 || (a.gy == 1 && a.level < L && !c.hit && np[a.level] <= 32), "%s: split launch %d", nm,
                  j);
            CHECK(a.aes_waves >= 1 && a.aes_waves < SCHED_EVAL_WAVES && a.ppw >= 1 && a.gy >= 1 &&
                      (long)a.gy * a.par_waves * a.ppw >= (long)a.cnt * a.split,
                  "%s: launch %d geometry", nm, j);
            // ring slots: the first launch of level l >= NSLOT of a miss waits for level l - NSLOT's sponges
            const bool first = a.p0 == 0;
            CHECK(a.wait_level == ((!c.hit && first && a.level >= NSLOT) ? a.level - NSLOT : -1), "%s: launch %d waits %d",
                  nm, j, a.wait_level);
        }
        CHECK(level == L && next == np[L], "%s: launches end at level %d parent %d", nm, level, next);
        if (c.hit) CHECK(n_launch == 1 && n_sponge <= 2, "%s: a hit plans %d launches", nm, n_launch);
    }
    if (g_failures) return;

    // proofs: every node of every evaluated level once; `proved` = the step that makes it
    std::vector<std::vector<int>> proved(L + 1);
    for (int l = lo; l <= L; l++) proved[l].assign(2 * np[l], -1);
    auto prove = [&](int level, int node0, int nodes, int step) {
        for (int v = node0; v < node0 + nodes; v++) {
            const bool in = level >= lo && level <= L && v >= 0 && v < 2 * np[level];
            CHECK(in && proved[level][v] < 0, "%s: step %d proves level %d node %d again or out of range", nm, step, level, v);
            if (!in) return;
            proved[level][v] = step;
            // the node's seed comes from an earlier launch (or, fused, from this one)
            CHECK(made[level][v / 2] < step || (made[level][v / 2] == step && P.launches[step].fuse_proofs > 0),
                  "%s: step %d proves level %d node %d before launch %d made it", nm, step, level, v, made[level][v / 2]);
        }
    };
    for (int j = 0; j < n_launch; j++) {
        const LevelLaunch& a = P.launches[j];
        if (a.pv_nodes > 0) {
            prove(a.pv_level, a.pv_node0, a.pv_nodes, j);
            const int pw = SCHED_EVAL_WAVES - a.aes_waves;
            CHECK((long)a.pv_npw * a.gy * pw >= a.pv_nodes, "%s: launch %d proof waves", nm, j);
        }
        if (a.fuse_proofs > 0) prove(a.level, 2 * a.p0, 2 * a.cnt, j);
    }
    CHECK(P.fuse_last == (P.final_nn == 0), "%s: final step", nm);
    prove(L, P.final_n0, P.final_nn, n_launch);
    for (int l = c.hit ? L : 0; l <= L; l++)
        for (int v = 0; v < 2 * np[l]; v++) CHECK(proved[l][v] >= 0, "%s: level %d node %d has no proof", nm, l, v);
    if (g_failures) return;

    // sponges: per sponge the pieces are contiguous, in BFS order, cover the
    // evaluated levels once, enter at the bytes absorbed so far, run after
    // the step that makes their input and after the sponge's previous piece
    long bytes[2] = {F_OH, F_PL};
    for (int l = 0; l < lo; l++) bytes[0] += 2 * np[l] * 32, bytes[1] += l > 0 ? np[l] * wlw * 4 : 0;
    int level[2] = {lo, lo}, next[2] = {0, 0}, prev[2] = {-1, -1}, pieces = 0;
    std::vector<std::vector<int>> last_piece(2, std::vector<int>(L + 1, -1));  // by sponge and level
    int sp = 0;
    for (int step = 0; step <= n_launch; step++) {
        const int sp1 = step < n_launch ? P.launches[step].sp1 : n_sponge;
        CHECK((step < n_launch ? P.launches[step].sp0 : n_sponge - 1) == sp, "%s: step %d sponges start at %d", nm, step, sp);
        for (; sp < sp1; sp++) {
            const SpongeLaunch& s = P.sponges[sp];
            CHECK(s.after == step && s.which0 >= 0 && s.nwh >= 1 && s.which0 + s.nwh <= 2, "%s: sponge %d", nm, sp);
            CHECK(s.f_oh == bytes[0] % SCHED_SPONGE_RATE && s.f_pl == bytes[1] % SCHED_SPONGE_RATE,
                  "%s: sponge %d enters at %d, %d", nm, sp, s.f_oh, s.f_pl);
            pieces += s.marks == MK_PIECE;
            bool needs_prev = false;
            for (int w = s.which0; w < s.which0 + s.nwh; w++) {
                const int unit = w ? 1 : 2, limit = unit * np[level[w]];  // nodes / parents of a level
                if (next[w] == limit && level[w] < L) level[w]++, next[w] = 0;
                if (w == 1 && level[w] == 0 && next[w] == 0 && s.level > 0) level[w] = 1;  // level 0 has no payload bytes
                const int first = w ? s.piece.parent0 : s.piece.node0, count = w ? s.piece.parents : s.piece.nodes;
                CHECK(s.level == level[w] && first == next[w] && count > 0 && first + count <= unit * np[s.level],
                      "%s: sponge %d (%d) is level %d [%d, +%d), expected level %d from %d", nm, sp, w, s.level, first,
                      count, level[w], next[w]);
                if (g_failures) return;
                next[w] = first + count;
                bytes[w] += w ? (s.level > 0 ? count * wlw * 4 : 0) : count * 32;
                // its input: proofs (one-hot) / payload differences of the parents' launch (payload)
                for (int v = first; v < first + count; v++)
                    CHECK((w ? made[s.level][v] : proved[s.level][v]) <= step, "%s: sponge %d (%d) runs before step %d", nm,
                          sp, w, w ? made[s.level][v] : proved[s.level][v]);
                if (prev[w] >= 0 && P.sponges[prev[w]].stream != s.stream) {
                    needs_prev = true;
                    CHECK(s.prev == prev[w], "%s: sponge %d (%d) follows %d, waits for %d", nm, sp, w, prev[w], s.prev);
                }
                prev[w] = sp;
                last_piece[w][s.level] = sp;
            }
            if (!needs_prev) CHECK(s.prev == -1, "%s: sponge %d waits for %d", nm, sp, s.prev);
            CHECK(s.stream == ST_MAIN || s.stream == ST_SPONGE || (s.stream == ST_THIRD && !c.pipelined),
                  "%s: sponge %d on stream %d", nm, sp, s.stream);
        }
        // a launch that waits for a ring slot: every piece of that level's sponges was issued before it
        if (step + 1 < n_launch && P.launches[step + 1].wait_level >= 0) {
            const int wl = P.launches[step + 1].wait_level;
            for (int w = 0; w < 2; w++)
                CHECK(level[w] > wl || (level[w] == wl && next[w] == (w ? 1 : 2) * np[wl]),
                      "%s: launch %d reuses level %d's slot before sponge %d is through", nm, step + 1, wl, w);
        }
    }
    for (int w = 0; w < (L > 0 ? 2 : 1); w++)
        CHECK(level[w] == L && next[w] == (w ? 1 : 2) * np[L], "%s: sponge %d ends at level %d, %d", nm, w, level[w], next[w]);
    // closed-form totals
    long tot_oh = F_OH, tot_pl = F_PL;
    for (int l = 0; l <= L; l++) tot_oh += 64L * np[l], tot_pl += l > 0 ? 4L * np[l] * wlw : 0;
    CHECK(P.f_oh == tot_oh % SCHED_SPONGE_RATE && P.f_pl == tot_pl % SCHED_SPONGE_RATE, "%s: final fill %d, %d", nm, P.f_oh,
          P.f_pl);
    CHECK(P.sponges.back().stream == P.last_stream, "%s: last sponge's stream", nm);
    CHECK(2 + P.n_timing == 2 + 6 * (n_launch + 1 + pieces), "%s: %d timing events", nm, P.n_timing);
    CHECK(P.n_sync == n_launch + n_sponge + 1 + (c.t.weight_check ? 2 : 0), "%s: %d sync events", nm, P.n_sync);
    // the call-wide choices
    CHECK(P.nseg >= 1 && P.nseg <= np[L] && (P.nseg == 1 || (!c.hit && !c.cache && !c.pipelined && P.pair && !P.fuse_last)),
          "%s: %d segments", nm, P.nseg);
    CHECK(!P.split || (!c.hit && !c.pipelined), "%s: split", nm);
    CHECK(P.wide == P.pair, "%s: wide", nm);
}

static int check_plans() {
    int n_plans = 0;
    for (int L : {0, 1, 2, 3, 5, 7})
        for (int big = 0; big < 2; big++) {
            // all levels <= 32 parents (every level but the last is a split level), or a level above 32
            std::vector<int> np;
            for (int l = 0; l <= L; l++) np.push_back(l == 0 ? 1 : big ? 20 * l + 25 : std::min(1 << l, 3 * l + 1));
            for (int field : {64, 128})
                for (int mode = 0; mode < 3; mode++)  // miss without cache, miss with cache, hit
                    for (int pipelined = 0; pipelined < 2; pipelined++)
                        for (int segs : {0, 1, 3, 1000})
                            for (int split : {-1, 0, 1})
                                for (int fuse : {0, 1})
                                    for (int absorb : {0, 1, 2})
                                        for (int balance : {0, 1})
                                            for (int n : {70, 100000})
                                                for (int wc = 0; wc < 2; wc++) {
                                                    if (mode == 2 && (L == 0 || wc)) continue;  // no hit at level 0 or with the FLP
                                                    Case c;
                                                    c.K.last_level_segments = segs;
                                                    c.K.split_sponges = split;
                                                    c.K.fuse_proofs = fuse != 0;
                                                    c.K.absorb_mode = absorb;
                                                    c.K.seg_balance = balance != 0;
                                                    c.p = params(field, field == 64 ? 2 : 18);
                                                    c.t = tree_of(np);
                                                    c.t.weight_check = wc != 0;
                                                    c.n = n;
                                                    c.hit = mode == 2;
                                                    c.cache = mode >= 1;
                                                    c.pipelined = pipelined != 0;
                                                    char buf[200];
                                                    snprintf(buf, sizeof buf,
                                                             "L%d big%d F%d mode%d pipe%d seg%d split%d fuse%d abs%d bal%d n%d wc%d", L,
                                                             big, field, mode, pipelined, segs, split, fuse, absorb, balance, n, wc);
                                                    c.name = buf;
                                                    check_plan(c);
                                                    n_plans++;
                                                    if (g_failures) return n_plans;
                                                }
        }
    return n_plans;
}

int main() {
    check_helpers();
    const int n_plans = g_failures ? 0 : check_plans();
    if (g_failures) {
        printf("schedule_host: %d failures\n", g_failures);
        return 1;
    }
    printf("plans checked: %d\n", n_plans);
    printf("schedule_host: OK\n");
    return 0;
}
