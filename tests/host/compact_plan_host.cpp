// csrc/compact_plan.hpp on the host (built with -fsanitize=address,undefined by
// tests/test_compact_plan_host.py).  Every plan is executed on a byte array
// with launch semantics: a launch reads all its source rows, then writes all
// its destination rows, and within a launch any order of rows must give the
// same result, so the rows a launch reads and the rows it writes have to be
// disjoint.  Checked per plan: that disjointness; no launch reads a row an
// earlier launch overwrote (every row is read while it still holds what was
// uploaded); the result equals the reference filter; the identity prefix is
// never written; staging rows and launch count stay within their bounds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../draft-mouris-cfrg-mastic_amd/csrc/compact_plan.hpp"

static long g_plans = 0;

#define REQUIRE(cond, ...)                                  \
    do {                                                    \
        if (!(cond)) {                                      \
            fprintf(stderr, "FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, "\n");                          \
            exit(1);                                        \
        }                                                   \
    } while (0)

// One plan: the mask, rows of `rb` bytes, staging of S rows.
static void run_plan(const std::vector<uint8_t>& keep, size_t rb, size_t S, const char* what) {
    const size_t n = keep.size();
    std::vector<uint8_t> seg(n * rb), orig;
    for (size_t i = 0; i < n; i++)
        for (size_t b = 0; b < rb; b++) seg[i * rb + b] = (uint8_t)(i * 131 + b * 7 + (i >> 8));
    orig = seg;
    // reference filter
    std::vector<uint8_t> want;
    std::vector<uint32_t> want_src;
    for (size_t i = 0; i < n; i++)
        if (keep[i]) {
            want.insert(want.end(), orig.begin() + i * rb, orig.begin() + (i + 1) * rb);
            want_src.push_back((uint32_t)i);
        }
    const CompactIndex ix = compact_index(keep.data(), n);
    REQUIRE(ix.n_kept == want_src.size() && ix.src == want_src, "%s n=%zu: index", what, n);
    size_t prefix = 0;
    while (prefix < n && keep[prefix]) prefix++;
    REQUIRE(ix.prefix == prefix, "%s n=%zu: prefix %zu", what, n, ix.prefix);
    for (size_t j = 0; j + 1 < ix.n_kept; j++)
        REQUIRE(ix.src[j + 1] - (j + 1) >= ix.src[j] - j, "%s: the gap decreases at %zu", what, j);

    const std::vector<CompactLaunch> plan = compact_launches(ix, S);
    REQUIRE(plan.size() <= compact_launch_bound(ix.moved(), S), "%s n=%zu S=%zu: %zu launches, bound %zu", what, n, S,
            plan.size(), compact_launch_bound(ix.moved(), S));
    if (ix.moved() == 0) REQUIRE(plan.empty(), "%s: launches though nothing moves", what);

    std::vector<uint8_t> stage(S * rb, 0xEE);
    std::vector<uint8_t> dirty(n, 0);  // row overwritten by an earlier launch
    std::vector<uint8_t> rd(n), wr(n);
    size_t next = ix.prefix;  // the tiles cover the moved rows in order, each once
    bool staged_pending = false;
    size_t pend_first = 0, pend_count = 0;
    for (const CompactLaunch& l : plan) {
        REQUIRE(l.count > 0, "%s: empty launch", what);
        std::fill(rd.begin(), rd.end(), 0);
        std::fill(wr.begin(), wr.end(), 0);
        if (l.op == CP_COPY_BACK) {
            REQUIRE(staged_pending && l.first == pend_first && l.count == pend_count, "%s: copy without its gather", what);
            staged_pending = false;
            for (size_t r = 0; r < l.count; r++) {
                const size_t d = l.first + r;
                REQUIRE(d >= ix.prefix && d < ix.n_kept, "%s: copy writes row %zu", what, d);
                wr[d] = 1;
            }
            memcpy(&seg[l.first * rb], stage.data(), l.count * rb);
        } else {
            REQUIRE(!staged_pending, "%s: a staged gather was not copied back", what);
            REQUIRE(l.first == next && l.first + l.count <= ix.n_kept, "%s: tile [%zu,+%zu) out of order", what, l.first,
                    l.count);
            next += l.count;
            const bool direct = l.op == CP_GATHER_DIRECT;
            if (!direct) REQUIRE(l.count <= S, "%s: %zu rows in a staging buffer of %zu", what, l.count, S);
            // all reads first (into a scratch), then all writes: launch semantics
            std::vector<uint8_t> tmp(l.count * rb);
            for (size_t r = 0; r < l.count; r++) {
                const size_t s = ix.src[l.first + r];
                REQUIRE(s < n, "%s: source row %zu", what, s);
                REQUIRE(!dirty[s], "%s n=%zu S=%zu: row %zu is read after an earlier launch overwrote it", what, n, S, s);
                rd[s] = 1;
                memcpy(&tmp[r * rb], &seg[s * rb], rb);
            }
            for (size_t r = 0; r < l.count; r++) {
                if (direct) {
                    const size_t d = l.first + r;
                    REQUIRE(d >= ix.prefix, "%s: the identity prefix is written (row %zu)", what, d);
                    wr[d] = 1;
                    memcpy(&seg[d * rb], &tmp[r * rb], rb);
                } else
                    memcpy(&stage[r * rb], &tmp[r * rb], rb);
            }
            if (!direct) {
                staged_pending = true;
                pend_first = l.first;
                pend_count = l.count;
            }
        }
        for (size_t i = 0; i < n; i++) {
            REQUIRE(!(rd[i] && wr[i]), "%s n=%zu S=%zu: row %zu is read and written by one launch", what, n, S, i);
            if (wr[i]) dirty[i] = 1;
        }
    }
    REQUIRE(!staged_pending, "%s: the last staged gather was not copied back", what);
    REQUIRE(next == ix.n_kept, "%s: rows %zu..%zu were never moved", what, next, ix.n_kept);
    REQUIRE(want.empty() || memcmp(seg.data(), want.data(), want.size()) == 0, "%s n=%zu S=%zu: result differs from the filter", what, n, S);
    for (size_t i = 0; i < ix.prefix; i++) REQUIRE(!dirty[i], "%s: prefix row %zu written", what, i);
    g_plans++;
}

static void run_mask(const std::vector<uint8_t>& keep, const char* what) {
    const size_t n = keep.size();
    const size_t stagings[] = {1, 2, 3, 7, 64, n / 3 + 1, n + 5};
    for (size_t S : stagings) run_plan(keep, 3, S, what);
    run_plan(keep, 1, 5, what);
    run_plan(keep, 17, 1, what);
}

int main() {
    std::mt19937_64 rng(20240611);
    const size_t sizes[] = {0, 1, 2, 3, 63, 64, 65, 257, 1000, 4099};
    for (size_t n : sizes) {
        std::vector<uint8_t> k(n);
        std::fill(k.begin(), k.end(), 1);
        run_mask(k, "all kept");
        std::fill(k.begin(), k.end(), 0);
        run_mask(k, "none kept");
        if (n) {
            std::fill(k.begin(), k.end(), 1);
            k[0] = 0;
            run_mask(k, "only the first dropped");
            std::fill(k.begin(), k.end(), 0);
            k[n - 1] = 1;
            run_mask(k, "only the last kept");
            std::fill(k.begin(), k.end(), 1);
            k[n - 1] = 0;
            run_mask(k, "only the last dropped");
        }
        for (int ph = 0; ph < 2; ph++) {
            for (size_t i = 0; i < n; i++) k[i] = (i & 1) == (size_t)ph;
            run_mask(k, "alternating");
        }
        if (n >= 3) {
            // a dropped run inside a kept run, at several places and lengths
            for (size_t at : {size_t(1), n / 3, n / 2, n - 2})
                for (size_t len : {size_t(1), size_t(2), n / 5 + 1}) {
                    std::fill(k.begin(), k.end(), 1);
                    for (size_t i = at; i < std::min(n, at + len); i++) k[i] = 0;
                    run_mask(k, "a dropped run inside a kept run");
                }
        }
        for (int pct : {1, 10, 50, 90, 99})
            for (int rep = 0; rep < 12; rep++) {
                for (size_t i = 0; i < n; i++) k[i] = (int)(rng() % 100) < pct;
                run_mask(k, "random");
            }
    }
    // the staging size rule
    REQUIRE(compact_staging_bytes(0, 100, 1u << 30) == CompactKnobs::default_staging_bytes, "default staging");
    REQUIRE(compact_staging_bytes(1, 579, 1000) == 579, "staging is clamped up to one row");
    REQUIRE(compact_staging_bytes(1u << 20, 100, 7) == 700, "staging is no larger than the rows that move");
    REQUIRE(compact_stage_rows(579, 579) == 1 && compact_stage_rows(579, 16) == 36 && compact_stage_rows(3, 16) == 1,
            "staging rows");
    printf("plans checked: %ld\n", g_plans);
    printf("compact_plan_host: OK\n");
    return 0;
}
