// csrc/group_fold.hpp on the host (tests/test_group_fold_host.py builds the
// host side of this file with ASan / UBSan; csrc/field.hpp needs the HIP
// headers, so the compiler is hipcc and the sanitizers go to -Xarch_host):
//  * limbs_to_elem<F> for both fields against the sum formed by repeated
//    F::add (random elements, every word 0xFFFFFFFF, p-1 repeated) and, for
//    counts of 1, 2^16 and 2^31-1 equal elements, against count * x formed
//    with F::mul (the word sums S_i = count * word_i are formed
//    arithmetically, not by looping);
//  * check_groups: the sentinel, the first bad index, counts with and
//    without a mask;
//  * plan_group_fold over a grid of shapes: the invariants the library and
//    k_fold_grouped rely on, and a replay of the kernel's own indexing
//    (every group in exactly one pass, every report in exactly one chunk);
//  * plan_fold (the ungrouped fold) against a table of the values its
//    expression returned before it moved out of the executor, and its
//    invariants.
// Prints "plans checked: N", "fold plans checked: N" and "group_fold_host: OK".
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../draft-mouris-cfrg-mastic_amd/csrc/field.hpp"
#include "../../draft-mouris-cfrg-mastic_amd/csrc/group_fold.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static std::mt19937_64 rng(20240607);

template <class F> typename F::E p_minus_1();
template <> uint64_t p_minus_1<F64>() { return F64::P - 1; }
template <> F128::E p_minus_1<F128>() { return F128::E{F128::P_LO - 1, F128::P_HI}; }

// a canonical element from raw words (all-ones words are >= p: reduced as the
// kernel never has to, since out shares are canonical; the word sums below are
// taken from the raw words all the same, limbs_to_elem does not care)
template <class F> typename F::E random_elem() {
    for (;;) {
        uint32_t w[4];
        for (auto& x : w) x = (uint32_t)rng();
        const typename F::E e = F::from_words(w);
        if (F::valid(e)) return e;
    }
}

template <class F> void add_words(uint64_t* s, typename F::E x) {
    for (int i = 0; i < F::W32; i++) s[i] += F::word(x, i);
}

template <class F> void check_limbs(const char* name) {
    typedef typename F::E E;
    // random elements: integer word sums against repeated F::add
    for (int count : {1, 2, 3, 64, 1000, 65536}) {
        uint64_t s[4] = {0, 0, 0, 0};
        E want = F::zero();
        for (int k = 0; k < count; k++) {
            const E x = random_elem<F>();
            add_words<F>(s, x);
            want = F::add(want, x);
        }
        CHECK(F::eq(limbs_to_elem<F>(s), want));
    }
    // p-1 repeated, by looping (2^16) ...
    {
        uint64_t s[4] = {0, 0, 0, 0};
        E want = F::zero();
        for (int k = 0; k < 65536; k++) {
            add_words<F>(s, p_minus_1<F>());
            want = F::add(want, p_minus_1<F>());
        }
        CHECK(F::eq(limbs_to_elem<F>(s), want));
    }
    // ... and arithmetically: S_i = count * word_i, expected count * x mod p
    const uint64_t counts[] = {1, (uint64_t)1 << 16, ((uint64_t)1 << 31) - 1};
    std::vector<E> xs = {p_minus_1<F>(), F::from_u64(1), F::zero(), random_elem<F>(), random_elem<F>()};
    for (uint64_t count : counts)
        for (const E& x : xs) {
            uint64_t s[4] = {0, 0, 0, 0};
            for (int i = 0; i < F::W32; i++) s[i] = count * (uint64_t)F::word(x, i);
            CHECK(F::eq(limbs_to_elem<F>(s), F::mul(F::from_u64(count), x)));
        }
    // every word 0xFFFFFFFF (the largest word sums a chunk can reach): the
    // integer sum_i S_i 2^(32 i) = count * (2^(32 W32) - 1), and
    // 2^(32 W32) - 1 mod p is the field's own constant
    for (uint64_t count : counts) {
        uint64_t s[4];
        for (int i = 0; i < F::W32; i++) s[i] = count * 0xFFFFFFFFull;
        CHECK(s[0] < ((uint64_t)1 << 63));
        uint32_t ones[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        // (2^(32 W32) - 1) mod p by Horner over the words with F arithmetic on single words
        E all = F::zero();
        for (int i = F::W32 - 1; i >= 0; i--)
            all = F::add(F::mul(all, F::from_u64((uint64_t)1 << 32)), F::from_u64(ones[i]));
        CHECK(F::eq(limbs_to_elem<F>(s), F::mul(F::from_u64(count), all)));
    }
    // the all-ones constant against the closed forms: 2^64 - 1 = 2^32 - 2 mod p64,
    // 2^128 - 1 = 28 * 2^64 - 2 mod p128
    {
        uint64_t s[4] = {0xFFFFFFFFull, 0xFFFFFFFFull, 0xFFFFFFFFull, 0xFFFFFFFFull};
        const E got = limbs_to_elem<F>(s);
        if (F::W32 == 2) CHECK(F::word(got, 0) == 0xFFFFFFFEu && F::word(got, 1) == 0);
        else CHECK(F::word(got, 0) == 0xFFFFFFFEu && F::word(got, 1) == 0xFFFFFFFFu && F::word(got, 2) == 27 &&
                   F::word(got, 3) == 0);
    }
    printf("limbs_to_elem %s: ok\n", name);
}

static void check_ids() {
    const uint32_t NONE = MASTIC_GROUP_NONE;
    {
        const uint32_t g[] = {0, 2, NONE, 2, 1, 2, NONE, 0};
        const uint8_t v[] = {1, 0, 1, 1, 1, 7, 0, 0};
        uint64_t c[3] = {9, 9, 9};
        CHECK(check_groups(g, 8, 3, nullptr, c) == -1);
        CHECK(c[0] == 2 && c[1] == 1 && c[2] == 3);
        CHECK(check_groups(g, 8, 3, v, c) == -1);
        CHECK(c[0] == 1 && c[1] == 1 && c[2] == 2);
        CHECK(check_groups(g, 8, 3, v, nullptr) == -1);
        CHECK(check_groups(g, 8, 2, nullptr, nullptr) == 1);  // the first id >= n_groups
        CHECK(check_groups(g, 1, 2, nullptr, nullptr) == -1);
    }
    {
        const uint32_t g[] = {0, 1, 5, 7, NONE};
        uint64_t c[5];
        CHECK(check_groups(g, 5, 5, nullptr, c) == 2);  // an id equal to n_groups
        const uint8_t v[] = {1, 1, 0, 1, 1};
        CHECK(check_groups(g, 5, 5, v, c) == 2);        // a masked report's id is checked too
        CHECK(check_groups(g, 5, 8, nullptr, nullptr) == -1);
        CHECK(check_groups(g, 5, MASTIC_MAX_GROUPS, nullptr, nullptr) == -1);
    }
    {
        uint64_t c[2] = {5, 5};
        CHECK(check_groups(nullptr, 0, 2, nullptr, c) == -1 && c[0] == 0 && c[1] == 0);
        const uint32_t g[] = {NONE, NONE};
        CHECK(check_groups(g, 2, 1, nullptr, c) == -1 && c[0] == 0);
    }
    printf("check_groups: ok\n");
}

static size_t check_plans() {
    const int w32s[] = {2, 4};
    const size_t ns[] = {0, 1, 63, 64, 255, 256, 257, 8191, 8192, (size_t)1 << 20};
    const size_t rowss[] = {1, 10, 700, 20000};
    const size_t Gs[] = {1, 2, 63, 64, 65, 4096, 4097, 65536};
    const size_t lds_budgets[] = {0, (size_t)16 << 10, (size_t)64 << 10};
    const size_t part_budgets[] = {0, (size_t)1 << 20};
    size_t checked = 0, multi_chunk = 0, multi_pass = 0;
    for (int w32 : w32s)
        for (size_t n : ns)
            for (size_t rows : rowss)
                for (size_t G : Gs)
                    for (size_t lb : lds_budgets)
                        for (size_t pb : part_budgets) {
                            if (G * rows > (size_t)INT_MAX) continue;  // the library refuses these
                            const GroupFoldPlan pl = plan_group_fold(w32, n, rows, G, 256, lb, pb);
                            const size_t lds = lb ? lb : GroupFoldKnobs::default_lds_budget;
                            const size_t part = pb ? pb : GroupFoldKnobs::default_partial_budget;
                            const size_t gpp = pl.groups_per_pass;
                            CHECK(gpp >= 1 && pl.passes >= 1);
                            CHECK((size_t)pl.passes * gpp >= G);
                            CHECK((size_t)(pl.passes - 1) * gpp < G);  // no empty pass
                            // every group in exactly one pass, by the kernel's own test (g - g0 < gpp)
                            for (size_t g : {(size_t)0, G / 2, G - 1}) {
                                int hits = 0;
                                for (uint32_t k = 0; k < pl.passes; k++) {
                                    const uint32_t g0 = k * pl.groups_per_pass;
                                    const uint32_t in_pass = (uint32_t)std::min<size_t>(gpp, G - g0);
                                    hits += (uint32_t)g - g0 < in_pass;
                                    CHECK(MASTIC_GROUP_NONE - g0 >= in_pass);
                                }
                                CHECK(hits == 1);
                            }
                            CHECK(pl.copies >= 1 && pl.copies <= 16 && (pl.copies & (pl.copies - 1)) == 0);
                            CHECK(pl.lds_bytes == (size_t)pl.copies * gpp * w32 * 8);
                            CHECK(pl.lds_bytes <= lds && pl.lds_bytes <= ((size_t)64 << 10));
                            CHECK(pl.chunk % 256 == 0 && pl.chunk > 0);
                            CHECK((size_t)pl.chunks * pl.chunk >= n);
                            if (n) {
                                CHECK(pl.chunks >= 1);
                                CHECK((size_t)(pl.chunks - 1) * pl.chunk < n);  // no empty chunk
                                CHECK(pl.grid_x == rows && pl.grid_y == pl.chunks);
                            } else {
                                CHECK(pl.chunks == 0);
                            }
                            CHECK(pl.grid_y <= 65535);
                            CHECK((size_t)std::max<uint32_t>(pl.chunks, 1) * gpp * rows <= (size_t)INT_MAX);
                            if (pl.chunks > 1) {
                                CHECK(pl.partial_bytes == (size_t)pl.chunks * gpp * rows * w32 * 4);
                                CHECK(pl.partial_bytes <= part);
                                // a chunk's partials are small beside what it reads
                                CHECK(pl.chunk >= GroupFoldKnobs::chunk_per_group * gpp || pl.chunks == 1);
                            } else {
                                CHECK(pl.partial_bytes == 0);  // written in place
                            }
                            checked++;
                            multi_chunk += pl.chunks > 1;
                            multi_pass += pl.passes > 1;
                        }
    CHECK(multi_chunk > 0 && multi_pass > 0);
    // the shapes the design quotes
    {
        const GroupFoldPlan a = plan_group_fold(2, 16384, 20000, 8, 256, 0, 0);
        CHECK(a.passes == 1 && a.chunks == 1 && a.copies == 16 && a.lds_bytes == 2048);
        const GroupFoldPlan b = plan_group_fold(2, (size_t)1 << 20, 700, 64, 256, 0, 0);
        CHECK(b.passes == 1 && b.chunks > 1 && b.copies == 16);
        const GroupFoldPlan c = plan_group_fold(2, 150, 10, 65536, 256, 0, 0);
        CHECK(c.passes == 16 && c.groups_per_pass == 4096 && c.copies == 1);
        const GroupFoldPlan d = plan_group_fold(4, 150, 20, 65536, 256, 0, 0);
        CHECK(d.passes == 32 && d.groups_per_pass == 2048);
        const GroupFoldPlan e = plan_group_fold(2, 8453, 10, 3, 256, 0, 0);
        CHECK(e.chunks == 2);  // tests/test_gpu_aggregate_grouped.py relies on it
        const GroupFoldPlan f = plan_group_fold(4, 8453, 20, 64, 256, 0, 0);
        CHECK(f.chunks == 2);
    }
    return checked;
}

// plan_fold (the ungrouped fold's chunking) pinned to the values the expression
// returned while it stood inline in aggregate_impl (recorded from that code
// before the move, not from plan_fold): n_cus, n, rows -> chunks, chunk, and
// the partials buffer for Field64 / Field128.  The last two rows (a chip that
// does not exist) are where the partials pass their 1 MiB floor.
static size_t check_fold_plans() {
    static const struct {
        int n_cus;
        size_t n, rows, chunks, chunk, part2, part4;
    } want[] = {
        {256, 0, 1, 1, 1, 0, 0},
        {256, 0, 10, 1, 1, 0, 0},
        {256, 0, 20, 1, 1, 0, 0},
        {256, 0, 700, 1, 1, 0, 0},
        {256, 0, 4095, 1, 1, 0, 0},
        {256, 0, 4096, 1, 1, 0, 0},
        {256, 0, 20000, 1, 1, 0, 0},
        {256, 1, 1, 1, 1, 0, 0},
        {256, 1, 10, 1, 1, 0, 0},
        {256, 1, 20, 1, 1, 0, 0},
        {256, 1, 700, 1, 1, 0, 0},
        {256, 1, 4095, 1, 1, 0, 0},
        {256, 1, 4096, 1, 1, 0, 0},
        {256, 1, 20000, 1, 1, 0, 0},
        {256, 8191, 1, 1, 8191, 0, 0},
        {256, 8191, 10, 1, 8191, 0, 0},
        {256, 8191, 20, 1, 8191, 0, 0},
        {256, 8191, 700, 1, 8191, 0, 0},
        {256, 8191, 4095, 1, 8191, 0, 0},
        {256, 8191, 4096, 1, 8191, 0, 0},
        {256, 8191, 20000, 1, 8191, 0, 0},
        {256, 8192, 1, 2, 4096, 1048576, 1048576},
        {256, 8192, 10, 2, 4096, 1048576, 1048576},
        {256, 8192, 20, 2, 4096, 1048576, 1048576},
        {256, 8192, 700, 2, 4096, 1048576, 1048576},
        {256, 8192, 4095, 2, 4096, 1048576, 1048576},
        {256, 8192, 4096, 1, 8192, 0, 0},
        {256, 8192, 20000, 1, 8192, 0, 0},
        {256, 8453, 1, 2, 4352, 1048576, 1048576},
        {256, 8453, 10, 2, 4352, 1048576, 1048576},
        {256, 8453, 20, 2, 4352, 1048576, 1048576},
        {256, 8453, 700, 2, 4352, 1048576, 1048576},
        {256, 8453, 4095, 2, 4352, 1048576, 1048576},
        {256, 8453, 4096, 1, 8453, 0, 0},
        {256, 8453, 20000, 1, 8453, 0, 0},
        {256, 16384, 1, 4, 4096, 1048576, 1048576},
        {256, 16384, 10, 4, 4096, 1048576, 1048576},
        {256, 16384, 20, 4, 4096, 1048576, 1048576},
        {256, 16384, 700, 4, 4096, 1048576, 1048576},
        {256, 16384, 4095, 2, 8192, 1048576, 1048576},
        {256, 16384, 4096, 1, 16384, 0, 0},
        {256, 16384, 20000, 1, 16384, 0, 0},
        {256, 1048576, 1, 256, 4096, 1048576, 1048576},
        {256, 1048576, 10, 256, 4096, 1048576, 1048576},
        {256, 1048576, 20, 205, 5120, 1048576, 1048576},
        {256, 1048576, 700, 6, 174848, 1048576, 1048576},
        {256, 1048576, 4095, 2, 524288, 1048576, 1048576},
        {256, 1048576, 4096, 1, 1048576, 0, 0},
        {256, 1048576, 20000, 1, 1048576, 0, 0},
        {256, 2097152, 1, 512, 4096, 1048576, 1048576},
        {256, 2097152, 10, 410, 5120, 1048576, 1048576},
        {256, 2097152, 20, 205, 10240, 1048576, 1048576},
        {256, 2097152, 700, 6, 349696, 1048576, 1048576},
        {256, 2097152, 4095, 2, 1048576, 1048576, 1048576},
        {256, 2097152, 4096, 1, 2097152, 0, 0},
        {256, 2097152, 20000, 1, 2097152, 0, 0},
        {64, 0, 1, 1, 1, 0, 0},
        {64, 0, 10, 1, 1, 0, 0},
        {64, 0, 20, 1, 1, 0, 0},
        {64, 0, 700, 1, 1, 0, 0},
        {64, 0, 4095, 1, 1, 0, 0},
        {64, 0, 4096, 1, 1, 0, 0},
        {64, 0, 20000, 1, 1, 0, 0},
        {64, 1, 1, 1, 1, 0, 0},
        {64, 1, 10, 1, 1, 0, 0},
        {64, 1, 20, 1, 1, 0, 0},
        {64, 1, 700, 1, 1, 0, 0},
        {64, 1, 4095, 1, 1, 0, 0},
        {64, 1, 4096, 1, 1, 0, 0},
        {64, 1, 20000, 1, 1, 0, 0},
        {64, 8191, 1, 1, 8191, 0, 0},
        {64, 8191, 10, 1, 8191, 0, 0},
        {64, 8191, 20, 1, 8191, 0, 0},
        {64, 8191, 700, 1, 8191, 0, 0},
        {64, 8191, 4095, 1, 8191, 0, 0},
        {64, 8191, 4096, 1, 8191, 0, 0},
        {64, 8191, 20000, 1, 8191, 0, 0},
        {64, 8192, 1, 2, 4096, 1048576, 1048576},
        {64, 8192, 10, 2, 4096, 1048576, 1048576},
        {64, 8192, 20, 2, 4096, 1048576, 1048576},
        {64, 8192, 700, 2, 4096, 1048576, 1048576},
        {64, 8192, 4095, 1, 8192, 0, 0},
        {64, 8192, 4096, 1, 8192, 0, 0},
        {64, 8192, 20000, 1, 8192, 0, 0},
        {64, 8453, 1, 2, 4352, 1048576, 1048576},
        {64, 8453, 10, 2, 4352, 1048576, 1048576},
        {64, 8453, 20, 2, 4352, 1048576, 1048576},
        {64, 8453, 700, 2, 4352, 1048576, 1048576},
        {64, 8453, 4095, 1, 8453, 0, 0},
        {64, 8453, 4096, 1, 8453, 0, 0},
        {64, 8453, 20000, 1, 8453, 0, 0},
        {64, 16384, 1, 4, 4096, 1048576, 1048576},
        {64, 16384, 10, 4, 4096, 1048576, 1048576},
        {64, 16384, 20, 4, 4096, 1048576, 1048576},
        {64, 16384, 700, 2, 8192, 1048576, 1048576},
        {64, 16384, 4095, 1, 16384, 0, 0},
        {64, 16384, 4096, 1, 16384, 0, 0},
        {64, 16384, 20000, 1, 16384, 0, 0},
        {64, 1048576, 1, 256, 4096, 1048576, 1048576},
        {64, 1048576, 10, 103, 10240, 1048576, 1048576},
        {64, 1048576, 20, 52, 20224, 1048576, 1048576},
        {64, 1048576, 700, 2, 524288, 1048576, 1048576},
        {64, 1048576, 4095, 1, 1048576, 0, 0},
        {64, 1048576, 4096, 1, 1048576, 0, 0},
        {64, 1048576, 20000, 1, 1048576, 0, 0},
        {64, 2097152, 1, 512, 4096, 1048576, 1048576},
        {64, 2097152, 10, 103, 20480, 1048576, 1048576},
        {64, 2097152, 20, 52, 40448, 1048576, 1048576},
        {64, 2097152, 700, 2, 1048576, 1048576, 1048576},
        {64, 2097152, 4095, 1, 2097152, 0, 0},
        {64, 2097152, 4096, 1, 2097152, 0, 0},
        {64, 2097152, 20000, 1, 2097152, 0, 0},
        {8192, 2097152, 700, 187, 11264, 1048576, 2094400},
        {8192, 2097152, 20000, 7, 299776, 1120000, 2240000},
    };
    size_t checked = 0, split = 0;
    for (const auto& w : want) {
        const FoldPlan a = plan_fold(2, w.n, w.rows, w.n_cus), b = plan_fold(4, w.n, w.rows, w.n_cus);
        CHECK(a.chunks == w.chunks && a.chunk == w.chunk && a.partial_bytes == w.part2);
        CHECK(b.chunks == w.chunks && b.chunk == w.chunk && b.partial_bytes == w.part4);
        // what k_fold's grid (rows, chunks) and its chunk argument rely on
        if (a.chunks > 1) CHECK(a.chunk % 256 == 0);
        CHECK(a.chunk >= 1 && a.chunks >= 1 && a.chunks <= 1024);
        CHECK(a.chunks * a.chunk >= w.n);
        CHECK((a.chunks - 1) * a.chunk < std::max<size_t>(w.n, 1));  // no empty chunk (an empty batch: its one chunk)
        CHECK((a.partial_bytes == 0) == (a.chunks == 1));
        if (a.chunks > 1) CHECK(a.partial_bytes >= a.chunks * w.rows * 2 * 4 && a.partial_bytes >= ((size_t)1 << 20));
        if (b.chunks > 1) CHECK(b.partial_bytes >= b.chunks * w.rows * 4 * 4);
        checked++;
        split += a.chunks > 1;
    }
    CHECK(checked >= 2 * 8 * 7 && split > 0);
    // the shapes tests/test_gpu_aggregate_grouped.py::test_one_group_is_the_ungrouped_fold runs split
    CHECK(plan_fold(2, 8453, 10, 256).chunks == 2 && plan_fold(2, 8453, 10, 256).chunk == 4352);
    CHECK(plan_fold(4, 8453, 20, 256).chunks == 2);
    return checked;
}

int main() {
    check_limbs<F64>("F64");
    check_limbs<F128>("F128");
    check_ids();
    printf("plans checked: %zu\n", check_plans());
    printf("fold plans checked: %zu\n", check_fold_plans());
    printf("group_fold_host: OK\n");
    return 0;
}
