// csrc/nonce_set.hpp on the host (tests/test_nonce_set_host.py builds this with
// ASan / UBSan): the sizing and growth rules over a grid, the keyed hash, and a
// sequential model of the insert / resolve / commit / rehash kernels
// (csrc/nonce_set_kernels.hpp), written with the header's own hash and probe
// functions, against std::set semantics.  The model visits the lanes of each
// phase in a given order, so the claim that the result does not depend on the
// order in which lanes arrive is checked for forward, reverse and shuffled
// orders (an interleaving inside one lane's probe is the kernel's business:
// tests/test_gpu_nonce_set.py).
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <set>
#include <vector>

#include "../../draft-mouris-cfrg-mastic_amd/csrc/nonce_set.hpp"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

typedef std::array<uint32_t, 4> Nonce;
static NsKey key_of(const Nonce& x) { return NsKey{{x[0], x[1], x[2], x[3]}}; }

// ------------------------------------------------------------------ the model
struct Model {
    NsHashKey hk;
    std::vector<NsKey> arena;    // count = arena.size()
    std::vector<uint32_t> slot;  // 0 = empty, else id + 1
    uint64_t arena_cap = 0, most_keys = 0;
    int table_growths = 0, arena_growths = 0;
    bool error = false;

    explicit Model(NsHashKey k, uint64_t hint = 0) : hk(k) { reserve(hint); }
    uint32_t slots() const { return (uint32_t)slot.size(); }
    uint32_t count() const { return (uint32_t)arena.size(); }

    void reserve(uint64_t keys) {
        const uint64_t s = ns_grown_slots(slot.size(), keys);
        const uint64_t cap = ns_grown_arena(arena_cap, s, keys);
        if (cap != arena_cap) {
            arena_growths += arena_cap != 0;
            arena_cap = cap;
        }
        if (s != slot.size()) {
            table_growths += !slot.empty();
            slot.assign(s, 0);
            for (uint32_t id = 0; id < count(); id++) {  // k_ns_rehash
                uint32_t at = ns_home(hk, arena[id], slots());
                uint32_t step = 0;
                for (; step < slots() && slot[at] != 0; step++) at = ns_next(at, slots());
                if (step == slots()) error = true;
                else slot[at] = id + 1;
            }
        }
        // the invariants every admit relies on; the memory bound is per key the set was ever sized for
        // (a capacity hint counts: the caller asked for that much)
        most_keys = std::max(most_keys, keys);
        CHECK((s & (s - 1)) == 0 && s >= 2 * keys && arena_cap >= keys && arena_cap <= s / 2);
        if (s > NS_MIN_SLOTS) CHECK(ns_set_bytes(s, arena_cap) <= 32 * most_keys);
        else CHECK(ns_set_bytes(s, arena_cap) == ns_set_bytes(NS_MIN_SLOTS, NS_MIN_SLOTS / 2));
    }
    NsKey occupant(const std::vector<Nonce>& batch, uint32_t v) const {
        const uint32_t id = v - 1;
        return id < count() ? arena[id] : key_of(batch[id - count()]);
    }
    // fresh mask of the batch; `order` is the order in which the lanes of every phase run
    std::vector<uint8_t> admit(const std::vector<Nonce>& batch, const std::vector<uint32_t>& order) {
        const uint32_t n = (uint32_t)batch.size();
        reserve((uint64_t)count() + n);
        for (uint32_t i : order) {  // k_ns_insert
            const NsKey me = key_of(batch[i]);
            const uint32_t mine = count() + i + 1;
            uint32_t s = ns_home(hk, me, slots()), step = 0;
            for (; step < slots(); step++, s = ns_next(s, slots())) {
                if (slot[s] == 0) {
                    slot[s] = mine;
                    break;
                }
                if (ns_key_eq(occupant(batch, slot[s]), me)) {
                    if (slot[s] > count()) slot[s] = std::min(slot[s], mine);
                    break;
                }
            }
            if (step == slots()) error = true;
        }
        std::vector<uint8_t> fresh(n, 0);
        std::vector<uint32_t> slot_of(n, 0xffffffffu);
        for (uint32_t i : order) {  // k_ns_resolve
            const NsKey me = key_of(batch[i]);
            uint32_t s = ns_home(hk, me, slots()), step = 0;
            for (; step < slots(); step++, s = ns_next(s, slots())) {
                if (slot[s] == 0) {
                    error = true;
                    break;
                }
                if (ns_key_eq(occupant(batch, slot[s]), me)) {
                    fresh[i] = slot[s] == count() + i + 1;
                    if (fresh[i]) slot_of[i] = s;
                    break;
                }
            }
            if (step == slots()) error = true;
        }
        const uint32_t base = count();
        for (uint32_t i : order) {  // k_ns_commit
            if (!fresh[i]) continue;
            CHECK(slot[slot_of[i]] == base + i + 1);
            arena.push_back(key_of(batch[i]));
            slot[slot_of[i]] = count();  // id + 1 of the key just appended
        }
        CHECK(arena.size() <= arena_cap && 2 * arena.size() <= slot.size());
        for (uint32_t v : slot) CHECK(v <= count());  // arena ids only again
        return fresh;
    }
    bool contains(const Nonce& x) const {
        const NsKey me = key_of(x);
        uint32_t s = ns_home(hk, me, slots());
        for (uint32_t step = 0; step < slots(); step++, s = ns_next(s, slots())) {
            if (slot[s] == 0) return false;
            if (ns_key_eq(arena[slot[s] - 1], me)) return true;
        }
        return false;
    }
};

static std::mt19937_64 g_rng(20240607);
static Nonce rnd_nonce() {
    const uint64_t a = g_rng(), b = g_rng();
    return Nonce{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
}

static int g_admits = 0;
// Admit `batch` into three models that differ in hash key and lane order and
// into a std::set; all four must agree.
struct Harness {
    Model fwd, rev, shuf;
    std::set<Nonce> want;
    explicit Harness(uint64_t hint = 0)
        : fwd(NsHashKey{1, 2}, hint), rev(NsHashKey{0x0123456789abcdefull, 0xfedcba9876543210ull}, hint),
          shuf(NsHashKey{g_rng(), g_rng()}, hint) {}
    std::vector<uint8_t> admit(const std::vector<Nonce>& batch) {
        std::vector<uint8_t> expect;
        for (const Nonce& x : batch) expect.push_back(want.insert(x).second);
        std::vector<uint32_t> order(batch.size());
        std::iota(order.begin(), order.end(), 0u);
        CHECK(fwd.admit(batch, order) == expect);
        std::reverse(order.begin(), order.end());
        CHECK(rev.admit(batch, order) == expect);
        std::shuffle(order.begin(), order.end(), g_rng);
        CHECK(shuf.admit(batch, order) == expect);
        for (Model* m : {&fwd, &rev, &shuf}) {
            CHECK(!m->error && m->count() == want.size());
            for (const Nonce& x : batch) CHECK(m->contains(x));
            std::set<Nonce> got;
            for (const NsKey& k : m->arena) got.insert(Nonce{k.w[0], k.w[1], k.w[2], k.w[3]});
            CHECK(got == want);  // export: the same keys, each once
        }
        g_admits++;
        return expect;
    }
};

// ------------------------------------------------------------------- the checks
static void check_sizing() {
    std::vector<uint64_t> grid;
    for (uint64_t k = 0; k <= 5000; k++) grid.push_back(k);
    for (int b = 12; b <= 30; b++)
        for (int64_t d : {-1, 0, 1}) grid.push_back(((uint64_t)1 << b) + d);
    std::sort(grid.begin(), grid.end());
    uint64_t prev = 0;
    for (uint64_t keys : grid) {
        if (keys > NS_MAX_KEYS) continue;
        const uint64_t s = ns_table_slots(keys);
        CHECK((s & (s - 1)) == 0 && s >= NS_MIN_SLOTS && s >= 2 * keys && s >= prev);  // power of two, load <= 1/2, monotone
        CHECK(s == NS_MIN_SLOTS || s < 4 * keys);                                      // the least such power
        CHECK(s <= ((uint64_t)1 << 31));                                               // slot indices fit 32 bits
        prev = s;
        const uint64_t cap = ns_arena_keys(s, keys);
        CHECK(cap >= keys && cap <= s / 2);
        if (s > NS_MIN_SLOTS) CHECK(ns_set_bytes(s, cap) <= 32 * keys);
        // the growth rules keep what fits and never shrink
        CHECK(ns_grown_slots(s, keys) == s && ns_grown_slots(2 * s, keys) == 2 * s);
        CHECK(ns_grown_slots(0, keys) == s && ns_grown_arena(0, s, keys) == cap && ns_grown_arena(cap, s, keys) == cap);
        if (keys) CHECK(ns_grown_slots(s, s / 2 + 1) == 2 * s);
    }
    // a set grown one nonce at a time: the arena is replaced O(log slots) times per table size
    Model m(NsHashKey{3, 4});
    for (int i = 0; i < 20000; i++) m.reserve(i + 1), m.arena.push_back(key_of(rnd_nonce()));
    CHECK(m.table_growths == 6);  // 1024 -> 2048 -> ... -> 65536 (>= 40000) slots
    CHECK(m.arena_growths <= 6 * 16);
}

static void check_hash() {
    // SipHash-2-4, key 00..0f, message 00..0f (the reference implementation's vectors, entry 16)
    const NsHashKey k{0x0706050403020100ull, 0x0f0e0d0c0b0a0908ull};
    const NsKey m{{0x03020100u, 0x07060504u, 0x0b0a0908u, 0x0f0e0d0cu}};
    CHECK((ns_siphash<2, 4>(k, m)) == 0x3f2acc7f57c29bdbull);
    // keying: another key, another hash and (nearly always) another home slot
    const NsHashKey k2{k.k0 ^ 1, k.k1};
    int same_home = 0;
    for (int i = 0; i < 4096; i++) {
        const NsKey x = key_of(rnd_nonce());
        CHECK(ns_hash(k, x) != ns_hash(k2, x));
        same_home += ns_home(k, x, 1024) == ns_home(k2, x, 1024);
        CHECK(ns_home(k, x, 1024) < 1024 && ns_next(1023, 1024) == 0 && ns_next(5, 1024) == 6);
    }
    CHECK(same_home < 40);  // expected 4; 40 is > 10 standard deviations away
    // every word of the nonce reaches the hash
    NsKey x = key_of(rnd_nonce());
    for (int w = 0; w < 4; w++) {
        NsKey y = x;
        y.w[w] ^= 0x80000000u;
        CHECK(ns_hash(k, x) != ns_hash(k, y));
    }
}

static void check_model() {
    {  // the empty batch, one nonce, the same nonce again
        Harness h;
        CHECK(h.admit({}).empty());
        const Nonce a = rnd_nonce();
        CHECK(h.admit({a}) == std::vector<uint8_t>{1});
        CHECK(h.admit({a}) == std::vector<uint8_t>{0});
        CHECK(h.admit({}).empty() && h.want.size() == 1);
    }
    {  // 257 equal nonces: the first wins; then none
        Harness h;
        std::vector<Nonce> b(257, rnd_nonce());
        std::vector<uint8_t> e(257, 0);
        e[0] = 1;
        CHECK(h.admit(b) == e);
        CHECK(h.admit(b) == std::vector<uint8_t>(257, 0));
    }
    for (int w = 0; w < 4; w++) {  // equal in three of four words: all distinct
        Harness h;
        const Nonce base = rnd_nonce();
        std::vector<Nonce> b;
        for (uint32_t i = 0; i < 300; i++) {
            Nonce x = base;
            x[w] = base[w] + (i % 150);  // every value twice, 150 apart
            b.push_back(x);
        }
        const std::vector<uint8_t> f = h.admit(b);
        CHECK(std::count(f.begin(), f.end(), 1) == 150 && h.want.size() == 150);
    }
    {  // home slots in the table's last two slots: the probes wrap to slot 0
        Harness h;
        std::vector<Nonce> b;
        while (b.size() < 12) {
            const Nonce x = rnd_nonce();
            if (ns_home(h.fwd.hk, key_of(x), NS_MIN_SLOTS) >= NS_MIN_SLOTS - 2) b.push_back(x);
        }
        const Nonce again = b[3], early = b[7];
        b.push_back(again);
        b.insert(b.begin(), early);
        h.admit(b);
        CHECK(h.fwd.slots() == NS_MIN_SLOTS && h.fwd.slot[NS_MIN_SLOTS - 1] && h.fwd.slot[NS_MIN_SLOTS - 2]);
        for (int s = 0; s < 10; s++) CHECK(h.fwd.slot[s] != 0);  // 12 keys, 2 slots before the wrap
        CHECK(h.admit(b) == std::vector<uint8_t>(b.size(), 0));
    }
    {  // a sequence that grows the table four times, with replays of earlier batches mixed in
        Harness h;
        std::vector<Nonce> seen;
        for (size_t n : {600, 1200, 2400, 4800}) {
            std::vector<Nonce> b;
            for (size_t i = 0; i < n; i++) b.push_back(i % 5 == 4 && !seen.empty() ? seen[g_rng() % seen.size()] : rnd_nonce());
            h.admit(b);
            seen.insert(seen.end(), b.begin(), b.end());
        }
        CHECK(h.fwd.table_growths >= 4 && h.rev.table_growths >= 4);
        for (int i = 0; i < 1000; i++) CHECK(!h.fwd.contains(rnd_nonce()));
    }
    {  // a capacity hint: no growth below it
        Harness h(5000);
        for (int r = 0; r < 5; r++) {
            std::vector<Nonce> b;
            for (int i = 0; i < 1000; i++) b.push_back(rnd_nonce());
            h.admit(b);
        }
        CHECK(h.fwd.table_growths == 0 && h.fwd.arena_growths == 0);
    }
}

int main() {
    check_sizing();
    check_hash();
    check_model();
    printf("admits checked: %d\n", g_admits);
    printf("nonce_set_host: OK\n");
    return 0;
}
