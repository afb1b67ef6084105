// The host side of the folds (C++17; no HIP): for mastic_aggregate_grouped the
// check of the group ids, the launch plan of k_fold_grouped (fold_kernels.hpp) and
// the exact recombination of its integer word sums into a field element; for
// the ungrouped fold the chunking of k_fold (plan_fold).  fold.hpp executes
// the plans and decides nothing itself; tests/host/group_fold_host.cpp checks
// all of it on the host.
//
// The fold.  The out shares are word planes out[row][word][stride]; a
// workgroup (row, chunk) streams the reports of its chunk exactly as k_fold
// does (lane r reads report r, coalesced, four loads in flight) and, instead
// of one running sum, keeps per group g of the pass the W32 integer sums
//   S_i[g] = sum over the chunk's reports of group g of word i of out[row]
// as 64-bit counters in LDS (plain integer LDS atomic adds: GF(p) has no
// atomic).  A chunk holds < 2^31 reports and a word is < 2^32, so S_i < 2^63
// and nothing wraps.  At the end of the chunk one lane per group forms
//   sum_i S_i * 2^(32 i) mod p        (limbs_to_elem, below)
// and stores it as a field element; k_fold_shares merges the chunks.
//
// Copies.  Lanes of one wave that add into the same group hit one LDS
// address and serialise.  Each (group, word) counter is therefore kept
// `copies` times, side by side ([group][word][copy]: a wave whose 64 ids are
// equal adds to consecutive 8-byte slots), indexed by lane & (copies - 1) and
// summed at the end.
//
// Passes.  A pass holds the groups whose counters fit the LDS budget (8 * W32
// bytes per group: 16 B Field64, 32 B Field128).  More groups take further
// passes, and EVERY pass reads the out shares again: reports whose group
// belongs to another pass contribute nothing.  At the default budget one pass
// holds 4,096 Field64 or 2,048 Field128 groups.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GF_HD __host__ __device__ inline
#else
#define GF_HD inline
#endif

#ifndef MASTIC_GROUP_NONE
#define MASTIC_GROUP_NONE 0xFFFFFFFFu
#endif
#ifndef MASTIC_MAX_GROUPS
#define MASTIC_MAX_GROUPS 65536
#endif

// Measured on one MI355X (profiles/grouped_fold.txt, DESIGN.md "Grouped fold";
// the blocking call, median of 5; `runs` = ids in time-ordered runs, so whole
// waves share one id, `random` = uniform ids):
//   sweep level, 1M reports x 700 rows, runs / random, ms by copies (LDS)
//     G = 64    1: 5.14/1.64   4: 1.67/1.56   8 (8 KiB): 1.53/1.56   16 (16 KiB): 1.55/1.57   64 (64 KiB): 3.07/3.11
//     G = 256   1: 5.22/1.80   4 (16 KiB): 1.77/1.66   8 (32 KiB): 2.07/2.25   16 (64 KiB): 3.09/3.11
//     G = 1024  1 (16 KiB): 5.65/2.25   2 (32 KiB): 3.40/2.55   4 (64 KiB): 3.42/3.65
//   C2 step, 16,384 reports x 20,000 rows, G = 1:  1: 2.23   4: 0.63   16: 0.48   64: 0.48
// One address shared by a whole wave costs 3-5x; 8 to 16 copies remove that,
// more add nothing; counters beyond 16 KiB per workgroup cost more in occupancy
// than their copies save (except for runs at G = 1024, where random ids lose
// what runs gain).  Two alternatives lost everywhere and are not in the tree:
// a wave whose ids are equal summing across its lanes first and adding once
// (sweep level, G = 8 runs: 3.26 ms against 1.47) and, for G <= 8, per-lane
// field accumulators in registers with no LDS counters (1.96-2.11 ms against
// 1.47-1.56; C2 step 0.86-0.88 against 0.61).
struct GroupFoldKnobs {
    // LDS of one workgroup's counters: the largest dynamic allocation a kernel
    // gets without raising its limit, two workgroups per CU.  (Half of it would
    // fold 4,096 Field64 groups in two passes over the out shares instead of
    // one slower pass; not measured to be better.)
    static constexpr size_t default_lds_budget = size_t(64) << 10;
    // Cap of the per-chunk partials buffer (raised to one chunk's partials).
    static constexpr size_t default_partial_budget = size_t(64) << 20;
    // Copies stop where their counters pass this many bytes: every workgroup
    // zeroes and sums all of them, and LDS per workgroup bounds the occupancy.
    static constexpr size_t copies_lds_cap = size_t(16) << 10;
    static constexpr uint32_t max_copies = 16;
    // A chunk is at least this many reports per group of its pass (and at
    // least min_chunk): each chunk writes one partial element per (group, row),
    // which is then read back, against chunk elements per row read.
    static constexpr size_t chunk_per_group = 8;
    static constexpr size_t min_chunk = 4096;
    static constexpr size_t max_chunks = 1024;  // <= 65,535 (grid y)
};

// First report index whose id is neither < n_groups nor MASTIC_GROUP_NONE, or
// -1.  counts[g] (n_groups entries, may be null) = the reports r with
// group[r] == g and (valid == null or valid[r] != 0); only meaningful when
// the result is -1.
inline long long check_groups(const uint32_t* group, size_t n, size_t n_groups, const uint8_t* valid,
                              uint64_t* counts) {
    if (counts) std::fill(counts, counts + n_groups, (uint64_t)0);
    for (size_t r = 0; r < n; r++) {
        const uint32_t g = group[r];
        if (g == MASTIC_GROUP_NONE) continue;
        if (g >= n_groups) return (long long)r;
        if (counts && (!valid || valid[r])) counts[g]++;
    }
    return -1;
}

// The ungrouped fold (k_fold, one running sum per row): few rows over many
// reports (a sweep level: ~700 rows x 1M reports) are split into chunks of
// reports so the grid (rows, chunks) fills the chip, and k_fold_shares merges
// the chunks' partial sums mod p.
struct FoldPlan {
    size_t chunks = 1;         // report chunks (grid y); an empty batch still writes its all-zero agg share: one chunk
    size_t chunk = 1;          // reports per chunk; a multiple of 256 when chunks > 1
    size_t partial_bytes = 0;  // [chunks][rows] elements, at least 1 MiB; 0 with one chunk (written in place)
};

// w32: 32-bit words per element (2 / 4).  rows >= 1 (no rows: nothing is launched).
inline FoldPlan plan_fold(int w32, size_t n, size_t rows, int n_cus) {
    FoldPlan pl;
    const size_t target = (size_t)n_cus * 16;
    size_t chunks = 1;
    if (rows && rows < target && n >= 8192) chunks = std::min<size_t>({(target + rows - 1) / rows, n / 4096, (size_t)1024});
    pl.chunk = chunks > 1 ? ((n + chunks - 1) / chunks + 255) / 256 * 256 : std::max<size_t>(n, 1);
    pl.chunks = std::max<size_t>(1, (n + pl.chunk - 1) / pl.chunk);
    if (pl.chunks > 1) pl.partial_bytes = std::max<size_t>(pl.chunks * rows * w32 * 4, (size_t)1 << 20);
    return pl;
}

struct GroupFoldPlan {
    uint32_t groups_per_pass = 0;  // groups of every pass but the last: pass k holds [k * gpp, min(G, (k + 1) * gpp))
    uint32_t passes = 0;
    uint32_t copies = 1;           // a power of two
    uint32_t chunks = 0;           // report chunks (0: no reports, nothing is launched)
    uint32_t chunk = 256;          // reports per chunk, a multiple of 256
    uint32_t grid_x = 0, grid_y = 0;  // (rows, chunks), 256 threads
    size_t lds_bytes = 0;          // dynamic LDS of k_fold_grouped
    size_t partial_bytes = 0;      // [chunks][groups_per_pass][rows] elements; 0 with one chunk (written in place)
};

// w32: 32-bit words per element (2 / 4).  lds_budget / partial_budget: 0 = the
// defaults above.  The caller has checked n_groups * rows <= INT_MAX and
// 1 <= n_groups <= MASTIC_MAX_GROUPS.
inline GroupFoldPlan plan_group_fold(int w32, size_t n, size_t rows, size_t n_groups, int n_cus, size_t lds_budget,
                                     size_t partial_budget) {
    GroupFoldPlan pl;
    if (!lds_budget) lds_budget = GroupFoldKnobs::default_lds_budget;
    if (!partial_budget) partial_budget = GroupFoldKnobs::default_partial_budget;
    const size_t slot = (size_t)w32 * 8;  // one group's counters
    const size_t max_slots = std::max<size_t>(1, lds_budget / slot);
    n_groups = std::max<size_t>(1, n_groups);
    // as few passes as the budget allows, then the groups spread evenly over them
    pl.passes = (uint32_t)((n_groups + max_slots - 1) / max_slots);
    pl.groups_per_pass = (uint32_t)((n_groups + pl.passes - 1) / pl.passes);
    const size_t gpp = pl.groups_per_pass;
    const size_t cap = std::min(lds_budget, GroupFoldKnobs::copies_lds_cap);
    while (pl.copies < GroupFoldKnobs::max_copies && 2 * (size_t)pl.copies * gpp * slot <= cap) pl.copies *= 2;
    pl.lds_bytes = (size_t)pl.copies * gpp * slot;
    pl.grid_x = (uint32_t)rows;
    if (n == 0 || rows == 0) return pl;
    // chunks: enough workgroups to fill the chip when the rows are few
    // (plan_fold's rule), bounded by the chunk length that amortises
    // a chunk's partials, the partials budget and the int element count of
    // k_fold_shares
    const size_t target = (size_t)std::max(1, n_cus) * 16;
    size_t chunks = rows < target ? (target + rows - 1) / rows : 1;
    const size_t min_chunk = std::max(GroupFoldKnobs::min_chunk, GroupFoldKnobs::chunk_per_group * gpp);
    const size_t per_chunk = gpp * rows;  // partial elements of one chunk (<= INT_MAX)
    chunks = std::min({chunks, n / min_chunk, GroupFoldKnobs::max_chunks, partial_budget / (per_chunk * w32 * 4),
                       (size_t)INT_MAX / per_chunk});
    chunks = std::max<size_t>(1, chunks);
    const size_t chunk = ((n + chunks - 1) / chunks + 255) / 256 * 256;
    pl.chunk = (uint32_t)chunk;
    pl.chunks = (uint32_t)((n + chunk - 1) / chunk);
    pl.grid_y = pl.chunks;
    pl.partial_bytes = pl.chunks > 1 ? (size_t)pl.chunks * per_chunk * w32 * 4 : 0;
    return pl;
}

// sum_i s[i] * 2^(32 i) mod p, s[i] < 2^63 (Horner from the top word; the same
// code runs in k_fold_grouped and on the host).
template <class F>
GF_HD typename F::E limbs_to_elem(const uint64_t* s) {
    const typename F::E b = F::from_u64((uint64_t)1 << 32);
    typename F::E acc = F::from_u64(s[F::W32 - 1]);
    for (int i = F::W32 - 2; i >= 0; i--) acc = F::add(F::mul(acc, b), F::from_u64(s[i]));
    return acc;
}
