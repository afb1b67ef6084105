// The plan of mastic_reports_compact (host only, C++17; no HIP): which rows a
// stable in-place compaction of a resident batch moves, and in which launches.
// mastic_hip.hip executes it with k_gather_rows (rows_kernels.hpp) and
// device-to-device copies; tests/host/compact_plan_host.cpp runs every plan on
// a byte array with launch semantics.
//
// keep[n] gives src[j], the ascending source row of kept row j, and the
// identity prefix (the kept rows with src[j] == j, which never move).  The gap
// g(j) = src[j] - j counts the rows dropped before src[j]; it never decreases
// with j, and that decides the schedule.  With `a` the first row not yet moved:
//
//   direct tile [a, b), b - a <= g(a): gathered straight into place by one
//     launch.  Every row it writes has index < b <= a + g(a) = src[a]; every
//     row this launch or a later one reads has index >= src[a] (src ascends).
//     So within the launch reads and writes are disjoint, and nothing a later
//     launch needs is overwritten.
//   staged tile [a, b), b - a <= S: gathered into the staging buffer by one
//     launch and copied to rows [a, b) by the next (contiguous).  The copy's
//     destination lies below every source row of every later tile:
//     src[j] >= j >= b.
//
// A launch is in-order on one stream after the previous one; no launch waits
// for anything inside itself.
//
// The rule (CompactKnobs): a tile is direct where 2 * g(a) >= S, staged
// otherwise.  A direct launch then moves at least S/2 rows, a staged pair S,
// so every launch but those of the last tile moves >= S/2 rows and the plan has
// at most 2 * ceil(moved / S) + 1 launches.  Direct tiles move each byte once,
// staged tiles twice, so the staging size trades memory and launch count (small
// gaps: one dropped report at row 0 keeps g = 1 for ever) against bytes moved.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

struct CompactKnobs {
    // Default staging buffer of mastic_reports_compact (staging_bytes = 0).
    // Measured (profiles/reports_compact.txt, DESIGN.md "Compacting a batch":
    // one MI355X, 1M C2-shaped reports, the blocking call, median of 5, spread
    // within 5 %):
    //   staging   keep 50 %   keep 99 %   keep 1 %
    //    16 MiB    2.58 ms     5.92 ms    1.16 ms
    //    64 MiB    2.56 ms     5.53 ms    1.30 ms
    //   256 MiB    2.76 ms     7.88 ms    1.20 ms
    // Where tiles are staged (99 % kept) 16 MiB takes twice the launches of
    // 64 MiB (366 against 177) and 256 MiB moves more rows twice (25.7 GB of
    // traffic against 20.6 GB): 64 MiB is fastest or level wherever rows move
    // in bulk; at 1 % kept the call is its fixed host cost at every size.
    static constexpr size_t default_staging_bytes = size_t(64) << 20;
    // A tile is direct where direct_gap_factor * g(a) >= S.  2 is the largest
    // factor the launch bound above holds for.
    static constexpr uint64_t direct_gap_factor = 2;
};

struct CompactIndex {
    std::vector<uint32_t> src;  // [n_kept], ascending
    size_t n_kept = 0;
    size_t prefix = 0;  // src[j] == j for j < prefix; those rows are never touched
    size_t moved() const { return n_kept - prefix; }
};

inline CompactIndex compact_index(const uint8_t* keep, size_t n) {
    CompactIndex ix;
    size_t kept = 0;
    for (size_t i = 0; i < n; i++) kept += keep[i] != 0;
    // Branch-free: every row writes its number at the cursor and only a kept
    // row advances it (one spare slot takes the writes after the last kept
    // row).  A branch per row mispredicts on half of a random mask, which at
    // 1M reports cost more than moving the rows (profiles/reports_compact.txt).
    ix.src.resize(kept + 1);
    uint32_t* out = ix.src.data();
    size_t j = 0;
    for (size_t i = 0; i < n; i++) {
        out[j] = (uint32_t)i;
        j += keep[i] != 0;
    }
    ix.src.resize(kept);
    ix.n_kept = kept;
    while (ix.prefix < kept && ix.src[ix.prefix] == ix.prefix) ix.prefix++;
    return ix;
}

enum CompactOp : uint8_t {
    CP_GATHER_DIRECT,  // rows src[first..first+count) -> rows [first, first+count) of the segment
    CP_GATHER_STAGE,   // rows src[first..first+count) -> rows [0, count) of the staging buffer
    CP_COPY_BACK,      // rows [0, count) of the staging buffer -> rows [first, first+count) of the segment
};

struct CompactLaunch {
    CompactOp op;
    size_t first, count;  // kept-row range [first, first + count)
};

// Staging capacity in rows of a segment whose rows are row_bytes wide.
inline size_t compact_stage_rows(size_t staging_bytes, size_t row_bytes) {
    return std::max<size_t>(1, staging_bytes / std::max<size_t>(1, row_bytes));
}

// The staging buffer's size: the caller's bound (0: the default), at least one
// row of the widest segment, and no more than the rows that move can fill.
inline size_t compact_staging_bytes(size_t asked, size_t widest_row, size_t moved_rows) {
    size_t b = asked ? asked : CompactKnobs::default_staging_bytes;
    b = std::max(b, widest_row);
    const size_t all = widest_row * std::max<size_t>(1, moved_rows);
    return std::min(b, all);
}

// The ordered launches of one segment with a staging capacity of S rows.
inline std::vector<CompactLaunch> compact_launches(const CompactIndex& ix, size_t S) {
    std::vector<CompactLaunch> out;
    if (S == 0) S = 1;
    size_t a = ix.prefix;
    while (a < ix.n_kept) {
        const size_t g = (size_t)ix.src[a] - a;  // >= 1 past the prefix
        if (CompactKnobs::direct_gap_factor * (uint64_t)g >= (uint64_t)S) {
            const size_t cnt = std::min(g, ix.n_kept - a);
            out.push_back({CP_GATHER_DIRECT, a, cnt});
            a += cnt;
        } else {
            const size_t cnt = std::min(S, ix.n_kept - a);
            out.push_back({CP_GATHER_STAGE, a, cnt});
            out.push_back({CP_COPY_BACK, a, cnt});
            a += cnt;
        }
    }
    return out;
}

inline size_t compact_launch_bound(size_t moved_rows, size_t S) {
    if (S == 0) S = 1;
    return 2 * ((moved_rows + S - 1) / S) + 1;
}
