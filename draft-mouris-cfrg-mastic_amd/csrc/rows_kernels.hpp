// k_gather_rows: row idx[first + r] of `src` becomes row r of `dst`, for
// r < count (mastic_reports_compact; the plan that makes an in-place use safe
// is compact_plan.hpp).  It serves every segment of a batch: row_bytes from 1
// (wire flags) and 16 (nonces) to hundreds of KB (C5's public shares), rows
// that are aligned to nothing, so source and destination rows start at any
// byte and their offsets differ modulo 4 and modulo 16 from row to row.
//
// Work split.  The destination is cut into 16-byte slots aligned on the
// destination ADDRESS; a row touches at most slots_per_row = (row_bytes + 14) /
// 16 + 1 of them, and one lane owns one (row, slot).  Lanes are numbered flat
// over (row, slot): rows narrower than a wave's 1 KiB are packed several to a
// wave, rows wider than a workgroup's 4 KiB spread over the grid.  A workgroup
// divides once (64-bit, uniform) for its first (row, slot); a lane adds its
// number with 32-bit arithmetic.
//
// A slot that lies wholly inside its row is the body: one aligned 16-byte
// store.  Its 16 source bytes start at any byte s: the lane loads the four
// 4-byte-aligned words from s & ~3 with one 16-byte load (the words need no
// more than 4-byte alignment), a fifth word only if s & 3 != 0, and realigns
// them in registers with v_alignbyte_b32.  All five words hold bytes of the
// source row (the fifth holds byte s + 15 exactly when s & 3 != 0), so no load
// reaches beyond the aligned words that contain the row, and none past the
// buffer's last word.  The bytes of a neighbouring row that share the first or
// last word are shifted out; if an in-place launch is writing that neighbour
// meanwhile, what is read of it is discarded.
//
// A slot the row covers only partly (its head, its tail, or a row shorter
// than a slot) is fetched the same way, loading only the words that hold bytes
// of the row, and goes out byte by byte from the registers: never a wider
// read-modify-write, because the rest of the slot belongs to the
// neighbouring row, which another lane of the same launch is writing.
//
// No lane waits for another; ordering comes from the stream only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int ROWS_THREADS = 256;

inline uint32_t rows_slots_per_row(size_t row_bytes) { return (uint32_t)((row_bytes + 14) / 16 + 1); }
// Workgroups of a launch over `count` rows.
inline uint64_t rows_grid(size_t row_bytes, size_t count) {
    return ((uint64_t)count * rows_slots_per_row(row_bytes) + ROWS_THREADS - 1) / ROWS_THREADS;
}
constexpr uint64_t ROWS_MAX_GRID = 0x7fffffffull;  // one launch's grid.x; the caller splits above it

struct __attribute__((packed, aligned(4))) RowsWords4 {
    uint32_t w[4];
};

// (k_gather_rows, the row-gathering overload of compaction; decide_kernels.hpp has the planes-to-wire-rows one)
__global__ __launch_bounds__(ROWS_THREADS) void k_gather_rows(const uint8_t* src, uint8_t* dst,
                                                              size_t row_bytes, const uint32_t* __restrict__ idx,
                                                              size_t first, size_t count, uint32_t slots_per_row) {
    const uint64_t t0 = (uint64_t)blockIdx.x * ROWS_THREADS;
    const uint64_t r0 = t0 / slots_per_row;
    const uint32_t u = (uint32_t)(t0 - r0 * slots_per_row) + threadIdx.x;  // < slots_per_row + 256
    const uint32_t dr = u / slots_per_row;
    const uint32_t k = u - dr * slots_per_row;
    const uint64_t r = r0 + dr;
    if (r >= count) return;
    const uint8_t* srow = src + (size_t)idx[first + r] * row_bytes;
    const uintptr_t d0 = (uintptr_t)dst + r * row_bytes, d1 = d0 + row_bytes;
    const uintptr_t a = (d0 & ~(uintptr_t)15) + 16 * (uintptr_t)k;  // this lane's slot [a, a + 16)
    const uintptr_t lo = a > d0 ? a : d0, hi = a + 16 < d1 ? a + 16 : d1;
    if (lo >= hi) return;  // a slot past the row's end
    // (pointer arithmetic from src / dst, so the accesses stay global ones)
    if (hi - lo == 16) {
        const uint8_t* sb = srow + (a - d0);
        const uint32_t m = (uint32_t)((uintptr_t)sb & 3);
        const uint32_t* wp = (const uint32_t*)(sb - m);
        const RowsWords4 q = *(const RowsWords4*)wp;
        uint32_t w4 = 0;
        if (m) w4 = wp[4];
        uint4 o;
        o.x = __builtin_amdgcn_alignbyte(q.w[1], q.w[0], m);
        o.y = __builtin_amdgcn_alignbyte(q.w[2], q.w[1], m);
        o.z = __builtin_amdgcn_alignbyte(q.w[3], q.w[2], m);
        o.w = __builtin_amdgcn_alignbyte(w4, q.w[3], m);
        *(uint4*)(dst + r * row_bytes + (a - d0)) = o;
    } else {
        // The slot's 16 source bytes start at sb, before the row for a head
        // slot; of the five words only those that hold bytes of the row are
        // loaded, all before the one wait, and the slot's bytes inside the row
        // leave the registers as byte stores.
        const ptrdiff_t off = (ptrdiff_t)(a - d0);
        const uint8_t* sb = srow + off;
        const uint32_t m = (uint32_t)((uintptr_t)sb & 3);
        const uint32_t* wp = (const uint32_t*)(sb - m);
        const uintptr_t w_lo = (uintptr_t)srow & ~(uintptr_t)3, w_hi = (uintptr_t)srow + row_bytes;
        uint32_t w[5];
#pragma unroll
        for (int i = 0; i < 5; i++) {
            const uintptr_t wa = (uintptr_t)wp + 4 * i;
            w[i] = 0;
            if (wa >= w_lo && wa < w_hi) w[i] = wp[i];
        }
        uint32_t o[4];
#pragma unroll
        for (int i = 0; i < 4; i++) o[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], m);
        uint8_t* dp = dst + r * row_bytes + off;
        const uint32_t j0 = (uint32_t)(lo - a), j1 = (uint32_t)(hi - a);
#pragma unroll
        for (uint32_t j = 0; j < 16; j++)
            if (j >= j0 && j < j1) dp[j] = (uint8_t)(o[j / 4] >> (8 * (j % 4)));
    }
}
