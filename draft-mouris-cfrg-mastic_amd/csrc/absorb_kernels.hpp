// The binder sponges: the one-hot and payload TurboSHAKE absorption of the
// words each level produces (k_absorb, k_absorb_pair), and k_spin, the test
// hook that delays the stream they run on.
#pragma once
#include "keccak.hpp"
#include "planes.hpp"

// ------------------------------------------------------------- binder absorb
// Continues the one-hot (sponge 0) or payload (sponge 1) TurboSHAKE over the
// words one level produced.  Positions are uniform (tracked by the host).
// Level buffers (proofs, payload differences) are TILED, not planes: word m
// of report r sits at  seg + (r / 64) * gstride + m * 64 + r % 64,  so a
// sponge wave (one report group) streams one contiguous region block after
// block, and a level-kernel store of one word for 64 reports is still one
// 256-byte row.
struct AbsorbArgs {
    const uint32_t* seg[2];
    int gstride[2];  // words per report group of each segment (planes: 64)
    int rstride;     // words between consecutive stream words of a report (tiled: 64, planes: stride)
    int nbytes[2];
    int f[2];
    int prio;  // s_setprio of the sponge waves (0..3)
    int dbg;   // timing experiments only (results wrong): 1 no loads, 2 no permutations, 4 neither (sleeps)
    int which0;  // sponge of grid row 0 (0 one-hot, 1 payload): a launch covers which0 .. which0 + gridDim.y - 1
};
MH_D void absorb_setprio(int prio) {
    switch (prio) {
        case 0: break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}

// The next block's 43 source words are loaded before the current block's
// permutation, so their HBM/L2 latency hides under ~2.3k VALU instructions.
// Blocks whose words are all in range (every block but the first and last of
// a launch) use plain loads: a zero-select right after a load would force a
// vmcnt(0) wait per word.
__global__ __launch_bounds__(256) void k_absorb(Planes pl, AbsorbArgs a) {
    // The sponge chain is the latency-critical path and runs beside the
    // level-eval waves: win every issue arbitration on the shared SIMD.
    absorb_setprio(a.prio);
    const int r = blockIdx.x * 256 + threadIdx.x;
    const int which = a.which0 + (int)blockIdx.y;
    if (r >= pl.stride) return;
    const int nb = a.nbytes[which];
    if (nb == 0) return;
    const int S = pl.stride;
    uint32_t* sp = which == 0 ? pl.sp_onehot : pl.sp_payload;
    const uint32_t* seg = a.seg[which] + (size_t)(r >> 6) * a.gstride[which];  // this wave's tile group
    const uint32_t lb = (uint32_t)r * 4u;
    const uint32_t lt = (uint32_t)(r & 63) * 4u;  // lane offset inside a tile row
    const uint32_t rowb = (uint32_t)a.rstride * 4u;  // bytes between stream words
    KState s;
#pragma unroll
    for (int i = 0; i < 25; i++) s.a[i] = u32x2{pld(sp + (size_t)(2 * i) * S, lb), pld(sp + (size_t)(2 * i + 1) * S, lb)};
    const int f = a.f[which];
    const int q = f >> 2;
    const int sh = f & 3;
    const int off = sh ? 1 : 0;           // window starts one word early when shifted
    const int amt = (32 - 8 * sh) & 31;  // block word j = alignbit(w[j+1], w[j], amt)
    const int nw = (nb + 3) >> 2;
    const int end = f + nb;
    auto load_block = [&](int b, uint32_t* w) {
        const int base = KECCAK_RATE_WORDS * b - q - off;
        if (base >= 0 && base + KECCAK_RATE_WORDS < nw) {
            const __amdgpu_buffer_rsrc_t rs = mh_rsrc(seg + (size_t)base * a.rstride);
            // the row offset is a running SGPR sum made opaque at every step,
            // so the compiler cannot hoist 43 loop-invariant offsets (which it
            // would spill to VGPRs and then waterfall)
            uint32_t so = 0;
#pragma unroll
            for (int j = 0; j < KECCAK_RATE_WORDS + 1; j++) {
                w[j] = pld_so(rs, lt, so);
                so += rowb;
                asm volatile("" : "+s"(so));
            }
        } else {
#pragma unroll
            for (int j = 0; j < KECCAK_RATE_WORDS + 1; j++) {
                const int m = base + j;
                const int mc = m < 0 ? 0 : (m >= nw ? nw - 1 : m);
                w[j] = pld(seg + (size_t)mc * a.rstride, lt);
            }
#pragma unroll
            for (int j = 0; j < KECCAK_RATE_WORDS + 1; j++) {
                const int m = base + j;
                w[j] = (m >= 0 && m < nw) ? w[j] : 0u;
            }
        }
    };
    // one block buffer, next block's loads issued after the XOR (see k_absorb_pair)
    uint32_t cur[KECCAK_RATE_WORDS + 1];
    load_block(0, cur);
    for (int b = 0;; b++) {
        const bool full = end >= KECCAK_RATE * (b + 1);
        const bool more = end > KECCAK_RATE * (b + 1);
#pragma unroll
        for (int j = 0; j < KECCAK_RATE_WORDS; j++) kxor_word(s, j, __builtin_amdgcn_alignbit(cur[j + 1], cur[j], amt));
        if (!full) break;
        asm volatile("" ::: "memory");
        if (more) load_block(b + 1, cur);
        keccak_p12(s);
        if (!more) break;
    }
#pragma unroll
    for (int i = 0; i < 25; i++) {
        pst(sp + (size_t)(2 * i) * S, lb, s.a[i].lo);
        pst(sp + (size_t)(2 * i + 1) * S, lb, s.a[i].hi);
    }
}

// Two lanes per sponge (keccak_p12_pair): lane h of report r holds state
// words 2i + h.  Block word j = alignbit(w[j+1], w[j], amt) as above; lane h
// needs the j = 2i + h, i.e. stream words base + h + k, k < 42, which it loads
// itself (the plane offset h*S is part of its per-lane buffer offset).
// Each lane keeps only its own stream words of a block, 2i + h (22 words):
// the word after each, 2i + h + 1, is the partner lane's word i (h = 0) or
// i + 1 (h = 1), fetched with one DPP swap per word when the fill offset is not
// a multiple of 4 (shifted byte image).  22 VGPRs of block buffer instead of
// 42, so the kernel fits 5 waves per SIMD without spills.
#define ABSORB_MIN_WAVES 5
// (partner exchanges through the LDS crossbar, keccak.hpp pair_swap<true>, instead
// of DPP moves: measured, not adopted; hence the `false` below)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ABSORB_MIN_WAVES)))
void k_absorb_pair(Planes pl, AbsorbArgs a) {
    absorb_setprio(a.prio);
    // (launched with optional dynamic LDS that is never touched: it only caps
    // how many absorb workgroups share a CU, see mastic_ctx::absorb_lds)
    const int h = threadIdx.x & 1;
    const int r = blockIdx.x * (int)(blockDim.x >> 1) + (int)(threadIdx.x >> 1);
    const int which = a.which0 + (int)blockIdx.y;
    if (r >= pl.stride) return;  // both lanes of a pair leave together
    const int nb = a.nbytes[which];
    if (nb == 0) return;
    const int S = pl.stride;
    uint32_t* sp = which == 0 ? pl.sp_onehot : pl.sp_payload;
    const uint32_t* seg = a.seg[which] + (size_t)(r >> 6) * a.gstride[which];  // this wave's tile group
    const uint32_t lbh = ((uint32_t)h * (uint32_t)S + (uint32_t)r) * 4u;  // state plane h of the pair
    const uint32_t lt = (uint32_t)(r & 63) * 4u;                            // lane offset in a tile row
    const uint32_t rowb = (uint32_t)a.rstride * 4u;                          // bytes between stream words
    const uint32_t lth = lt + (uint32_t)h * rowb;                           // ... of the next word for h = 1
    const uint32_t rowb2 = 2u * rowb;                                        // own words are every other word
    KHalf s;
#pragma unroll
    for (int i = 0; i < 25; i++) s.a[i] = pld(sp + (size_t)(2 * i) * S, lbh);
    const int f = a.f[which];
    const int q = f >> 2;
    const int sh = f & 3;
    const int off = sh ? 1 : 0;
    const int amt = (32 - 8 * sh) & 31;
    const int nw = (nb + 3) >> 2;
    const int end = f + nb;
    constexpr int NL = KECCAK_RATE_WORDS / 2 + 1;  // words loaded per lane and block: base + 2k + h, k < 22
    auto load_block = [&](int b, uint32_t* w) {
        const int base = KECCAK_RATE_WORDS * b - q - off;
        if (base >= 0 && base + KECCAK_RATE_WORDS + 1 < nw) {
            const __amdgpu_buffer_rsrc_t rs = mh_rsrc(seg + (size_t)base * a.rstride);
            uint32_t so = 0;  // running opaque row offset, as in k_absorb
#pragma unroll
            for (int k = 0; k < NL; k++) {
                w[k] = pld_so(rs, lth, so);
                so += rowb2;
                asm volatile("" : "+s"(so));
            }
        } else {
            // first / last block of the launch: clamped loads, zero outside
            // [0, nw); the word index is per lane (h), so it goes into the
            // lane offset (the descriptor, from a pointer, must be uniform)
#pragma unroll
            for (int k = 0; k < NL; k++) {
                const int m = base + 2 * k + h;
                const int mc = m < 0 ? 0 : (m >= nw ? nw - 1 : m);
                w[k] = pld(seg, (uint32_t)mc * rowb + lt);
            }
#pragma unroll
            for (int k = 0; k < NL; k++) {
                const int m = base + 2 * k + h;
                w[k] = (m >= 0 && m < nw) ? w[k] : 0u;
            }
        }
    };
    // One block buffer.  Per block: XOR the current block (waits for its
    // loads), THEN issue the next block's loads into the same registers, then
    // permute: the loads in flight during the permutation are exactly the
    // ones the next XOR waits for (vmcnt counts in issue order; loads issued
    // before the XOR would make its wait drain them too and expose the whole
    // memory latency once per block).
    uint32_t cur[NL];
    const uint32_t hmask = 0u - (uint32_t)h;  // all ones on the odd lane
    if (a.dbg == 1 || a.dbg == 4) {
#pragma unroll
        for (int k = 0; k < NL; k++) cur[k] = lt + k;
    } else {
        load_block(0, cur);
    }
    for (int b = 0;; b++) {
        const bool full = end >= KECCAK_RATE * (b + 1);
        const bool more = end > KECCAK_RATE * (b + 1);
#pragma unroll
        for (int i = 0; i < 21; i++) {
            // stream word 2i + h + 1: the partner's word i (h = 0) or i + 1 (h = 1)
            // each lane sends the one word its partner needs (h ? cur[i] : cur[i + 1],
            // as a bitwise select: a C++ select of two array elements became a per-lane
            // index into a scratch copy of cur[]): one swap per word
            uint32_t nxt = 0u;
            if (sh) nxt = pair_swap<false>((uint32_t)__builtin_amdgcn_bitop3_b32(hmask, cur[i], cur[i + 1], 0xCA));
            s.a[i] ^= __builtin_amdgcn_alignbit(nxt, cur[i], amt);
        }
        if (!full) break;
        asm volatile("" ::: "memory");
        if (more && a.dbg != 1 && a.dbg != 4) load_block(b + 1, cur);
        if (a.dbg == 0 || a.dbg == 1) keccak_p12_pair<12, false>(s, h != 0);
        else if (a.dbg == 4) __builtin_amdgcn_s_sleep(72);  // resident, ~4.6k cycles per block, no VALU
        if (!more) break;
    }
#pragma unroll
    for (int i = 0; i < 25; i++) pst(sp + (size_t)(2 * i) * S, lbh, s.a[i]);
}

// Test hook (mastic_set_test_sponge_delay): one wave idles `ticks` periods of
// the constant wall clock, holding the stream it is queued on, so the work a
// prep_init queues there afterwards completes late.  No memory access.
__global__ __launch_bounds__(64) void k_spin(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
