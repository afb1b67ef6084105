// Wire reports into planes: the range check of the wire field elements, the
// unpacking of a report's public and input share, and the per-report key setup
// (the two fixed AES key schedules, the start of both binder sponges).
#pragma once
#include "aes.hpp"
#include "keccak.hpp"
#include "params.hpp"
#include "planes.hpp"

// ------------------------------------------------------------- unpack
// per-report verdict of k_validate_wire (mastic_reports::wire_flags)
#define WIRE_BAD_PUB 1u  // a payload correction word element >= p
#define WIRE_BAD_LPS 2u  // a leader proof share element >= p
// nw little-endian words of one report's wire row into plane rows dst[k * step].
// A == 8: the row, the segment and every report's row start are 8-byte aligned
// (the common case: BITS a multiple of 32), so a lane reads two words per load
// instead of eight byte loads (each lane reads its own row: every load of the
// wave touches 64 cache lines, so the instruction count is what costs).
template <int A>
MH_D void unpack_words(const uint8_t* src, int nw, uint32_t* dst, size_t step) {
    if constexpr (A == 8) {
        const uint2* s2 = (const uint2*)src;
        int k = 0;
        for (; k + 1 < nw; k += 2) {
            const uint2 v = s2[k >> 1];
            dst[(size_t)k * step] = v.x;
            dst[(size_t)(k + 1) * step] = v.y;
        }
        if (k < nw) dst[(size_t)k * step] = ((const uint32_t*)src)[k];
    } else {
        for (int k = 0; k < nw; k++) dst[(size_t)k * step] = ld_u32_bytes(src + 4 * k);
    }
}

// Wire public share: pack_bits(ctrl) || seed_cw[B] || w_cw[B] || proof_cw[B]
// (poc/vidpf.py:382-394).  Input share: key || [leader proof share] || [seed]
// || [peer jr part] (poc/mastic.py:516-529).
// big = false: every segment; big = true: the correction words and the
// leader proof share are left to k_rows_to_planes (coalesced row tiles).
template <int A>
MH_D void unpack_report(const McParams& p, const Planes& pl, int agg_id, int r, const uint8_t* ps, const uint8_t* is,
                        const uint8_t* nc, int l_lo, int l_hi, bool big = false) {
    const size_t S = (size_t)pl.stride;
    const int nctrl = (2 * p.bits + 7) / 8;
    const int wl = p.value_len * p.w32;
    unpack_words<A>(nc, 4, pl.nonce + r, S);
    unpack_words<A>(is, 4, pl.key + r, S);
    for (int l = l_lo; l < l_hi; l++) {
        uint32_t c0 = (ps[(2 * l) >> 3] >> ((2 * l) & 7)) & 1;
        uint32_t c1 = (ps[(2 * l + 1) >> 3] >> ((2 * l + 1) & 7)) & 1;
        pl.cw_ctrl[(size_t)l * S + r] = c0 | (c1 << 1);
        if (big) continue;
        unpack_words<A>(ps + nctrl + 16 * l, 4, pl.cw_seed + (size_t)l * 4 * S + r, S);
        unpack_words<A>(ps + nctrl + 16 * p.bits + (size_t)l * p.value_len * p.enc, wl,
                        pl.cw_w + (size_t)l * wl * S + r, S);
        unpack_words<A>(ps + nctrl + 16 * p.bits + (size_t)p.bits * p.value_len * p.enc + 32 * l, 8,
                        pl.cw_proof + (size_t)l * 8 * S + r, S);
    }
    const uint8_t* q = is + 16;
    if (agg_id == 0) {
        if (!big) unpack_words<A>(q, p.proof_len * p.w32, pl.lps + r, S);
        q += (size_t)p.proof_len * p.enc;
    }
    if (agg_id == 1 || p.joint_rand_len > 0) {
        unpack_words<A>(q, 8, pl.seed + r, S);
        q += 32;
    }
    if (p.joint_rand_len > 0) unpack_words<A>(q, 8, pl.peer + r, S);
}

__global__ __launch_bounds__(256) void k_unpack(McParams p, Planes pl, int agg_id, const uint8_t* nonces,
                                                const uint8_t* pub, const uint8_t* ins, int l_lo, int l_hi,
                                                int big, const uint8_t* wire_flags) {
    // correction words of levels l_lo .. l_hi-1 only: a call at level L never
    // reads deeper ones, and a frontier-cache hit only reads level L's
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= pl.n) return;
    const size_t ps_size = mc_public_share_size(p);
    const size_t is_size = mc_input_share_size(p, agg_id);
    const uint8_t* ps = pub + ps_size * r;
    const uint8_t* is = ins + is_size * r;
    const uint8_t* nc = nonces + 16 * (size_t)r;
    const size_t nctrl = (2 * p.bits + 7) / 8;
    // every segment offset is nctrl plus multiples of 8 bytes (enc is 8 or 16)
    const bool a8 = (((uintptr_t)pub | (uintptr_t)ins | (uintptr_t)nonces | ps_size | is_size | nctrl) & 7) == 0;
    if (a8)
        unpack_report<8>(p, pl, agg_id, r, ps, is, nc, l_lo, l_hi, big != 0);
    else
        unpack_report<1>(p, pl, agg_id, r, ps, is, nc, l_lo, l_hi);
    // k_validate_wire's verdict on this aggregator's inputs (the status plane
    // was cleared just before; k_flp_query may still overwrite it with -2)
    if (wire_flags[r] & (agg_id == 0 ? WIRE_BAD_PUB | WIRE_BAD_LPS : WIRE_BAD_PUB)) pl.status[r] = -3;
}

// Field.decode_vec's range check (vdaf_poc field.py: "encoded element out of
// range") over a report's wire field elements: the payload correction words of
// every level of the public share (pub != nullptr) and the leader proof share
// (in0 != nullptr).  Runs once per upload / shard, not per prep_init: the
// verdict is kept per report (flags[r], WIRE_BAD_* bits; the bits of the
// segments given are replaced) and k_unpack turns it into status -3.  One wave
// per report, lanes on consecutive elements.
template <class F>
__global__ __launch_bounds__(256) void k_validate_wire(McParams p, int n, const uint8_t* pub, const uint8_t* in0,
                                                       uint8_t* flags) {
    const int r = blockIdx.x * 4 + (int)(threadIdx.x >> 6);  // wave-uniform
    const int lane = threadIdx.x & 63;
    if (r >= n) return;
    auto any_bad = [&](const uint8_t* src, int count) {
        const bool a4 = ((uintptr_t)src & 3) == 0;
        bool bad = false;
        for (int e = lane; e < count; e += 64) {
            uint32_t w[F::W32];
            const uint8_t* q = src + (size_t)e * F::ENC;
#pragma unroll
            for (int i = 0; i < F::W32; i++) w[i] = a4 ? ((const uint32_t*)q)[i] : ld_u32_bytes(q + 4 * i);
            bad |= !F::valid(F::from_words(w));
        }
        return __any(bad) != 0;
    };
    uint8_t set = 0, mask = 0;
    if (pub) {
        const size_t nctrl = (2 * p.bits + 7) / 8;
        mask |= WIRE_BAD_PUB;
        if (any_bad(pub + (size_t)mc_public_share_size(p) * r + nctrl + 16 * (size_t)p.bits, p.bits * p.value_len))
            set |= WIRE_BAD_PUB;
    }
    if (in0) {
        mask |= WIRE_BAD_LPS;
        if (any_bad(in0 + (size_t)mc_input_share_size(p, 0) * r + 16, p.proof_len)) set |= WIRE_BAD_LPS;
    }
    if (lane == 0) flags[r] = (uint8_t)((flags[r] & ~mask) | set);
}

// Words [0, nwords) of every report's wire row (row r at src + r * row_bytes,
// 8-byte aligned) into plane rows: dst[j * S + r] = word j of row r.  With one
// lane per report (k_unpack) every load of a wave touches 64 rows, i.e. 64
// cache lines for 8 bytes each (C5: 32 ms for its 526 KB public shares at
// 16,384 reports, ~0.5 TB/s); here a workgroup moves a tile of 64 reports x
// 64 words through LDS: each half-wave reads 256 contiguous bytes of one row,
// each wave writes 256 contiguous bytes of one plane row.
__global__ __launch_bounds__(256) void k_rows_to_planes(const uint8_t* src, size_t row_bytes, int n, int nwords,
                                                        uint32_t* dst, int S) {
    __shared__ uint32_t tile[64 * 65];  // [report][word], pitch 65: the transposed reads hit 64 banks
    const int r0 = blockIdx.x * 64, j0 = blockIdx.y * 64;
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int q = k * 256 + t;
        const int rr = q >> 5, wp = q & 31;  // report of the tile, word pair
        const int j = j0 + 2 * wp;
        uint2 v = make_uint2(0u, 0u);
        if (r0 + rr < n) {
            const uint8_t* row = src + (size_t)(r0 + rr) * row_bytes;
            if (j + 1 < nwords)
                v = *(const uint2*)(row + 4 * (size_t)j);
            else if (j < nwords)
                v.x = *(const uint32_t*)(row + 4 * (size_t)j);
        }
        tile[rr * 65 + 2 * wp] = v.x;
        tile[rr * 65 + 2 * wp + 1] = v.y;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const int q = k * 256 + t;
        const int jj = q >> 6, rr = q & 63;
        if (r0 + rr < n && j0 + jj < nwords) dst[(size_t)(j0 + jj) * S + r0 + rr] = tile[rr * 65 + jj];
    }
}

// ------------------------------------------------------------- key setup
// The two fixed AES keys of a report depend only on (ctx, usage, nonce)
// (vdaf_poc XofFixedKeyAes128): derive them once, expand once.  sponges:
// also start both binder sponges (not on a frontier-cache hit, which resumes
// them from the cache's planes).
__global__ __launch_bounds__(256) void k_setup(Planes pl, const PrefixState* pfx, int sponges) {
    __shared__ uint32_t T[AES_LDS_WORDS];
    aes_lds_fill(T, threadIdx.x, 256);
    __syncthreads();
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= pl.stride) return;
    const int S = pl.stride;
    AesLds TL{T + (threadIdx.x & 31)};
    for (int which = 0; which < 2; which++) {
        KState s;
        int f;
        load_prefix(pfx, which == 0 ? PFX_EXT : PFX_CONV, s, f);
        f = sponge_absorb_words(s, f, 16, [&](int m) { return pl.nonce[m * S + r]; });
        sponge_pad(s, f, 0x02);
        uint32_t key[4] = {s.a[0].lo, s.a[0].hi, s.a[1].lo, s.a[1].hi};
        uint32_t rk[44];
        aes128_expand(TL, key, rk);
        uint32_t* dst = which == 0 ? pl.rk_ext : pl.rk_conv;
#pragma unroll
        for (int i = 0; i < 44; i++) dst[i * S + r] = rk[i];
    }
    if (!sponges) return;
    KState s;
    int f;
    load_prefix(pfx, PFX_ONEHOT, s, f);
#pragma unroll
    for (int i = 0; i < 25; i++) {
        pl.sp_onehot[(2 * i) * S + r] = s.a[i].lo;
        pl.sp_onehot[(2 * i + 1) * S + r] = s.a[i].hi;
    }
    load_prefix(pfx, PFX_PAYLOAD, s, f);
#pragma unroll
    for (int i = 0; i < 25; i++) {
        pl.sp_payload[(2 * i) * S + r] = s.a[i].lo;
        pl.sp_payload[(2 * i + 1) * S + r] = s.a[i].hi;
    }
}
