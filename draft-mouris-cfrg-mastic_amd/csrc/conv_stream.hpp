// The convert streams of XofFixedKeyAes128: next_vec with rejection sampling,
// for the client-side shard kernel (ConvStream) and for the level kernel's
// exact fallback path.
#pragma once
#include "aes.hpp"
#include "field.hpp"

// ------------------------------------------------------------- convert stream
// XofFixedKeyAes128(seed, dst(ctx, CONVERT), nonce) after next(16):
// next_vec(field, VALUE_LEN) with rejection of candidates >= p.
template <class F> struct ConvStream;

template <> struct ConvStream<F64> {
    uint32_t seed[4];
    uint32_t blk[4];
    uint32_t ctr;
    uint32_t half;
    MH_D void init(const uint32_t s[4]) {
        seed[0] = s[0]; seed[1] = s[1]; seed[2] = s[2]; seed[3] = s[3];
        ctr = 1;
        half = 2;
    }
    // Common case: both children's streams need their next block at the same
    // element (no rejection so far): produce both in one paired AES call.
    template <class TT, class RK>
    MH_D void refill_pair(ConvStream& o, const TT& T, const RK& rk) {
        if (half == 2 && o.half == 2) {
            fixed_key_block2(T, rk, seed, ctr, o.seed, o.ctr, blk, o.blk);
            ctr++;
            o.ctr++;
            half = 0;
            o.half = 0;
        }
    }
    template <class TT, class RK>
    MH_D uint64_t next(const TT& T, const RK& rk) {
        uint64_t v;
        do {
            if (half == 2) {
                fixed_key_block(T, rk, seed, ctr, blk);
                ctr++;
                half = 0;
            }
            v = half ? (((uint64_t)blk[3] << 32) | blk[2]) : (((uint64_t)blk[1] << 32) | blk[0]);
            half++;
        } while (!F64::valid(v));
        return v;
    }
};

// The level kernel's exact stream (taken after a rejected candidate, or at the
// force_slow_blk test hook): one block buffered per node, i.e. two Field64
// candidates or one Field128 candidate.  Two sibling streams refill with one
// paired AES call (fixed_key_block_n<2>); a stream that rejected a candidate
// (probability ~2^-32) falls out of step with its sibling and refills alone,
// block by block, exactly as the reference's next_vec does.
// blk has room for two blocks and only the upper one, blk[4..7], is ever
// written or read: slots 0 and 1 (Field128: slot 0) of next()'s select never
// occur.  The lower block was a four-block lockstep refill's, which no kernel
// instantiated and which is gone.  Dropping the dead half as well (a blk[4],
// then one template over the field) leaves every kernel's size and resources
// alone but moves one or two instructions in each level kernel, so it is left
// to a change that measures it (profiles/r13_v1_device_split.txt).
template <class F> struct LevelStream;
template <> struct LevelStream<F64> {
    static constexpr int GROUP = 2;  // candidates per refill
    uint32_t seed[4];
    uint32_t blk[8];  // candidate i = blk[2i] | blk[2i+1] << 32
    uint32_t ctr;
    uint32_t pos;     // next candidate slot, 4 = empty
    MH_D void init(const uint32_t s[4]) {
        seed[0] = s[0]; seed[1] = s[1]; seed[2] = s[2]; seed[3] = s[3];
        ctr = 1;
        pos = 4;
    }
    template <class RK>
    MH_D void refill(LevelStream& o, const AesPerm& T, const RK& rk) {
        if (pos == 4 && o.pos == 4) {
            const uint32_t* const sd[2] = {seed, o.seed};
            const uint32_t cv[2] = {ctr, o.ctr};
            uint32_t* const ov[2] = {blk + 4, o.blk + 4};
            fixed_key_block_n<2>(T, rk, sd, cv, ov);
            ctr++;
            o.ctr++;
            pos = 2;
            o.pos = 2;
        }
    }
    template <class RK>
    MH_D uint64_t next(const AesPerm& T, const RK& rk) {
        uint64_t v;
        do {
            if (pos == 4) {
                const uint32_t* const sd[1] = {seed};
                const uint32_t cv[1] = {ctr};
                uint32_t* const ov[1] = {blk + 4};
                fixed_key_block_n<1>(T, rk, sd, cv, ov);
                ctr++;
                pos = 2;
            }
            const uint32_t lo = pos == 0 ? blk[0] : pos == 1 ? blk[2] : pos == 2 ? blk[4] : blk[6];
            const uint32_t hi = pos == 0 ? blk[1] : pos == 1 ? blk[3] : pos == 2 ? blk[5] : blk[7];
            v = ((uint64_t)hi << 32) | lo;
            pos++;
        } while (!F64::valid(v));
        return v;
    }
};

// Field128 counterpart: one candidate per block.
template <> struct LevelStream<F128> {
    static constexpr int GROUP = 1;
    uint32_t seed[4];
    uint32_t blk[8];  // candidate i = blk[4i .. 4i+3]
    uint32_t ctr;
    uint32_t pos;     // next candidate slot, 2 = empty
    MH_D void init(const uint32_t s[4]) {
        seed[0] = s[0]; seed[1] = s[1]; seed[2] = s[2]; seed[3] = s[3];
        ctr = 1;
        pos = 2;
    }
    template <class RK>
    MH_D void refill(LevelStream& o, const AesPerm& T, const RK& rk) {
        if (pos == 2 && o.pos == 2) {
            const uint32_t* const sd[2] = {seed, o.seed};
            const uint32_t cv[2] = {ctr, o.ctr};
            uint32_t* const ov[2] = {blk + 4, o.blk + 4};
            fixed_key_block_n<2>(T, rk, sd, cv, ov);
            ctr++;
            o.ctr++;
            pos = 1;
            o.pos = 1;
        }
    }
    template <class RK>
    MH_D F128::E next(const AesPerm& T, const RK& rk) {
        F128::E v;
        do {
            if (pos == 2) {
                const uint32_t* const sd[1] = {seed};
                const uint32_t cv[1] = {ctr};
                uint32_t* const ov[1] = {blk + 4};
                fixed_key_block_n<1>(T, rk, sd, cv, ov);
                ctr++;
                pos = 1;
            }
            uint32_t w[4];
#pragma unroll
            for (int i = 0; i < 4; i++) w[i] = pos == 0 ? blk[i] : blk[4 + i];
            v = F128::from_words(w);
            pos++;
        } while (!F128::valid(v));
        return v;
    }
};

template <> struct ConvStream<F128> {
    uint32_t seed[4];
    uint32_t blk[4];
    uint32_t ctr;
    uint32_t have;  // blk holds an unconsumed candidate
    MH_D void init(const uint32_t s[4]) {
        seed[0] = s[0]; seed[1] = s[1]; seed[2] = s[2]; seed[3] = s[3];
        ctr = 1;
        have = 0;
    }
    template <class TT, class RK>
    MH_D void refill(ConvStream& o, int, const TT& T, const RK& rk) {
        refill_pair(o, T, rk);
    }
    template <class TT, class RK>
    MH_D void refill_pair(ConvStream& o, const TT& T, const RK& rk) {
        if (!have && !o.have) {
            fixed_key_block2(T, rk, seed, ctr, o.seed, o.ctr, blk, o.blk);
            ctr++;
            o.ctr++;
            have = 1;
            o.have = 1;
        }
    }
    template <class TT, class RK>
    MH_D F128::E next(const TT& T, const RK& rk) {
        F128::E v;
        do {
            if (!have) {
                fixed_key_block(T, rk, seed, ctr, blk);
                ctr++;
            }
            have = 0;
            v = F128::from_words(blk);
        } while (!F128::valid(v));
        return v;
    }
};
