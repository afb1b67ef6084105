// The replay set of an aggregator (mastic_nonce_set): the keyed hash of a
// 16-byte nonce, the probe step, and the rules that size its slot table and
// key arena.  Plain C++17, no HIP: nonce_set_kernels.hpp probes with these
// functions on the device, mastic_hip.hip sizes the set's buffers with them,
// and tests/host/nonce_set_host.cpp runs a sequential model of the kernels on
// them on a CPU under ASan / UBSan.
//
// Layout.  The keys live in an append-only arena, keys[id][4 words].  The slot
// table is open addressing over 32-bit words: 0 = empty, else id + 1, where
// id < count names an arena key and, during an admit of n nonces into a set of
// `count`, id = count + i names nonce i of the batch.  Slots are never
// vacated.  The table is a power of two and at least 2 * (count + n) slots
// before the first insert of an admit, so it is never more than half full and
// a probe always meets an empty slot.
#pragma once
#ifdef __HIP__
#include "common.hpp"
#else
#include <stdint.h>
#define MH_HD inline
#endif

struct NsKey {
    uint32_t w[4];
};
MH_HD bool ns_key_eq(const NsKey& a, const NsKey& b) {
    return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && a.w[3] == b.w[3];
}

// The set's 128-bit hash secret.  Clients choose their nonces, so the home
// slot of a nonce must not be computable without it (an unkeyed hash lets a
// client build one long probe chain).
struct NsHashKey {
    uint64_t k0, k1;
};

MH_HD uint64_t ns_rotl(uint64_t x, int b) { return (x << b) | (x >> (64 - b)); }
MH_HD void ns_sipround(uint64_t& v0, uint64_t& v1, uint64_t& v2, uint64_t& v3) {
    v0 += v1;
    v1 = ns_rotl(v1, 13);
    v1 ^= v0;
    v0 = ns_rotl(v0, 32);
    v2 += v3;
    v3 = ns_rotl(v3, 16);
    v3 ^= v2;
    v0 += v3;
    v3 = ns_rotl(v3, 21);
    v3 ^= v0;
    v2 += v1;
    v1 = ns_rotl(v1, 17);
    v1 ^= v2;
    v2 = ns_rotl(v2, 32);
}
// SipHash-C-D (Aumasson, Bernstein 2012) of the 16 bytes of a nonce, words
// little-endian: two message blocks and the length block.  <2, 4> is the
// published function (its test vector is checked on the host); the set uses
// <1, 3>, the hash-table strength.
template <int C, int D>
MH_HD uint64_t ns_siphash(const NsHashKey& k, const NsKey& x) {
    uint64_t v0 = k.k0 ^ 0x736f6d6570736575ull, v1 = k.k1 ^ 0x646f72616e646f6dull;
    uint64_t v2 = k.k0 ^ 0x6c7967656e657261ull, v3 = k.k1 ^ 0x7465646279746573ull;
    const uint64_t m[3] = {(uint64_t)x.w[0] | ((uint64_t)x.w[1] << 32), (uint64_t)x.w[2] | ((uint64_t)x.w[3] << 32),
                           (uint64_t)16 << 56};
    for (int i = 0; i < 3; i++) {
        v3 ^= m[i];
        for (int r = 0; r < C; r++) ns_sipround(v0, v1, v2, v3);
        v0 ^= m[i];
    }
    v2 ^= 0xff;
    for (int r = 0; r < D; r++) ns_sipround(v0, v1, v2, v3);
    return v0 ^ v1 ^ v2 ^ v3;
}
MH_HD uint64_t ns_hash(const NsHashKey& k, const NsKey& x) { return ns_siphash<1, 3>(k, x); }

// Home slot and probe step of a table of `slots` (a power of two) slots:
// linear probing, so equal keys walk the same slots in the same order.
MH_HD uint32_t ns_home(const NsHashKey& k, const NsKey& x, uint32_t slots) { return (uint32_t)ns_hash(k, x) & (slots - 1); }
MH_HD uint32_t ns_next(uint32_t slot, uint32_t slots) { return (slot + 1) & (slots - 1); }

// ------------------------------------------------------------ sizing (host)
// Ids are 32-bit and a slot holds id + 1; the slot count must fit 32 bits too.
constexpr uint64_t NS_MAX_KEYS = (uint64_t)1 << 30;
constexpr uint64_t NS_MIN_SLOTS = 1024;

// Slots of a table that is to hold `keys` keys (the set's count plus every
// nonce of the batch about to be admitted, as if all were fresh): the least
// power of two >= 2 * keys, at least NS_MIN_SLOTS.  keys <= NS_MAX_KEYS.
inline uint64_t ns_table_slots(uint64_t keys) {
    uint64_t s = NS_MIN_SLOTS;
    while (s < 2 * keys) s <<= 1;
    return s;
}
// Growth rule of the table: it is replaced (and the arena's ids re-inserted)
// only when it is too small for `keys`, and then by ns_table_slots(keys).
inline uint64_t ns_grown_slots(uint64_t slots, uint64_t keys) { return slots >= 2 * keys && slots ? slots : ns_table_slots(keys); }
// Growth rule of the arena (in keys) under a table of `slots`: it is replaced
// only when it is too small for `keys`, and then sized so that table plus
// arena stay within 32 bytes per key above the minimum table:
// 4 * slots + 16 * cap <= 32 * keys  <=>  cap <= 2 * keys - slots / 4.
// A table just grown (keys barely over slots / 4) leaves no headroom, and the
// headroom doubles with the distance from there, up to the slots / 2 keys the
// table can take: log2(slots) arena copies per table size at the worst.
inline uint64_t ns_arena_keys(uint64_t slots, uint64_t keys) {
    if (slots <= NS_MIN_SLOTS) return slots / 2;
    const uint64_t room = 2 * keys > slots / 4 ? 2 * keys - slots / 4 : 0;
    const uint64_t cap = room < slots / 2 ? room : slots / 2;
    return cap > keys ? cap : keys;
}
inline uint64_t ns_grown_arena(uint64_t cap, uint64_t slots, uint64_t keys) { return cap >= keys && cap ? cap : ns_arena_keys(slots, keys); }
// Device bytes of a set sized by these rules.
inline uint64_t ns_set_bytes(uint64_t slots, uint64_t arena_keys) { return 4 * slots + 16 * arena_keys; }
