// Kernels of the replay set (mastic_nonce_set; layout and hash in
// nonce_set.hpp).  One lane per nonce, 256 lanes per workgroup.
//
// An admit of n nonces into a set of `count` keys is three launches on the
// ctx's main stream: k_ns_insert, k_ns_resolve, k_ns_commit.
//
// Memory rules.  A slot word is read and written only through relaxed
// agent-scope atomics: a plain load could be served from this CU's L1 or this
// XCD's L2 with a value another XCD has since replaced.  Keys are read with
// plain loads: the batch's nonces are written before the admit's first launch,
// and arena keys are appended only by k_ns_commit, which probes nothing, so no
// launch reads a key that the same launch writes.
//
// No lane waits for another.  Every probe loop runs at most `slots` steps; the
// table is at most half full, so a probe meets its key or an empty slot long
// before that, and one that does not sets err[NS_ERR] and gives up.
#pragma once
#include "nonce_set.hpp"

enum { NS_ERR = 0, NS_FRESH = 1, NS_WORDS = 4 };  // the set's device words (zeroed before every admit / query)
constexpr uint32_t NS_NO_SLOT = 0xffffffffu;

struct NsTable {
    uint32_t* slot;      // [slots]
    const uint4* keys;   // arena [count]
    uint32_t slots;      // power of two
    uint32_t count;      // arena keys; ids >= count name nonces of the batch
    NsHashKey hk;
};

__device__ __forceinline__ NsKey ns_load_key(const uint4* p, size_t i) {
    const uint4 v = p[i];
    return NsKey{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ uint32_t ns_slot_load(uint32_t* s) {
    return __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The key an occupied slot's word v names: an arena key or a nonce of the batch.
__device__ __forceinline__ NsKey ns_occupant(const NsTable& t, const uint4* batch, uint32_t v) {
    const uint32_t id = v - 1;
    return id < t.count ? ns_load_key(t.keys, id) : ns_load_key(batch, id - t.count);
}

// Insert.  Lane i claims the first empty slot of its probe sequence with
// id + 1 = count + i + 1, unless it meets its own key first: in an arena slot
// (a replay of the set: nothing to do) or in a slot another lane of the batch
// claimed, which then keeps the smaller of the two ids.  Equal keys walk the
// same sequence and slots are never vacated, so every copy of a key ends at
// the one slot the first claimant took, and after the launch that slot holds
// the smallest index of the key in the batch: atomicMin is commutative, so
// the result does not depend on the order in which the lanes arrive.  A slot
// claimed under a lane's feet (the compare-and-swap fails) is examined like
// any occupied slot, with the value the swap returned.  A slot's word may drop
// from one batch id to a smaller one at any time, but both name the same key,
// so a comparison made against the earlier occupant stays right.
__global__ __launch_bounds__(256) void k_ns_insert(NsTable t, const uint4* batch, uint32_t n, uint32_t* err) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const NsKey me = ns_load_key(batch, i);
    const uint32_t mine = t.count + i + 1;
    uint32_t s = ns_home(t.hk, me, t.slots);
    for (uint32_t step = 0; step < t.slots; step++, s = ns_next(s, t.slots)) {
        uint32_t v = ns_slot_load(t.slot + s);
        if (v == 0) {
            uint32_t expect = 0;
            if (__hip_atomic_compare_exchange_strong(t.slot + s, &expect, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT))
                return;
            v = expect;
        }
        if (ns_key_eq(ns_occupant(t, batch, v), me)) {
            if (v > t.count) __hip_atomic_fetch_min(t.slot + s, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    __hip_atomic_store(err + NS_ERR, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Resolve (after every insert: the next launch).  Lane i walks to its key's
// slot: fresh[i] = 1 iff that slot names nonce i itself, i.e. the key was not
// in the set and i is its first index in the batch.  slot_of[i] is that slot
// for a fresh nonce (k_ns_commit rewrites it), NS_NO_SLOT otherwise.
// batch == nullptr is the query: every id is an arena id, found[i] = 1 iff the
// key is in the table, and nothing is written but found.
__global__ __launch_bounds__(256) void k_ns_resolve(NsTable t, const uint4* batch, const uint4* query, uint32_t n,
                                                    uint8_t* fresh, uint32_t* slot_of, uint32_t* err) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const bool admit = batch != nullptr;
    const NsKey me = ns_load_key(admit ? batch : query, i);
    const uint32_t mine = t.count + i + 1;
    uint32_t s = ns_home(t.hk, me, t.slots);
    uint8_t hit = 0;
    uint32_t at = NS_NO_SLOT;
    bool bad = true;  // until the probe ends at its key or, for a query, at an empty slot
    for (uint32_t step = 0; step < t.slots; step++, s = ns_next(s, t.slots)) {
        const uint32_t v = ns_slot_load(t.slot + s);
        if (v == 0) {
            bad = admit;  // an admit's nonce was inserted, so its probe cannot end at an empty slot
            break;
        }
        if (!admit && v > t.count) break;  // a table that still holds batch ids: an admit did not finish
        if (ns_key_eq(ns_occupant(t, batch, v), me)) {
            hit = admit ? (v == mine) : 1;
            if (admit && hit) at = s;
            bad = false;
            break;
        }
    }
    if (bad) __hip_atomic_store(err + NS_ERR, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    fresh[i] = hit;
    if (slot_of) slot_of[i] = at;
}

// Commit (after resolve: the next launch).  Every fresh nonce takes the next
// arena id, appends its key and rewrites its slot, so the table holds arena
// ids only again.  The ids come from one counter, one atomic per wave: the
// wave's fresh lanes are counted with a ballot, lane 0 of them adds the count
// and the base is broadcast.  Which wave gets which ids depends on arrival, so
// the arena's order is unspecified; no result reads it.
__global__ __launch_bounds__(256) void k_ns_commit(uint32_t* slot, uint4* keys, uint32_t count, const uint4* batch,
                                                   uint32_t n, const uint8_t* fresh, const uint32_t* slot_of,
                                                   uint32_t* words) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool f = i < n && fresh[i] != 0;
    const unsigned long long m = __ballot(f);
    if (m == 0) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader)
        base = __hip_atomic_fetch_add(words + NS_FRESH, (uint32_t)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, leader);
    if (!f) return;
    const uint32_t id = count + base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
    keys[id] = batch[i];
    __hip_atomic_store(slot + slot_of[i], id + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Growth: re-insert arena ids 0..n-1 into a larger, zeroed table.
// The keys are distinct, so a lane only ever looks for an empty slot.
__global__ __launch_bounds__(256) void k_ns_rehash(NsTable t, uint32_t n, uint32_t* err) {
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id >= n) return;
    const NsKey me = ns_load_key(t.keys, id);
    uint32_t s = ns_home(t.hk, me, t.slots);
    for (uint32_t step = 0; step < t.slots; step++, s = ns_next(s, t.slots)) {
        if (ns_slot_load(t.slot + s) != 0) continue;
        uint32_t expect = 0;
        if (__hip_atomic_compare_exchange_strong(t.slot + s, &expect, id + 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
    }
    __hip_atomic_store(err + NS_ERR, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
