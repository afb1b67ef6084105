// Vidpf.node_proof: the body of one node proof (node_proof_one) and the
// kernel that computes a level's proofs on its own (k_node_proof); the level
// kernel's proof waves (level_kernel.hpp) call the same body.
#pragma once
#include "keccak.hpp"
#include "params.hpp"
#include "planes.hpp"

// ------------------------------------------------------------- node proof body
#define NP_WIN 14
template <int Q>
MH_D void np_xor_window(KState& s, const uint32_t* x) {
#pragma unroll
    for (int k = 0; k < NP_WIN; k++)
        if (Q + k < KECCAK_RATE_WORDS) kxor_word(s, Q + k, x[k]);
}
template <int Q>
MH_D void np_xor_overflow(KState& s, const uint32_t* x) {
#pragma unroll
    for (int k = 0; k < NP_WIN; k++)
        if (Q + k >= KECCAK_RATE_WORDS) kxor_word(s, Q + k - KECCAK_RATE_WORDS, x[k]);
}
#define NP_CASES(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) \
    M(15) M(16) M(17) M(18) M(19) M(20) M(21) M(22) M(23) M(24) M(25) M(26) M(27) M(28) M(29) M(30) \
    M(31) M(32) M(33) M(34) M(35) M(36) M(37) M(38) M(39) M(40) M(41)

// One node proof: TurboSHAKE128 over the pre-absorbed prefix state np (fill
// position f) and the body  seed || le16(BITS) || le16(level) || path,
// XORed with the level's proof correction word when the node's control bit
// t is set.  Writes 8 words through `put(j, w)`.  All positions uniform.
template <bool FUSE_D = true, class Put>
MH_D void node_proof_one(const PrefixState* np, int f, int bits, int level, int path_bytes, const uint32_t seed[4],
                         const uint32_t* path, uint32_t t, const uint32_t pcw[8], Put put) {
    const int q = f >> 2;
    const int sh = f & 3;
    const int nbytes = 20 + path_bytes;  // body; the domain byte 0x01 follows
    const bool cross = f + nbytes >= KECCAK_RATE;
    const uint32_t amt = (32 - 8 * sh) & 31;
    const int dw = nbytes >> 2;
    const uint32_t dbit = 1u << (8 * (nbytes & 3));
    uint32_t B[NP_WIN];
#pragma unroll
    for (int i = 0; i < 4; i++) B[i] = seed[i];
    B[4] = (uint32_t)bits | ((uint32_t)level << 16);
#pragma unroll
    for (int k = 5; k < NP_WIN; k++) B[k] = k - 5 < 8 ? path[k - 5] : 0u;
#pragma unroll
    for (int k = 4; k < NP_WIN; k++) B[k] |= (k == dw) ? dbit : 0u;
    uint32_t x[NP_WIN];
#pragma unroll
    for (int k = 0; k < NP_WIN; k++) {
        const uint32_t hi = B[k];
        const uint32_t lo = k ? B[k - 1] : 0u;
        x[k] = sh ? __builtin_amdgcn_alignbit(hi, lo, amt) : hi;
    }
    asm volatile("" ::: "memory");  // re-read the uniform prefix state, do not pin 50 registers
    KState s = np->st;
    switch (q) {
#define NP_W(Q) case Q: np_xor_window<Q>(s, x); break;
        NP_CASES(NP_W)
#undef NP_W
    }
    if (cross) {
        keccak_p12<12, FUSE_D>(s);
        switch (q) {
#define NP_O(Q) case Q: np_xor_overflow<Q>(s, x); break;
            NP_CASES(NP_O)
#undef NP_O
        }
    }
    s.a[20].hi ^= 0x80000000u;
    keccak_p12<12, FUSE_D>(s);
#pragma unroll
    for (int j = 0; j < 8; j++) put(j, kword(s, j) ^ (t ? pcw[j] : 0u));
}

// ------------------------------------------------------------- node proofs
// TurboSHAKE128(seed, dst(ctx, NODE_PROOF), le16(BITS) || le16(l) || path)
// (vidpf.py:366-380), XORed with the proof CW when the node's control bit is
// set (vidpf.py:321-323).  The prefix le16(len(dst)) || dst || u8(16) is
// pre-absorbed (PrefixState); the body plus the domain byte (<= 14 words)
// lands at the uniform fill position f: a switch on f/4 selects a straight-
// line XOR pattern, so no LDS staging and no per-lane indexing is needed.
struct ProofArgs {
    int oh_gstride;      // words per report group of the (tiled) proof buffer
    int bin_rstride;     // words between consecutive words of a report
    int level;
    int n_nodes;
    int npw;             // nodes per wave
    int path_bytes;      // ceil((level + 1) / 8)
    const uint32_t* child_path;  // [n_nodes][8]
    const uint32_t* cs;          // child seeds of this level [node][5]
    uint32_t* onehot;            // [n_nodes * 8]
    const PrefixState* np;       // node-proof prefix state (device memory)
    int f;                       // its fill position
};

__global__ __launch_bounds__(256) void k_node_proof(McParams p, Planes pl, ProofArgs a) {
    const int S = pl.stride;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = blockIdx.x * 64 + lane;
    const uint32_t lb = (uint32_t)r * 4u;
    const int nbeg = (blockIdx.y * 4 + wave) * a.npw;
    if (nbeg >= a.n_nodes) return;
    const int nend = min(nbeg + a.npw, a.n_nodes);
    const int l = a.level;
    uint32_t* ohg = a.onehot + (size_t)blockIdx.x * a.oh_gstride;  // tiled proof buffer of this group
    const uint32_t lt = (uint32_t)lane * 4u;
    uint32_t pcw[8];
#pragma unroll
    for (int j = 0; j < 8; j++) pcw[j] = pld(pl.cw_proof + ((size_t)l * 8 + j) * S, lb);
    for (int node = nbeg; node < nend; node++) {
        uint32_t seed[4];
#pragma unroll
        for (int i = 0; i < 4; i++) seed[i] = pld(a.cs + ((size_t)node * 5 + i) * S, lb);
        const uint32_t t = pld(a.cs + ((size_t)node * 5 + 4) * S, lb);
        node_proof_one(a.np, a.f, p.bits, l, a.path_bytes, seed, a.child_path + node * 8, t, pcw,
                       [&](int j, uint32_t w) { pst(ohg + ((size_t)node * 8 + j) * a.bin_rstride, lt, w); });
    }
}
