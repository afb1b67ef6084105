// Prefix sponge states (the TurboSHAKE state after each domain-separation
// prefix, absorbed once per context) and Planes, the per-report word planes
// that the kernels of a prep_init read and write (layout: kernels.hpp).
#pragma once
#include "keccak.hpp"

// ------------------------------------------------------------- prefix states
enum PfxId {
    PFX_EXT = 0,        // XofFixedKeyAes128 key, usage EXTEND  (D = 2)
    PFX_CONV,           // XofFixedKeyAes128 key, usage CONVERT (D = 2)
    PFX_NODE,           // node proof, seed length 16
    PFX_ONEHOT,         // onehot check, empty seed
    PFX_PAYLOAD,        // payload check, empty seed
    PFX_EVAL,           // eval proof, verify key as seed
    PFX_QUERY,          // query rand, verify key as seed
    PFX_PROOF_SHARE,    // helper proof share, 32-byte seed follows
    PFX_JR_PART,        // joint rand part, 32-byte seed follows
    PFX_JR_SEED,        // joint rand seed, empty seed
    PFX_JR,             // joint rand, 32-byte seed follows
    PFX_PROVE_RAND,     // prove rand (client), 32-byte seed follows
    PFX_TREE,           // eval-proof Merkle tree node hash (proof-aggregation mode), empty seed
    PFX_COUNT
};

struct PrefixState {
    KState st;
    int f;
    int pad[3];
};

__global__ void k_prefix_states(const uint8_t* bytes, const int* offs, const int* lens, int count,
                                PrefixState* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int i = 0; i < count; i++) {
        KState s;
        kstate_zero(s);
        int f = sponge_absorb_bytes_slow(s, 0, bytes + offs[i], lens[i]);
        out[i].st = s;
        out[i].f = f;
    }
}

MH_D void load_prefix(const PrefixState* ps, int id, KState& s, int& f) {
    s = ps[id].st;
    f = ps[id].f;
}

MH_D uint32_t ld_u32_bytes(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// ------------------------------------------------------------- planes
struct Planes {
    int n, stride;
    // report inputs (unpacked)
    uint32_t* key;       // [4]
    uint32_t* nonce;     // [4]
    uint32_t* cw_seed;   // [bits][4]
    uint32_t* cw_ctrl;   // [bits]
    uint32_t* cw_w;      // [bits][vl*w32]
    uint32_t* cw_proof;  // [bits][8]
    uint32_t* lps;       // [proof_len*w32] leader proof share (agg 0)
    uint32_t* seed;      // [8]  FLP seed (agg 1: helper seed, agg 0: leader seed)
    uint32_t* peer;      // [8]  peer joint rand part
    uint32_t* rk_ext;    // [44]
    uint32_t* rk_conv;   // [44]
    // sponges
    uint32_t* sp_onehot;   // [50]
    uint32_t* sp_payload;  // [50]
    // results
    uint32_t* rootsum;     // [vl*w32]   w_L0 + w_R0 (raw)
    uint32_t* beta;        // [vl*w32]   beta share (negated for agg 1)
    uint32_t* eval_proof;  // [8]
    uint32_t* proof;       // [proof_len*w32]
    uint32_t* qr;          // [qrl*w32]
    uint32_t* jr;          // [jrl*w32]
    uint32_t* jr_part;     // [8]
    uint32_t* jr_seed;     // [8]
    uint32_t* verifier;    // [verifier_len*w32]
    int32_t* status;       // [1]
};
