// Both aggregators' results together: the eval-proof Merkle tree, the prep
// message decision (k_decide, k_accept) and the wire encoding of result rows.
#pragma once
#include "flp.hpp"
#include "keccak.hpp"
#include "params.hpp"
#include "planes.hpp"

// ------------------------------------------------------------- proof tree
// VIDPF-proof aggregation mode (draft-mouris-cfrg-mastic.md, "Plain
// Heavy-Hitters with VIDPF-Proof Aggregation"): the aggregators compute
// identical eval proofs iff a report is valid, so they compare Merkle trees
// over the batch's eval proofs instead of exchanging every prep share, and
// descend into differing subtrees to isolate invalid reports.  The draft
// leaves the hash unspecified; here a node of two children is
//   XofTurboShake128(b'', dst(ctx, USAGE_PROOF_TREE = 12), left || right).next(32)
// and the last node of an odd level is promoted unchanged.  Nodes are 32-byte
// rows (node-major), levels concatenated leaves first.
__global__ __launch_bounds__(256) void k_proof_tree_leaves(const uint32_t* eval_proof, int n, int stride,
                                                          uint32_t* leaves) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
#pragma unroll
    for (int j = 0; j < 8; j++) leaves[(size_t)i * 8 + j] = eval_proof[(size_t)j * stride + i];
}

__global__ __launch_bounds__(256) void k_proof_tree_level(const PrefixState* pfx, const uint32_t* in, int n_in,
                                                         uint32_t* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n_out = (n_in + 1) >> 1;
    if (i >= n_out) return;
    const uint32_t* lr = in + (size_t)(2 * i) * 8;  // left || right: 16 consecutive words
    if (2 * i + 1 >= n_in) {
#pragma unroll
        for (int j = 0; j < 8; j++) out[(size_t)i * 8 + j] = lr[j];
        return;
    }
    KState s;
    int f;
    load_prefix(pfx, PFX_TREE, s, f);
    f = sponge_absorb_words(s, f, 64, [&](int m) { return lr[m]; });
    sponge_pad(s, f, 0x01);
    sponge_squeeze_words(s, 8, [&](int j, uint32_t w) { out[(size_t)i * 8 + j] = w; });
}

// ------------------------------------------------------------- decide
// prep_shares_to_prep (mastic.py:320-362) for a batch of report pairs.
// prep share wire: eval_proof || [jr_part] || [verifier]  (mastic.py:543-552)
template <class F>
__global__ __launch_bounds__(256) void k_decide(McParams p, int n, int stride, int weight_check,
                                                const uint8_t* ps0, const uint8_t* ps1, int ps_size,
                                                uint32_t* ver_scratch, const PrefixState* pfx,
                                                uint8_t* msg_out, uint8_t* status_out) {
    typedef typename F::E E;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint8_t* a = ps0 + (size_t)ps_size * r;
    const uint8_t* b = ps1 + (size_t)ps_size * r;
    // status: 1 = valid, 0 = VIDPF verification failed, 2 = FLP verification failed
    uint8_t st = 1;
    for (int i = 0; i < 32; i++)
        if (a[i] != b[i]) st = 0;
    if (st && weight_check) {
        const int jr = p.joint_rand_len > 0 ? 32 : 0;
        const uint8_t* va = a + 32 + jr;
        const uint8_t* vb = b + 32 + jr;
        for (int e = 0; e < p.verifier_len; e++) {
            uint32_t wa[F::W32], wb[F::W32];
            for (int i = 0; i < F::W32; i++) {
                wa[i] = ld_u32_bytes(va + e * F::ENC + 4 * i);
                wb[i] = ld_u32_bytes(vb + e * F::ENC + 4 * i);
            }
            E xa = F::from_words(wa), xb = F::from_words(wb);
            if (!F::valid(xa) || !F::valid(xb)) st = 2;
            pl_store<F>(ver_scratch, e, stride, r, F::add(xa, xb));
        }
        if (st == 1 && !flp_decide<F>(p, ver_scratch, stride, r)) st = 2;
        if (st == 1 && p.joint_rand_len > 0) {
            KState s;
            int f;
            load_prefix(pfx, PFX_JR_SEED, s, f);
            f = sponge_absorb_words(s, f, 64, [&](int m) {
                return m < 8 ? ld_u32_bytes(a + 32 + 4 * m) : ld_u32_bytes(b + 32 + 4 * (m - 8));
            });
            sponge_pad(s, f, 0x01);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                uint32_t w = kword(s, j);
                for (int i = 0; i < 4; i++) msg_out[(size_t)32 * r + 4 * j + i] = (uint8_t)(w >> (8 * i));
            }
        }
    }
    status_out[r] = st;
}

// ------------------------------------------------------------- wire encoding
// Planes -> report-major wire bytes on the device (mastic.py:537-552): row r
// of the output is the concatenation of up to 3 plane segments (seg[k]:
// words[k] planes of stride S), i.e. the prep share eval_proof || [jr_part]
// || [verifier] (encode_vec is little-endian words, the planes' byte order),
// or an out share (encode_vec of the truncated vector).  Consecutive threads
// on consecutive words of a row; a grid-stride loop over the output words (a
// grid's work-items must stay below 2^32, an output may be larger: C2's
// 12,288 x 10k-prefix out shares are 2.5e9 words).
struct RowSegs {
    const uint32_t* seg[3];
    int words[3];
};
// (k_gather_rows, the planes-to-wire-rows overload; rows_kernels.hpp has the row-gathering one of compaction)
__global__ __launch_bounds__(256) void k_gather_rows(RowSegs sg, int n, int stride, uint32_t* out) {
    const size_t row_words = (size_t)sg.words[0] + sg.words[1] + sg.words[2];
    const size_t total = (size_t)n * row_words;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int r = (int)(i / row_words);
        int k = (int)(i - (size_t)r * row_words);
        int s = 0;
        while (k >= sg.words[s]) {
            k -= sg.words[s];
            s++;
        }
        out[i] = sg.seg[s][(size_t)k * stride + r];
    }
}

// Both aggregators' prep_shares_to_prep + prep_next outcome per report, from
// k_decide's code, the two query statuses and (weight check with joint
// randomness) the joint-rand confirmation of each aggregator
// (mastic.py:364-377): accept = 1 iff all pass.
__global__ __launch_bounds__(256) void k_accept(int n, int stride, int check_jr, const uint8_t* code,
                                                const int32_t* st0, const int32_t* st1, const uint8_t* msg,
                                                const uint32_t* jrs0, const uint32_t* jrs1, uint8_t* accept) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    bool ok = code[r] == 1 && st0[r] == 0 && st1[r] == 0;
    if (check_jr) {
        for (int j = 0; j < 8; j++) {
            const uint32_t m = ld_u32_bytes(msg + (size_t)32 * r + 4 * j);
            ok = ok && m == jrs0[(size_t)j * stride + r] && m == jrs1[(size_t)j * stride + r];
        }
    }
    accept[r] = ok ? 1 : 0;
}
