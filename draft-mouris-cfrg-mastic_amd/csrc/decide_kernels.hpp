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

// ------------------------------------------------------------- decide against a peer
// One aggregator of two (mastic_decide_peer): prep_shares_to_prep plus this
// aggregator's prep_next (mastic.py:320-377) for a batch, from this
// aggregator's result planes and the other aggregator's prep shares as they
// came over the wire.  Lane r is report r: its own eval proof, joint-rand
// part, verifier share, joint-rand seed and status are words r of their
// planes (a wave reads 256 contiguous bytes per word), its peer row is
// peer + psz * r.  code[r]: k_decide's code for (share of aggregator 0, share
// of aggregator 1), or DECIDE_PEER_SKIPPED when the own status is nonzero or
// the peer does not offer the report (peer_ok, null: all offered); msg[r] (32
// bytes, with the weight check and joint randomness only): the prep message
// where k_decide writes it, else zero; accept[r]: code OK and the prep message
// equals the own joint-rand seed.
//
// The peer rows are a multiple of 8 bytes long (32 + [32] + elements of 8 or
// 16) and start 8-byte aligned.  LDS = false: every lane loads the words of
// its own row (a wave's load touches 64 rows).  LDS = true: each wave first
// copies its 64 rows, which are contiguous, with coalesced loads into its
// slice of LDS ([row][pitch], pitch odd: lane r then reads word j at bank
// (r * pitch + j) % 64, all different) and reads its row from there; rows of
// more than DECIDE_PEER_LDS_WORDS words do not fit a workgroup's 64 KiB.
constexpr int DECIDE_PEER_SKIPPED = 3;     // MASTIC_DECIDE_SKIPPED
constexpr int DECIDE_PEER_LDS_WORDS = 63;  // 256 rows x pitch 63 words x 4 bytes < 64 KiB
struct PeerOwn {  // this aggregator's result planes (stride S)
    const uint32_t* eval_proof;  // [8]
    const uint32_t* jr_part;     // [8]   weight check with joint randomness
    const uint32_t* verifier;    // [verifier_len * w32]   weight check
    const uint32_t* jr_seed;     // [8]   weight check with joint randomness
    const int32_t* status;
};
inline int decide_peer_pitch(int row_words) { return row_words | 1; }

template <class F, bool LDS>
__global__ __launch_bounds__(256) void k_decide_peer(McParams p, int n, int stride, int weight_check, int agg_id,
                                                     PeerOwn own, const uint8_t* peer, int ps_size,
                                                     const uint8_t* peer_ok, uint32_t* ver_scratch,
                                                     const PrefixState* pfx, uint8_t* msg_out, uint8_t* code_out,
                                                     uint8_t* accept_out) {
    typedef typename F::E E;
    extern __shared__ uint32_t peer_lds[];
    const int r = blockIdx.x * 256 + threadIdx.x;
    const int W = ps_size >> 2;
    const uint32_t* row = (const uint32_t*)(peer + (size_t)ps_size * r);  // dereferenced for r < n only
    if (LDS) {
        const int pitch = W | 1;
        const int lane = threadIdx.x & 63;
        const int r0 = r - lane;  // the wave's first report
        uint32_t* slice = peer_lds + (size_t)(threadIdx.x >> 6) * 64 * pitch;
        const int rows = n - r0 < 64 ? n - r0 : 64;  // <= 0: a wave past the batch
        const uint32_t* src = (const uint32_t*)(peer + (size_t)ps_size * r0);
        // word i of the wave's rows is (row, col) = (i / W, i % W): one divide per lane, then steps of 64 words
        const int drow = 64 / W, dcol = 64 - drow * W;
        int rr = lane / W, col = lane - rr * W;
        for (int i = lane; i < rows * W; i += 64) {
            slice[rr * pitch + col] = src[i];
            rr += drow;
            col += dcol;
            if (col >= W) {
                col -= W;
                rr++;
            }
        }
        __syncthreads();
        row = slice + lane * pitch;
    }
    if (r >= n) return;
    auto pw = [&](int j) { return row[j]; };  // word j of the peer's row
    const bool check_jr = weight_check && p.joint_rand_len > 0;
    uint32_t msg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint8_t st = DECIDE_PEER_SKIPPED;
    bool ok = false;
    if (own.status[r] == 0 && (!peer_ok || peer_ok[r] != 0)) {
        st = 1;
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (own.eval_proof[(size_t)j * stride + r] != pw(j)) st = 0;
        if (st && weight_check) {
            const int v0 = check_jr ? 16 : 8;  // the verifier's first word
            for (int e = 0; e < p.verifier_len; e++) {
                uint32_t wb[F::W32];
                for (int i = 0; i < F::W32; i++) wb[i] = pw(v0 + e * F::W32 + i);
                const E xa = pl_load<F>(own.verifier, e, stride, r), xb = F::from_words(wb);
                if (!F::valid(xa) || !F::valid(xb)) st = 2;
                pl_store<F>(ver_scratch, e, stride, r, F::add(xa, xb));
            }
            if (st == 1 && !flp_decide<F>(p, ver_scratch, stride, r)) st = 2;
            if (st == 1 && p.joint_rand_len > 0) {
                // aggregator 0's part first, whichever side this is
                KState s;
                int f;
                load_prefix(pfx, PFX_JR_SEED, s, f);
                f = sponge_absorb_words(s, f, 64, [&](int m) {
                    const bool mine = (m < 8) == (agg_id == 0);
                    return mine ? own.jr_part[(size_t)(m & 7) * stride + r] : pw(8 + (m & 7));
                });
                sponge_pad(s, f, 0x01);
#pragma unroll
                for (int j = 0; j < 8; j++) msg[j] = kword(s, j);
            }
        }
        ok = st == 1;
        if (check_jr) {
#pragma unroll
            for (int j = 0; j < 8; j++) ok = ok && msg[j] == own.jr_seed[(size_t)j * stride + r];
        }
    }
    if (check_jr) {
        uint4* m = (uint4*)(msg_out + (size_t)32 * r);  // 16-byte aligned (the host's staging layout)
        m[0] = make_uint4(msg[0], msg[1], msg[2], msg[3]);
        m[1] = make_uint4(msg[4], msg[5], msg[6], msg[7]);
    }
    code_out[r] = st;
    accept_out[r] = ok ? 1 : 0;
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
