// The level kernel: one tree level of Vidpf.eval for every report (k_eval_aes
// and k_eval_aes_wide, one body), with the previous level's node proofs on its
// proof waves and the frontier cache's recompute and fused proofs.
#pragma once
#include "aes.hpp"
#include "conv_stream.hpp"
#include "flp.hpp"
#include "node_proof.hpp"
#include "params.hpp"
#include "planes.hpp"

// ------------------------------------------------------------- eval level
// A tree level is evaluated by two kernels:
//   k_eval_aes    extend + correct + convert of both children of every parent
//                 (all the AES: 2 + 2 * (1 + ceil(VL*ENC/16)) blocks per
//                 parent), payload corrections, the parent payload difference
//                 and the truncated out shares;
//   k_node_proof  the children's node proofs (one Keccak-p each).
// The next seeds and control bits of all children go through a per-level
// plane buffer ("child seeds", 5 words per node) from the first to the second
// kernel and to the next level's k_eval_aes.  Splitting lets the LDS-bound AES
// run at 4 waves/SIMD and the VALU-only Keccak overlap it on another stream.
struct AesArgs {
    int level;
    int agg_id;
    int n_parents;       // parents at this level (1 = the root at level 0)
    int ppw;             // items per wave (an item is a parent, or one block range of one)
    // Small levels (few parents: the top of every tree) leave most waves of a
    // workgroup idle and each parent's ~2 + 2 nblk AES blocks a serial chain
    // of one wave.  There a parent is split into `split` items: item k
    // recomputes the parent's extend pair (2 blocks) and evaluates blocks
    // [k * split_blocks, (k + 1) * split_blocks) of both children's convert
    // streams (counter mode: the blocks are independent); item 0 also the
    // next seeds.  Never at a level that emits out shares (the truncation
    // accumulates across elements) or on a frontier-cache hit.
    int split;
    int split_blocks;
    const int32_t* parent_node;  // [n_parents] node index of each parent in level-1 (level >= 1)
    const int32_t* child_exp;    // [2 * n_parents] index into this level's frontier, -1 = leaf
    const int32_t* child_pfx;    // [2 * n_parents] index into the prefix list (level L), -1 = none
    const uint32_t* cs_in;       // child seeds of level-1: [node][5]
    uint32_t* cs_out;            // child seeds of this level: [node][5] (seed words, ctrl)
    const uint32_t* fr_w_in;     // payloads of level-1's expanded nodes [e][vl*w32]
    uint32_t* fr_w_out;
    uint32_t* payload;   // [n_parents * vl*w32]  w_p - w_L - w_R of the parents (BFS order)
    uint32_t* out;       // [n_prefixes * (1 + out_len) * w32] planes of the result buffer (row stride out_stride)
    int out_stride;
    int force_slow_blk;  // test hook: the Field64 fast path hands over to the exact stream at this block (-1 = never)
    // frontier cache (mastic_set_frontier_cache).  A cached node is 5 words: its convert seed (the
    // extend output after correction, the seed of convert) and its control bit.  Last level of a
    // prep_init: every child's node is written straight into the cache's spare slot (cache_out,
    // plane stride cache_stride).  Cache hit: the parents come from the cache (cs_in, stride
    // in_stride), and each parent's seed (block 0 of its convert stream) and payload (the rest of
    // the stream, corrected) are recomputed, the payload into wp_buf by parent ordinal.
    uint32_t* cache_out;
    int cache_stride;
    uint32_t* wp_buf;
    int recompute_wp;
    int in_stride;  // plane stride of cs_in (the cache's, on a hit; else the work buffer's)
    // Node formats (FC only; mastic_set_frontier_cache_nodes).  A slot holds seeds-format nodes (the
    // 5 words above) or payloads-format nodes: [next seed 4][ctrl][payload, VALUE_LEN * w32 words],
    // the next seed being block 0 of the node's convert stream and the payload as emit corrected it.
    // The slot a hit reads and the slot the call writes may differ in format, so the two switches
    // are independent (both live in the PAY instantiation, launched when either is > 5).
    // in_nw: words per node of cs_in (5: the work buffer's child seeds, or a seeds-format slot, then
    // recompute_wp = 1 on a hit; > 5: a payloads-format slot, whose parents need no recompute and
    // whose payload the children read from the slot, plane stride in_stride).
    // out_nw: words per node of cache_out (> 5: emit also stores both children's corrected elements
    // into their nodes and the header takes the next seeds).  That is safe because a launch that
    // writes the cache is a call's last level, which emits out shares and is therefore never split
    // into block-range items (every element of a node comes from the one item that owns the parent),
    // and because it is never cut into parent ranges (schedule.hpp plan_chunk segments a last level
    // only without the cache; the host offsets cache_out by a range's first parent as it does
    // cs_out), so cache_out is indexed by parent.
    int in_nw;
    int out_nw;
    // frontier-cache hit (FC only): the AES waves also compute THIS level's
    // node proofs right after each parent's payloads (no k_node_proof launch)
    int fuse_proofs;
    int cur_path_bytes;              // ceil((level + 1) / 8)
    const uint32_t* cur_child_path;  // [2 * n_parents][8]
    uint32_t* cur_onehot;            // this level's proof tiles
    // node proofs of the PREVIOUS level (vidpf.py:366-380, :321-323), computed
    // by the workgroup's EVAL_PROOF_WAVES proof waves beside the AES waves
    int pv_level;                   // level - 1
    int pv_nodes;                   // its node count (0 at level 0)
    int pv_npw;                     // nodes per proof wave
    int pv_path_bytes;              // ceil(level / 8)
    const uint32_t* pv_child_path;  // [pv_nodes][8]
    uint32_t* pv_onehot;            // [pv_nodes * 8] proofs of level - 1 (tiled, see AbsorbArgs)
    // The job is "the proofs of pv_nodes nodes of level pv_level, seeds at
    // pv_cs" (the work buffer's plane stride): level - 1's nodes in cs_in by
    // default; a segmented last level (mastic_set_last_level_segments) hands
    // range q >= 1 the nodes range q - 1 stored in cs_out, pv_level = level.
    const uint32_t* pv_cs;          // [pv_nodes][5] seeds and control bits of those nodes
    int oh_gstride;                 // words per report group of the proof buffers
    int bin_rstride;                // words between consecutive words of a report in them
    int pay_gstride;                // ... of the payload-difference buffers
    const PrefixState* np;          // node-proof prefix state
    int np_f;                       // its fill position
    int aes_waves;                  // waves [0, aes_waves) walk parents, the rest are proof waves
    int par_waves;                  // parents per workgroup = par_waves * ppw (aes_waves, or all 16 waves)
    int proof_prio;                 // s_setprio of the proof waves
    int aes_prio;                   // s_setprio of the AES waves
    int dbg_skip;                   // timing experiments only (results wrong): 1 = no proof work, 2 = no AES work
};

// Frontier-cache hit: the payload w_p of a parent (a node of the cached
// level), elements [e_lo, e_hi), recomputed from its convert seed cv and
// control bit t exactly as its own evaluation produced it (vidpf.py:352-364
// then the payload correction of eval_next, vidpf.py:317-319) and stored as
// element row0 + e of the planes `out`.  Fast path: consecutive blocks of the
// one stream in pairs (counters c, c+1 share their rounds 1-2 when c >> 8
// agrees), speculating that no candidate is rejected; if a lane of the wave
// meets a candidate >= p among the elements it uses, the exact next_vec
// stream takes over from that element.
template <class F>
MH_D void parent_payload(const AesPerm& TL, const RkLds& rkc, const uint32_t cv[4], uint32_t t, const uint32_t* cw,
                         int S, int r, int e_lo, int e_hi, uint32_t* out, int row0, int force_slow_blk,
                         uint32_t seed_out[4]) {
    typedef typename F::E E;
    constexpr int EPB = F::W32 == 2 ? 2 : 1;  // elements per block
    const int nblk = (e_hi + EPB - 1) / EPB;
    AesCtrGroup g;
    uint32_t g_hi = 0u;
    {
        // the parent's seed: block 0 of the same stream (next(16), vidpf.py:352-364), in the
        // counter group of the payload's first blocks
        const uint32_t* const sd[1] = {cv};
        const uint32_t hv[1] = {0u};
        AesCtrGroup* const gi[1] = {&g};
        ctr_group_init<1>(TL, rkc, sd, hv, gi);
        const AesCtrGroup* const gg[1] = {&g};
        const uint32_t c0v[1] = {0u};
        uint32_t* const ov[1] = {seed_out};
        ctr_blocks_n<1>(TL, rkc, gg, sd, c0v, ov);
    }
    int e_fast = e_lo;
    auto put = [&](int e, E x) {
        if (t) x = F::add(x, pl_load<F>(cw, e, S, r));
        pl_store<F>(out, row0 + e, S, r, x);
    };
    for (int b = e_lo / EPB; b < nblk; b += 2) {
        asm volatile("" ::: "memory");
        const uint32_t c0 = (uint32_t)(b + 1), c1 = c0 + 1;
        const bool two = b + 1 < nblk;
        // this pair's payload correction words, loaded before its AES (after
        // the previous pair's stores they would wait for those stores)
        E cwv[2 * EPB];
#pragma unroll
        for (int k = 0; k < 2 * EPB; k++) cwv[k] = pl_load<F>(cw, min(EPB * b + k, e_hi - 1), S, r);
        uint32_t o[2][4];
        if ((c0 & ~0xffu) == (c1 & ~0xffu)) {
            if ((c0 & ~0xffu) != g_hi) {
                const uint32_t* const sd[1] = {cv};
                const uint32_t hv[1] = {c0 & ~0xffu};
                AesCtrGroup* const gi[1] = {&g};
                ctr_group_init<1>(TL, rkc, sd, hv, gi);
                g_hi = c0 & ~0xffu;
            }
            const AesCtrGroup* const gg[2] = {&g, &g};
            const uint32_t* const sd2[2] = {cv, cv};
            const uint32_t cvv[2] = {c0, c1};
            uint32_t* const ov[2] = {o[0], o[1]};
            ctr_blocks_n<2>(TL, rkc, gg, sd2, cvv, ov);
        } else {  // the pair straddles a counter group (C5's long streams)
            const uint32_t* const sd2[2] = {cv, cv};
            const uint32_t cvv[2] = {c0, c1};
            uint32_t* const ov[2] = {o[0], o[1]};
            fixed_key_block_n<2>(TL, rkc, sd2, cvv, ov);
        }
        // candidates of these blocks that the parent uses: elements EPB*b ..
        bool sus = false;
        const int e0 = EPB * b;
#pragma unroll
        for (int k = 0; k < 2 * EPB; k++) {
            const int e = e0 + k;
            const uint32_t top = EPB == 2 ? o[k >> 1][2 * (k & 1) + 1] : o[k][3];
            if (e < e_hi && (k < EPB || two)) sus |= top == ~0u;
        }
        if (__builtin_expect(__any(sus), 0) || b == force_slow_blk || b + 1 == force_slow_blk) break;
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the loads above and the previous stores are done
#pragma unroll
        for (int k = 0; k < 2 * EPB; k++) {
            const int e = e0 + k;
            if (e < e_hi && (k < EPB || two)) {
                E x = F::from_words(&o[k / EPB][(k % EPB) * F::W32]);
                if (t) x = F::add(x, cwv[k]);
                pl_store<F>(out, row0 + e, S, r, x);
            }
        }
        e_fast = min(e_hi, e0 + 2 * EPB);
    }
    if (e_fast < e_hi) {
        // exact next_vec stream from the stream's start, emitting from e_fast on
        LevelStream<F> st;
        st.init(cv);
        for (int e = 0; e < e_hi; e++) {
            asm volatile("" ::: "memory");
            const E x = st.next(TL, rkc);
            if (e >= e_fast) put(e, x);
        }
    }
}

// One workgroup = 64 reports (one per lane) x 16 waves: 8 AES waves walk
// this level's parents and 8 proof waves first compute the node proofs of the
// previous level's children (a Keccak-p per node, VALU only), then join the
// AES waves; parents are claimed in runs through an LDS counter.  LDS-bound
// AES and VALU-bound Keccak share every CU inside one launch instead of two
// kernels competing for CU slots.  LDS: the v_perm-addressed T0/T2 table (64 KiB,
// aes.hpp AesPerm) and the 64 reports' two AES key schedules (22 KiB, one
// ds_read_b128 per round) are shared by all 16 waves: 86 KiB per workgroup,
// one workgroup = 4 waves per SIMD per CU.
#define EVAL_WAVES 16
#define EVAL_PROOF_WAVES 8  // default split (schedule.hpp SchedKnobs::proof_waves); measured best of 2..12
// VGPR cap of the level kernel: 4 waves x 96 per SIMD leave 128 of the 512
// for one binder-sponge wave, so the two kernels can share a CU instead of
// taking turns.  The one-lane sponge kernel (k_absorb: 122 VGPRs, allocated
// 128) needs all of that; the 2-lane one (k_absorb_pair: 93, allocated 96)
// leaves 32 more, which k_eval_aes_wide below takes.
// (expressed as a minimum occupancy: 5 waves/SIMD <=> at most 96 VGPRs)
#define EVAL_MIN_WAVES 5
// The frontier-cache instantiation (FC: a cache hit's one level, a cache-on
// call's last level) runs with no binder-sponge waves beside it on a hit, so
// it may take all 128 VGPRs of its 4 waves per SIMD (the LDS-resident tables
// allow one workgroup per CU): no spills of the recompute / fused-proof state.
#define EVAL_FC_MIN_WAVES 4
#define EVAL_VGPR_ATTR __attribute__((amdgpu_waves_per_eu(FC ? EVAL_FC_MIN_WAVES : EVAL_MIN_WAVES)))
// The plain variants beside 2-lane sponges (WIDE, k_eval_aes_wide): 104 VGPRs,
// 4 x 104 + 96 = 512.  No occupancy gives 104, so the cap is amdgpu_num_vgpr,
// which takes a literal (hence a kernel of its own, not a template argument)
// and which on gfx90a and later, with their unified VGPR / AGPR file, counts
// HALF of the budget: the compiler doubles it, drops a value above the
// occupancy's own limit (num_vgpr(104) -> 208 > 128: ignored, 117 allocated)
// and, since the kernel uses no AGPRs, hands all of it to the VGPRs.  52 -> 104.
#define EVAL_WIDE_ATTR __attribute__((amdgpu_waves_per_eu(4), amdgpu_num_vgpr(52)))
// workgroup sync words after the key schedules: [0] parent-run counter, [1]
// node-proof counter (frontier-cache hits), [8, 40) "child seeds stored" bitmap
// of the workgroup's parents (<= 16 waves x 64 parents per wave)
#define EVAL_SYNC_WORDS 40
#define EVAL_LDS_BYTES (AES_PERM_LDS_WORDS * 4 + 2 * 64 * 11 * 16 + 4 * EVAL_SYNC_WORDS)
// GEN: the general level (the root level, which writes the root sum instead
// of parent payload differences, and the last level, which emits the
// truncated out shares, with their field multiplications for grouped
// truncations); the interior levels (all others: 30 of C2's 32, 31 of C5's)
// run an instantiation without that code, whose block loop then needs fewer
// scalar registers (no spills of uniform flags into VGPR lanes).  FC: the
// frontier cache's convert-seed staging, parent-payload recompute and fused
// proofs are compiled in (only at a call's last level, so always with GEN);
// the plain instantiation carries none of it (the uniform branches cost 2.5 %
// at C2).
// SPLIT: a small level's parents split into block-range items (AesArgs::split;
// never with FC); a separate instantiation so the other levels' kernels carry
// none of its bookkeeping (in the plain kernel it quadrupled the SGPR spills).
// WIDE: the 104-VGPR budget above; the proof waves run the fused-theta
// permutation (never with FC).  PAY (only with FC): the payloads node format
// of the frontier cache (AesArgs::in_nw / out_nw) is compiled in, for a launch
// whose input or output slot has it; the seeds-only FC kernel carries none of
// it (in one kernel the two formats cost it 80 more spilled SGPRs).  One body,
// two kernels (k_eval_aes and k_eval_aes_wide below) that differ in their
// register attributes only.
template <class F, bool GEN, bool FC, bool SPLIT, bool WIDE, bool PAY = false>
MH_D void eval_aes_body(const McParams& p, const Planes& pl, const AesArgs& a) {
    typedef typename F::E E;
    // dynamic LDS (EVAL_LDS_BYTES): with a static size the compiler derives
    // the occupancy from it and ignores the VGPR cap of EVAL_VGPR_ATTR
    extern __shared__ uint4 eval_lds[];
    uint32_t* T = (uint32_t*)eval_lds;
    uint4* RKE = eval_lds + AES_PERM_LDS_WORDS / 4;
    uint4* RKC = RKE + 64 * 11;
    uint32_t* next_parent = (uint32_t*)(RKC + 64 * 11);  // the workgroup's parent-run counter
    uint32_t* next_proof = next_parent + 1;               // fused proofs: next node (workgroup ordinal)
    uint32_t* parent_done = next_parent + 8;              // fused proofs: parents whose child seeds are stored
    // the T-table lookups use the v_perm result as the absolute LDS address
    // (aes.hpp lds_read_asm): the table must start at LDS address 0
    if ((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint4*)eval_lds != 0u) __builtin_trap();

    const int S = pl.stride;
    const int S_in = FC ? a.in_stride : S;  // cs_in / fr_w_in
    const int NW_in = (FC && PAY) ? a.in_nw : 5;     // words per node of cs_in (AesArgs::in_nw)
    const int NW_out = (FC && PAY) ? a.out_nw : 5;  // ... of cache_out (AesArgs::out_nw)
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = blockIdx.x * 64 + lane;
    const uint32_t lb = (uint32_t)r * 4u;
    {
        // the two key schedules' 44 words per report: every wave's loads issued
        // first (one HBM round trip per workgroup, not three), the table filled
        // while they are in flight, then the words stored
        uint32_t* ke = (uint32_t*)RKE;
        uint32_t* kc = (uint32_t*)RKC;
        constexpr int KR = (44 + EVAL_WAVES - 1) / EVAL_WAVES;
        uint32_t xe[KR], xc[KR];
#pragma unroll
        for (int j = 0; j < KR; j++) {
            const int i = wave + j * EVAL_WAVES;
            if (i < 44) {
                xe[j] = pld(pl.rk_ext + (size_t)i * S, lb);
                xc[j] = pld(pl.rk_conv + (size_t)i * S, lb);
            }
        }
        aes_perm_fill(T, threadIdx.x, 64 * EVAL_WAVES);
#pragma unroll
        for (int j = 0; j < KR; j++) {
            const int i = wave + j * EVAL_WAVES;
            if (i < 44) {
                ke[lane * 44 + i] = aes_perm_key_word(i, xe[j]);
                kc[lane * 44 + i] = aes_perm_key_word(i, xc[j]);
            }
        }
    }
    // words [8, 40): the fused-proof bitmap (FC) or, with split parents, each
    // parent's first element whose block a lane flagged (split_first below)
    if (threadIdx.x < EVAL_SYNC_WORDS) next_parent[threadIdx.x] = (SPLIT && threadIdx.x >= 8) ? ~0u : 0u;
    __syncthreads();
    const int aes_waves = a.aes_waves;
    // Proof waves: node proofs of level - 1 (children seeds from pv_cs), then
    // they help with the parents; with no proofs to do (level 0, a frontier-
    // cache hit) they walk parents from the start.  No wave returns early: a
    // cache hit's fused proofs below take nodes from every wave (and the A/B
    // barrier schedule ends with a workgroup barrier).
    if (wave >= aes_waves && a.pv_nodes > 0 && !(a.dbg_skip & 1)) {
        if (a.proof_prio == 1) __builtin_amdgcn_s_setprio(1);
        if (a.proof_prio == 2) __builtin_amdgcn_s_setprio(2);
        const int nbeg = (blockIdx.y * (EVAL_WAVES - aes_waves) + (wave - aes_waves)) * a.pv_npw;
        const int nend = min(nbeg + a.pv_npw, a.pv_nodes);
        const int pl_ = a.pv_level;
        uint32_t* ohg = a.pv_onehot + (size_t)blockIdx.x * a.oh_gstride;  // tile group of these 64 reports
        const uint32_t lt = (uint32_t)lane * 4u;
        uint32_t pcw[8];
        if constexpr (!WIDE) {
#pragma unroll
            for (int j = 0; j < 8; j++) pcw[j] = pld(pl.cw_proof + ((size_t)pl_ * 8 + j) * S, lb);
        }
        for (int node = nbeg; node < nend; node++) {
            uint32_t sd[4];
#pragma unroll
            for (int i = 0; i < 4; i++) sd[i] = pld(a.pv_cs + ((size_t)node * 5 + i) * S, lb);
            if constexpr (WIDE) {
                // fused theta keeps the parities live through rho: the control
                // bit and the proof correction word (the same 8 cached rows for
                // every node) are loaded after the permutation instead of being
                // held in 9 registers across it, which spilled them
                uint32_t w8[8];
                node_proof_one<true>(a.np, a.np_f, p.bits, pl_, a.pv_path_bytes, sd, a.pv_child_path + node * 8, 0u, pcw,
                                     [&](int j, uint32_t w) { w8[j] = w; });
                const uint32_t t = pld(a.pv_cs + ((size_t)node * 5 + 4) * S, lb);
#pragma unroll
                for (int j = 0; j < 8; j++) pcw[j] = pld(pl.cw_proof + ((size_t)pl_ * 8 + j) * S, lb);
#pragma unroll
                for (int j = 0; j < 8; j++)
                    pst(ohg + ((size_t)node * 8 + j) * a.bin_rstride, lt, w8[j] ^ (t ? pcw[j] : 0u));
            } else {
                const uint32_t t = pld(a.pv_cs + ((size_t)node * 5 + 4) * S, lb);
                node_proof_one<FC>(a.np, a.np_f, p.bits, pl_, a.pv_path_bytes, sd, a.pv_child_path + node * 8, t, pcw,
                                   [&](int j, uint32_t w) { pst(ohg + ((size_t)node * 8 + j) * a.bin_rstride, lt, w); });
            }
        }
        if (a.proof_prio) __builtin_amdgcn_s_setprio(0);
        // then help with this workgroup's parents (below)
    }
    // Parents of this workgroup: [wp0, wp1), claimed in runs of `run` by
    // every wave through an LDS counter: the proof waves join once their
    // proofs are done, so no wave idles while another still has parents.
    const int wp0 = blockIdx.y * a.par_waves * a.ppw;
    const int wp1 = min(wp0 + a.par_waves * a.ppw, SPLIT ? a.n_parents * a.split : a.n_parents);  // items
    // Frontier-cache hit (FC, fuse_proofs == 1): THIS level's node proofs
    // (vidpf.py:366-380, :321-323) of the workgroup's children, overlapped with
    // its parents' AES.  The AES waves [0, aes_waves) walk the parents; a wave
    // that has stored a parent's child seeds and control bits marks the parent
    // in parent_done (release, workgroup scope).  The proof waves take the
    // children in order through next_proof and wait (acquire) for their
    // parent's mark; AES waves that run out of parents join them.  So some
    // waves run the LDS-bound AES while others run the VALU-bound Keccak: with
    // one workgroup per CU (150 KiB of LDS) the two pipes otherwise take turns
    // (AES of every parent, barrier, proofs).  The host sizes the split by the
    // two kinds' work per parent.  fuse_proofs == 3 (A/B only): the barrier
    // schedule.  (Taking ready nodes inside the parent loop instead keeps the
    // loop's state live across the Keccak: 74 spilled VGPRs, 769 scratch loads.)
    const int pn_beg = 2 * wp0, pn_end = 2 * wp1;  // this workgroup's child nodes
    const bool fuse_ovl = FC && a.fuse_proofs == 1;
    auto parent_marked = [&](int q) -> bool {
        const uint32_t w = __hip_atomic_load(parent_done + (q >> 5), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
        return (__builtin_amdgcn_readfirstlane(w) >> (q & 31)) & 1u;
    };
    auto claim_node = [&]() -> int {
        uint32_t o = 0;
        if (lane == 0) o = atomicAdd(next_proof, 1u);
        return pn_beg + (int)__builtin_amdgcn_readfirstlane(o);
    };
    auto node_proof_at = [&](int node) {
        if (a.dbg_skip & 2) return;  // timing knob: no parents were evaluated
        if (fuse_ovl)
            while (!parent_marked((node - pn_beg) >> 1)) __builtin_amdgcn_s_sleep(2);
        const int l = a.level;
        uint32_t* ohg = a.cur_onehot + (size_t)blockIdx.x * a.oh_gstride;
        const uint32_t lt = (uint32_t)lane * 4u;
        uint32_t pcw[8];
#pragma unroll
        for (int j = 0; j < 8; j++) pcw[j] = pld(pl.cw_proof + ((size_t)l * 8 + j) * S, lb);
        uint32_t sd[4];
#pragma unroll
        for (int i = 0; i < 4; i++) sd[i] = pld(a.cs_out + ((size_t)node * 5 + i) * S, lb);
        const uint32_t t = pld(a.cs_out + ((size_t)node * 5 + 4) * S, lb);
        node_proof_one<FC>(a.np, a.np_f, p.bits, l, a.cur_path_bytes, sd, a.cur_child_path + node * 8, t, pcw,
                       [&](int j, uint32_t w) { pst(ohg + ((size_t)node * 8 + j) * a.bin_rstride, lt, w); });
    };
    if (a.dbg_skip & 2) goto aes_done;
    if (fuse_ovl && wave >= aes_waves) goto aes_done;  // proof waves of a hit
    {
        if (a.aes_prio == 1) __builtin_amdgcn_s_setprio(1);
        if (a.aes_prio == 2) __builtin_amdgcn_s_setprio(2);
        const int l = a.level;
        const int vl = p.value_len;
        const int wl = vl * F::W32;
        const AesPerm TL{T, 4u * (uint32_t)(lane & 31), 128u + 4u * (uint32_t)(lane & 31)};
        const RkLds rke{RKE + lane * 11};
        const RkLds rkc{RKC + lane * 11};

        uint32_t scw[4];
#pragma unroll
        for (int i = 0; i < 4; i++) scw[i] = pld(pl.cw_seed + ((size_t)l * 4 + i) * S, lb);
        const uint32_t ccw = pld(pl.cw_ctrl + (size_t)l * S, lb);
        const uint32_t* wcw = pl.cw_w + (size_t)l * wl * S;

        // Split parents (AesArgs::split, small levels; never FC): pass 0 runs the
        // items.  A block range that meets a candidate >= p (or the test hook's
        // block) does not run the exact stream itself -- a rejection shifts every
        // later element, including other items' ranges, which may already be
        // stored -- but records its first element in split_first; after a
        // workgroup barrier, pass 1 re-evaluates each flagged parent with the
        // exact next_vec stream from that element to the end, overwriting.
        // (Both children of a parent and all its items are in this workgroup: the
        // host gives a split level one workgroup per report group.)
        const int K = SPLIT ? a.split : 1;
        constexpr int npass = SPLIT ? 2 : 1;
        const int pb = wp0 / K, pe = (wp1 + K - 1) / K;  // parents of this workgroup
        uint32_t* const split_first = parent_done;
        for (int pass = 0; pass < npass; pass++) {
            if (pass == 1) __syncthreads();  // every item of pass 0 is stored (workgroup fence + barrier)
            const int run = pass ? 1 : max(1, a.ppw / 8);
            const int pend = pass ? pe : wp1;
            auto claim = [&]() -> int {
                uint32_t o = 0;
                if (pass == 0) {
                    if (lane == 0) o = atomicAdd(next_parent, (uint32_t)run);
                    return wp0 + (int)__builtin_amdgcn_readfirstlane(o);
                }
                for (;;) {  // pass 1: the next flagged parent
                    if (lane == 0) o = atomicAdd(next_parent + 1, 1u);
                    const int q = pb + (int)__builtin_amdgcn_readfirstlane(o);
                    if (q >= pe || __builtin_amdgcn_readfirstlane(split_first[q - pb]) < (uint32_t)p.value_len) return q;
                }
            };
            int rbeg = claim();
            if (rbeg >= pend) continue;
            int rend = min(rbeg + run, pend);
            // Parent seed / control bit, software-pipelined one parent ahead so the
            // HBM latency of the child-seed planes hides under the previous parent's
            // AES work.
            auto load_parent = [&](int item, uint32_t* ps, uint32_t& pctrl) {
                const int pi = (K > 1 && !pass) ? item / K : item;
                if (l == 0) {
#pragma unroll
                    for (int i = 0; i < 4; i++) ps[i] = pld(pl.key + (size_t)i * S, lb);
                    pctrl = a.agg_id;
                } else {
                    const int pn = a.parent_node[pi];
                    const size_t n0 = (size_t)pn * NW_in;  // either node format starts with a seed and the control bit
#pragma unroll
                    for (int i = 0; i < 4; i++) ps[i] = pld(a.cs_in + (n0 + i) * S_in, lb);
                    pctrl = pld(a.cs_in + (n0 + 4) * S_in, lb);
                }
            };
            uint32_t nps[4], npctrl;
            load_parent(rbeg, nps, npctrl);
            for (int item = rbeg; item >= 0;) {
                const int pi = (K > 1 && !pass) ? item / K : item;  // parent
                const int kp = pass ? 1 : (K > 1 ? item - pi * K : 0);  // its block range (pass 1: no next seeds)
                constexpr int EPB_ = F::W32 == 2 ? 2 : 1;  // elements per block
                const int e_lo = pass ? (int)__builtin_amdgcn_readfirstlane(split_first[pi - pb]) : kp * a.split_blocks * EPB_;
                const int e_hi = (K > 1 && !pass) ? min(vl, e_lo + a.split_blocks * EPB_) : vl;
                bool deferred = false;  // pass 0 of a split parent met a suspicious block: pass 1 redoes it
                // The key schedules are re-read from LDS (one ds_read_b128 per round):
                // without the barrier the compiler hoists all 22 reads out of the loop
                // and pins 88 VGPRs.
                asm volatile("" ::: "memory");
                uint32_t ps[4] = {nps[0], nps[1], nps[2], nps[3]};
                const uint32_t pctrl = npctrl;
                // next item: the rest of this run, else a new run
                int nxt = item + 1;
                if (nxt == rend) {
                    rbeg = claim();
                    rend = min(rbeg + run, pend);
                    nxt = rbeg < pend ? rbeg : -1;
                }
                if (nxt >= 0) load_parent(nxt, nps, npctrl);
                if constexpr (FC) {
                    if (a.recompute_wp) {
                        // frontier-cache hit: ps holds this parent's cached convert seed; its payload
                        // and its seed (into ps) from the convert stream
                        const uint32_t pcv[4] = {ps[0], ps[1], ps[2], ps[3]};
                        parent_payload<F>(TL, rkc, pcv, pctrl, pl.cw_w + (size_t)(l - 1) * wl * S, S, r, e_lo, e_hi, a.wp_buf,
                                          pi * vl, a.force_slow_blk, ps);
                        // the children's loop below reads these elements back (same lanes)
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    }
                }
                // extend: block 0 -> left child, block 1 -> right child (one paired
                // AES call), correct, then both children's convert seed blocks.
                uint32_t cs0[4], cs1[4], ns0[4], ns1[4];
                {
                    // both extend blocks share the parent seed (aes.hpp counter groups:
                    // rounds 1-2 shared by the blocks of one seed in the extend pair,
                    // the convert seeds and the payload fast path)
                    AesCtrGroup gp;
                    const uint32_t* const sd[1] = {ps};
                    const uint32_t ch[1] = {0u};
                    AesCtrGroup* const gi[1] = {&gp};
                    ctr_group_init<1>(TL, rke, sd, ch, gi);
                    const AesCtrGroup* const gg[2] = {&gp, &gp};
                    const uint32_t* const sd2[2] = {ps, ps};
                    const uint32_t cv[2] = {0u, 1u};
                    uint32_t* const ov[2] = {cs0, cs1};
                    ctr_blocks_n<2>(TL, rke, gg, sd2, cv, ov);
                }
                uint32_t tc0 = cs0[0] & 1u, tc1 = cs1[0] & 1u;
                cs0[0] &= ~1u;
                cs1[0] &= ~1u;
                if (pctrl) {
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        cs0[i] ^= scw[i];
                        cs1[i] ^= scw[i];
                    }
                    tc0 ^= ccw & 1u;
                    tc1 ^= (ccw >> 1) & 1u;
                }
                // each child's convert stream (next seed: counter 0, payload blocks:
                // counters 1, 2, ...) is one counter group per 256 counters
                AesCtrGroup g0, g1;
                uint32_t g_hi = 0;  // counter bits above 7 of the groups (uniform)
                const uint32_t* const csd[2] = {cs0, cs1};
                auto init_groups = [&](uint32_t hi) {
                    const uint32_t ch2[2] = {hi, hi};
                    AesCtrGroup* const gi[2] = {&g0, &g1};
                    ctr_group_init<2>(TL, rkc, csd, ch2, gi);
                    g_hi = hi;
                };
                const AesCtrGroup* const gg[2] = {&g0, &g1};
                init_groups(0u);
                if (kp == 0) {
                    const uint32_t cv[2] = {0u, 0u};
                    uint32_t* const ov[2] = {ns0, ns1};
                    ctr_blocks_n<2>(TL, rkc, gg, csd, cv, ov);
                }
                if constexpr (FC) {
                    if (a.cache_out) {
                        // the last level's children as frontier-cache nodes: convert seed (payloads
                        // format: next seed; emit below adds the payload), control bit
                        const int CS = a.cache_stride;
                        const bool pay = NW_out > 5;
                        const size_t n0 = (size_t)(2 * pi) * NW_out, n1 = n0 + NW_out;
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            pst(a.cache_out + (n0 + i) * CS, lb, pay ? ns0[i] : cs0[i]);
                            pst(a.cache_out + (n1 + i) * CS, lb, pay ? ns1[i] : cs1[i]);
                        }
                        pst(a.cache_out + (n0 + 4) * CS, lb, tc0);
                        pst(a.cache_out + (n1 + 4) * CS, lb, tc1);
                    }
                }
                if (kp == 0) {
                    const size_t n0 = (size_t)(2 * pi) * 5, n1 = n0 + 5;
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        pst(a.cs_out + (n0 + i) * S, lb, ns0[i]);
                        pst(a.cs_out + (n1 + i) * S, lb, ns1[i]);
                    }
                    pst(a.cs_out + (n0 + 4) * S, lb, tc0);
                    pst(a.cs_out + (n1 + 4) * S, lb, tc1);
                }
                const int ce0 = a.child_exp[2 * pi], ce1 = a.child_exp[2 * pi + 1];
                const int pf0 = GEN ? a.child_pfx[2 * pi] : -1, pf1 = GEN ? a.child_pfx[2 * pi + 1] : -1;
                const int row = 1 + p.output_len;
                E acc0 = F::zero(), acc1 = F::zero(), coef = F::from_u64(1);
                // Element e of both children: payload correction, frontier payloads,
                // the parent's payload difference (or the root sum), out shares.
                uint32_t* const payg = a.payload + (size_t)blockIdx.x * a.pay_gstride;  // tiled group
                constexpr bool x_fr = true, x_diff = true;
                // payloads-format cache nodes of the two children (FC, AesArgs::out_nw > 5): their payload planes
                uint32_t* cpay0 = nullptr;
                uint32_t* cpay1 = nullptr;
                if constexpr (FC && PAY) {
                    if (a.cache_out && NW_out > 5) {
                        cpay0 = a.cache_out + ((size_t)(2 * pi) * NW_out + 5) * a.cache_stride;
                        cpay1 = cpay0 + (size_t)NW_out * a.cache_stride;
                    }
                }
                auto emit = [&](int e, E x0, E x1, E cw, E wp) {
                    if (tc0) x0 = F::add(x0, cw);
                    if (tc1) x1 = F::add(x1, cw);
                    if constexpr (FC && PAY) {
                        // the same coalesced plane stores as fr_w_out's (the last level makes none of those)
                        if (cpay0) {
                            pl_store<F>(cpay0, e, a.cache_stride, r, x0);
                            pl_store<F>(cpay1, e, a.cache_stride, r, x1);
                        }
                    }
                    if (x_fr && ce0 >= 0) pl_store<F>(a.fr_w_out, ce0 * vl + e, S, r, x0);
                    if (x_fr && ce1 >= 0) pl_store<F>(a.fr_w_out, ce1 * vl + e, S, r, x1);
                    if (GEN && l == 0) {
                        pl_store<F>(pl.rootsum, e, S, r, F::add(x0, x1));
                    } else if (!x_diff) {
                        if (F::is_zero(F::sub(F::sub(wp, x0), x1))) a.out[0] = 0u;  // keep the work, drop the store
                    } else {
                        // tiled (AbsorbArgs): word m of this group's 64 reports = one row
                        pl_store_rows<F>(payg, pi * vl + e, a.bin_rstride, (uint32_t)lane * 4u, F::sub(F::sub(wp, x0), x1));
                    }
                    if (GEN && (pf0 >= 0 || pf1 >= 0)) {
                        // truncated out share, negated for the helper (vidpf.py:259, mastic.py:311-314)
                        if (e == 0) {
                            if (pf0 >= 0) pl_store<F>(a.out, pf0 * row, a.out_stride, r, a.agg_id ? F::neg(x0) : x0);
                            if (pf1 >= 0) pl_store<F>(a.out, pf1 * row, a.out_stride, r, a.agg_id ? F::neg(x1) : x1);
                        } else if (e - 1 < p.tlimit) {
                            const int m = e - 1;
                            const int g = m % p.tgroup;
                            if (p.tgroup == 1) {
                                acc0 = x0;
                                acc1 = x1;
                            } else {
                                coef = g == 0 ? F::from_u64(1) : F::add(coef, coef);
                                acc0 = F::add(g == 0 ? F::zero() : acc0, F::mul(coef, x0));
                                acc1 = F::add(g == 0 ? F::zero() : acc1, F::mul(coef, x1));
                            }
                            if (g == p.tgroup - 1) {
                                const int o = 1 + m / p.tgroup;
                                if (pf0 >= 0) pl_store<F>(a.out, pf0 * row + o, a.out_stride, r, a.agg_id ? F::neg(acc0) : acc0);
                                if (pf1 >= 0) pl_store<F>(a.out, pf1 * row + o, a.out_stride, r, a.agg_id ? F::neg(acc1) : acc1);
                            }
                        }
                    }
                };
                auto load_cw = [&](int e) { return pl_load<F>(wcw, e, S, r); };
                const uint32_t* wpb = a.fr_w_in;
                int wp_S = S, wp_e0 = pi * vl;  // plane stride and first element of this parent's payload in wpb
                if constexpr (FC) {
                    wpb = a.recompute_wp ? a.wp_buf : a.fr_w_in;
                    if (PAY && NW_in > 5) {
                        // a hit on a payloads-format slot: the parent's payload straight from its node
                        wpb = a.cs_in + ((size_t)a.parent_node[pi] * NW_in + 5) * S_in;
                        wp_S = S_in;
                        wp_e0 = 0;
                    }
                }
                // level 0: the root's "parent payload" planes are zeroed by the host
                // (no branch, no zero-initialised registers in the block loop)
                auto load_wp = [&](int e) { return pl_load<F>(wpb, wp_e0 + e, wp_S, r); };
                int e_fast = e_lo;  // elements completed by the fast path
                // the same before the block loop: the next parent's prefetched seed
                // and this parent's child-seed stores are long done; without it the
                // waitcnt pass keeps a vmcnt wait in the loop header (every block)
                __builtin_amdgcn_s_waitcnt(0x0F70);
                if constexpr (FC) {
                    if (fuse_ovl && lane == 0) {
                        // the child seeds / control bits above are stored: their proofs may start
                        const int q = pi - wp0;
                        __hip_atomic_fetch_or(parent_done + (q >> 5), 1u << (q & 31), __ATOMIC_RELEASE,
                                              __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                {
                    // Fast path: block b (counter b + 1) of each child's convert stream
                    // holds Field64 candidates 2b and 2b + 1, or Field128 candidate b
                    // (vdaf_poc next_vec after next(16)).  Speculate that no candidate
                    // is rejected: one paired AES call per block index, straight-line.
                    // A candidate >= p has its top word 0xffffffff (probability 2^-32
                    // for Field64, ~2^-59 for Field128); if any lane of the wave sees
                    // such a word among the elements it is about to use, the exact
                    // stream below redoes this parent from that element on (elements
                    // before it are unaffected by the rejection).
                    constexpr int EPB = F::W32 == 2 ? 2 : 1;  // elements per block
                    const int nblk = pass ? 0 : (e_hi + EPB - 1) / EPB;  // pass 1: the exact stream only
                    for (int b = e_lo / EPB; b < nblk; b++) {
                        asm volatile("" ::: "memory");
                        const int e = EPB * b;
                        const bool two = EPB == 2 && e + 1 < e_hi;
                        const int e1 = two ? e + 1 : e;  // uniform clamp
                        const E cwa = load_cw(e), wpa = load_wp(e);
                        E cwb = cwa, wpb = wpa;
                        if constexpr (EPB == 2) {
                            cwb = load_cw(e1);
                            wpb = load_wp(e1);
                        }
                        uint32_t o0[4], o1[4];
                        {
                            const uint32_t c = (uint32_t)(b + 1);
                            if ((c & ~0xffu) != g_hi) init_groups(c & ~0xffu);
                            const uint32_t cv[2] = {c, c};
                            uint32_t* const ov[2] = {o0, o1};
                            ctr_blocks_n<2>(TL, rkc, gg, csd, cv, ov);
                        }
                        bool sus;
                        if constexpr (EPB == 2)
                            sus = (o0[1] == ~0u) | (o1[1] == ~0u) | (two & ((o0[3] == ~0u) | (o1[3] == ~0u)));
                        else
                            sus = (o0[3] == ~0u) | (o1[3] == ~0u);
                        if (__builtin_expect(__any(sus), 0) || b == a.force_slow_blk) {
                            if (K > 1) {
                                if (lane == 0) atomicMin(split_first + (pi - pb), (uint32_t)e);
                                deferred = true;
                            }
                            break;
                        }
                        // All of this block's loads (issued before its AES) and the
                        // previous block's stores have long completed: say so with one
                        // explicit wait.  Otherwise the waitcnt pass, which loses track
                        // of the conditionally issued loads, waits for vmcnt(2..3)
                        // between the stores below, i.e. for the stores themselves to
                        // be acknowledged, several times per block.
                        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt / lgkmcnt untouched
                        emit(e, F::from_words(o0), F::from_words(o1), cwa, wpa);
                        if constexpr (EPB == 2) {
                            if (two) emit(e + 1, F::from_words(o0 + 2), F::from_words(o1 + 2), cwb, wpb);
                        }
                        e_fast = e + 1 + (two ? 1 : 0);
                    }
                }
                if (e_fast < e_hi && !deferred) {
                    // exact next_vec streams (rejection sampling), element by element
                    // from the stream's start (a rejection shifts every later element)
                    // up to e_hi, emitting from e_fast on; elements before it were
                    // emitted by the fast path
                    LevelStream<F> st0, st1;
                    st0.init(cs0);
                    st1.init(cs1);
                    constexpr int G = LevelStream<F>::GROUP;
                    for (int e0 = 0; e0 < e_hi; e0 += G) {
                        asm volatile("" ::: "memory");
                        st0.refill(st1, TL, rkc);
#pragma unroll
                        for (int i = 0; i < G; i++) {
                            const int e = e0 + i;
                            if (e >= e_hi) break;
                            const E x0 = st0.next(TL, rkc);
                            const E x1 = st1.next(TL, rkc);
                            if (e >= e_fast) emit(e, x0, x1, load_cw(e), load_wp(e));
                        }
                    }
                }
                item = nxt;
            }
        }  // pass
    }
aes_done:
    if constexpr (FC) {
        if (a.fuse_proofs) {
            // the nodes nobody has taken yet (overlapped: their parents may still
            // be running; A/B barrier schedule: after every parent is done)
            if (!fuse_ovl) __syncthreads();
#pragma unroll 1
            for (int node = claim_node(); node < pn_end; node = claim_node()) node_proof_at(node);
        }
    }
}

template <class F, bool GEN, bool FC, bool SPLIT = false, bool PAY = false>
__global__ __launch_bounds__(64 * EVAL_WAVES) EVAL_VGPR_ATTR
void k_eval_aes(McParams p, Planes pl, AesArgs a) {
    eval_aes_body<F, GEN, FC, SPLIT, false, PAY>(p, pl, a);
}
template <class F, bool GEN, bool SPLIT = false>
__global__ __launch_bounds__(64 * EVAL_WAVES) EVAL_WIDE_ATTR
void k_eval_aes_wide(McParams p, Planes pl, AesArgs a) {
    eval_aes_body<F, GEN, false, SPLIT, true>(p, pl, a);
}
