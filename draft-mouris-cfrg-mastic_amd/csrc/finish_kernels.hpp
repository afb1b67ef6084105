// After the last level: the checks and the eval proof (k_finalize), then the
// FLP's randomness and query (k_flp_rand, k_flp_query).
#pragma once
#include "flp.hpp"
#include "keccak.hpp"
#include "params.hpp"
#include "planes.hpp"

// ------------------------------------------------------------- finalize
// payload_check, onehot_check, counter_check, eval_proof (mastic.py:277-306).
struct FinalArgs {
    int agg_id;
    int f_onehot;
    int f_payload;
};

template <class F>
__global__ __launch_bounds__(256) void k_finalize(McParams p, Planes pl, FinalArgs a, const PrefixState* pfx) {
    __shared__ uint32_t V[24 * 256];
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= pl.stride) return;
    const int S = pl.stride;
    uint32_t oh[8], pc[8];
    {
        KState s;
#pragma unroll
        for (int i = 0; i < 25; i++) s.a[i] = u32x2{pl.sp_onehot[(2 * i) * S + r], pl.sp_onehot[(2 * i + 1) * S + r]};
        sponge_pad(s, a.f_onehot, 0x01);
#pragma unroll
        for (int j = 0; j < 8; j++) oh[j] = kword(s, j);
#pragma unroll
        for (int i = 0; i < 25; i++) s.a[i] = u32x2{pl.sp_payload[(2 * i) * S + r], pl.sp_payload[(2 * i + 1) * S + r]};
        sponge_pad(s, a.f_payload, 0x01);
#pragma unroll
        for (int j = 0; j < 8; j++) pc[j] = kword(s, j);
    }
    typename F::E cnt = F::add(pl_load<F>(pl.rootsum, 0, S, r), F::from_u64((uint64_t)a.agg_id));
    // body = onehot_check || counter_check || payload_check
    const int t = threadIdx.x;
    for (int j = 0; j < 8; j++) V[j * 256 + t] = oh[j];
    for (int j = 0; j < F::W32; j++) V[(8 + j) * 256 + t] = F::word(cnt, j);
    for (int j = 0; j < 8; j++) V[(8 + F::W32 + j) * 256 + t] = pc[j];
    KState s;
    int f;
    load_prefix(pfx, PFX_EVAL, s, f);
    f = sponge_absorb_words(s, f, 64 + F::ENC, [&](int m) { return V[m * 256 + t]; });
    sponge_pad(s, f, 0x01);
#pragma unroll
    for (int j = 0; j < 8; j++) pl.eval_proof[j * S + r] = kword(s, j);
}

// ------------------------------------------------------------- FLP randomness
template <class F, class Put>
MH_D void squeeze_elems(KState& s, int count, Put put) {
    sponge_squeeze_vec<F::W32>(
        s, count, [&](const uint32_t* w) { return F::valid(F::from_words(w)); },
        [&](int e, const uint32_t* w) { put(e, F::from_words(w)); });
}

struct FlpArgs {
    int agg_id;
    int level;
};

template <class F>
__global__ __launch_bounds__(256) void k_flp_rand(McParams p, Planes pl, FlpArgs a, const PrefixState* pfx) {
    typedef typename F::E E;
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= pl.stride) return;
    const int S = pl.stride;
    // beta share (get_beta_share, vidpf.py:263-279): w_L0 + w_R0, negated by the helper
    for (int e = 0; e < p.value_len; e++) {
        E x = pl_load<F>(pl.rootsum, e, S, r);
        pl_store<F>(pl.beta, e, S, r, a.agg_id ? F::neg(x) : x);
    }
    KState s;
    int f;
    // query rand: TS(verify_key, dst_alg(ctx, QUERY_RAND), nonce || le16(level))
    load_prefix(pfx, PFX_QUERY, s, f);
    f = sponge_absorb_words(s, f, 18, [&](int m) {
        return m < 4 ? pl.nonce[m * S + r] : (uint32_t)(a.level & 0xffff);
    });
    sponge_pad(s, f, 0x01);
    squeeze_elems<F>(s, p.query_rand_len, [&](int e, E x) { pl_store_lane<F>(pl.qr, e, S, r, x); });
    // proof share: leader from the input share, helper expands its seed
    if (a.agg_id == 0) {
        for (int k = 0; k < p.proof_len * F::W32; k++) pl.proof[(size_t)k * S + r] = pl.lps[(size_t)k * S + r];
    } else {
        load_prefix(pfx, PFX_PROOF_SHARE, s, f);
        f = sponge_absorb_words(s, f, 32, [&](int m) { return pl.seed[m * S + r]; });
        sponge_pad(s, f, 0x01);
        squeeze_elems<F>(s, p.proof_len, [&](int e, E x) { pl_store_lane<F>(pl.proof, e, S, r, x); });
    }
    if (p.joint_rand_len > 0) {
        // part = TS(seed, dst_alg(JOINT_RAND_PART), nonce || encode(beta_share[1:]))
        load_prefix(pfx, PFX_JR_PART, s, f);
        const int mw = p.meas_len * F::W32;
        f = sponge_absorb_words(s, f, 32 + 16 + mw * 4, [&](int m) {
            if (m < 8) return pl.seed[m * S + r];
            if (m < 12) return pl.nonce[(m - 8) * S + r];
            return pl.beta[(size_t)(F::W32 + m - 12) * S + r];
        });
        sponge_pad(s, f, 0x01);
        uint32_t part[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            part[j] = kword(s, j);
            pl.jr_part[j * S + r] = part[j];
        }
        // seed = TS(b'', dst_alg(JOINT_RAND_SEED), part_0 || part_1)
        load_prefix(pfx, PFX_JR_SEED, s, f);
        const bool leader = a.agg_id == 0;
        f = sponge_absorb_words(s, f, 64, [&](int m) {
            const bool own = leader ? (m < 8) : (m >= 8);
            const int j = m & 7;
            return own ? pl.jr_part[j * S + r] : pl.peer[j * S + r];
        });
        sponge_pad(s, f, 0x01);
#pragma unroll
        for (int j = 0; j < 8; j++) pl.jr_seed[j * S + r] = kword(s, j);
        // joint rand = TS(seed, dst_alg(JOINT_RAND), b'').next_vec(JRL)
        load_prefix(pfx, PFX_JR, s, f);
        f = sponge_absorb_words(s, f, 32, [&](int m) { return pl.jr_seed[m * S + r]; });
        sponge_pad(s, f, 0x01);
        squeeze_elems<F>(s, p.joint_rand_len, [&](int e, E x) { pl_store_lane<F>(pl.jr, e, S, r, x); });
    }
}

template <class F>
__global__ __launch_bounds__(256) void k_flp_query(McParams p, Planes pl, FlpConsts<F> c) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= pl.stride) return;
    const int S = pl.stride;
    const bool ok = flp_query<F>(p, c, pl.beta + (size_t)F::W32 * S, pl.proof, pl.qr, pl.jr, pl.verifier, S, r);
    if (!ok) pl.status[r] = -2;  // test point is a root of unity
}
