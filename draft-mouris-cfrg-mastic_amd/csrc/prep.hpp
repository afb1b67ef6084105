// prep_init and what reads its results: prefix states, trees, the work layout, one chunk's executor (struct
// Chunk; plans: schedule.hpp, memplan.hpp), the result getters, decide, the proof tree, the timing getters.
#pragma once
// ---------------------------------------------------------------- helpers
static void put_le16(std::vector<uint8_t>& v, uint32_t x) {
    v.push_back((uint8_t)x);
    v.push_back((uint8_t)(x >> 8));
}

// dst (poc/dst.py:30-32) and dst_alg (:35-42)
static std::vector<uint8_t> dst(const uint8_t* ctx, size_t n, int usage) {
    std::vector<uint8_t> d = {'m', 'a', 's', 't', 'i', 'c', 0, (uint8_t)usage};
    d.insert(d.end(), ctx, ctx + n);
    return d;
}
static std::vector<uint8_t> dst_alg(const uint8_t* ctx, size_t n, int usage, uint32_t id) {
    std::vector<uint8_t> d = {'m', 'a', 's', 't', 'i', 'c', 0, (uint8_t)usage,
                              (uint8_t)(id >> 24), (uint8_t)(id >> 16), (uint8_t)(id >> 8), (uint8_t)id};
    d.insert(d.end(), ctx, ctx + n);
    return d;
}

// Compute the sponge prefix states for (ctx, verify_key) on the device.  The
// verify key is XofTurboShake128's seed (u8 length prefix, mastic.py:302-306,
// 499-510), so any length up to 255 bytes is accepted (the reference's own
// driver uses 16, examples.py:38,176; VERIFY_KEY_SIZE is 32, mastic.py:73).
static int build_prefixes(mastic_ctx* c, const uint8_t* app_ctx, size_t ctx_len, const uint8_t* vk, size_t vk_len) {
    if (ctx_len > 65535 - 12) return fail(c, MASTIC_EINVAL, "ctx too long");
    if (vk && vk_len > 255) return fail(c, MASTIC_EINVAL, "verify key too long");
    // callers without a verify key (decide, shard, proof tree) never read the
    // two verify-key states (PFX_EVAL, PFX_QUERY: prep_init only), so any
    // states of the same ctx serve them.  Key layout: u8(len) || vk || ctx || 1.
    if (!vk && !c->pfx_key.empty()) {
        const size_t kl = c->pfx_key[0];
        if (c->pfx_key.size() == 1 + kl + ctx_len + 1 &&
            (ctx_len == 0 || std::equal(app_ctx, app_ctx + ctx_len, c->pfx_key.begin() + 1 + kl)))
            return 0;
    }
    static const uint8_t zero_vk[32] = {0};
    if (!vk) {
        vk = zero_vk;
        vk_len = 32;
    }
    std::vector<uint8_t> key(1, (uint8_t)vk_len);
    key.insert(key.end(), vk, vk + vk_len);
    key.insert(key.end(), app_ctx, app_ctx + ctx_len);
    key.push_back(1);  // never equal to the empty "none" key
    if (key == c->pfx_key) return 0;  // same verify key and ctx as the states already in pfx
    c->pfx_key.clear();
    std::vector<std::vector<uint8_t>> m(PFX_COUNT);
    auto xof_ts = [&](int id, const std::vector<uint8_t>& d, int seed_len, const uint8_t* seed) {
        put_le16(m[id], (uint32_t)d.size());
        m[id].insert(m[id].end(), d.begin(), d.end());
        m[id].push_back((uint8_t)seed_len);
        if (seed) m[id].insert(m[id].end(), seed, seed + seed_len);
    };
    auto xof_aes = [&](int id, const std::vector<uint8_t>& d) {
        put_le16(m[id], (uint32_t)d.size());
        m[id].insert(m[id].end(), d.begin(), d.end());
    };
    const uint32_t ID = c->p.alg_id;
    xof_aes(PFX_EXT, dst(app_ctx, ctx_len, 10));
    xof_aes(PFX_CONV, dst(app_ctx, ctx_len, 11));
    xof_ts(PFX_NODE, dst(app_ctx, ctx_len, 9), 16, nullptr);
    xof_ts(PFX_ONEHOT, dst_alg(app_ctx, ctx_len, 6, ID), 0, nullptr);
    xof_ts(PFX_PAYLOAD, dst_alg(app_ctx, ctx_len, 7, ID), 0, nullptr);
    xof_ts(PFX_EVAL, dst_alg(app_ctx, ctx_len, 8, ID), (int)vk_len, vk);
    xof_ts(PFX_QUERY, dst_alg(app_ctx, ctx_len, 2, ID), (int)vk_len, vk);
    xof_ts(PFX_PROOF_SHARE, dst_alg(app_ctx, ctx_len, 1, ID), 32, nullptr);
    xof_ts(PFX_JR_PART, dst_alg(app_ctx, ctx_len, 4, ID), 32, nullptr);
    xof_ts(PFX_JR_SEED, dst_alg(app_ctx, ctx_len, 3, ID), 0, nullptr);
    xof_ts(PFX_JR, dst_alg(app_ctx, ctx_len, 5, ID), 32, nullptr);
    xof_ts(PFX_PROVE_RAND, dst_alg(app_ctx, ctx_len, 0, ID), 32, nullptr);
    xof_ts(PFX_TREE, dst(app_ctx, ctx_len, 12), 0, nullptr);
    std::vector<uint8_t> all;
    std::vector<int> meta(2 * PFX_COUNT);
    for (int i = 0; i < PFX_COUNT; i++) {
        c->pfx_f[i] = (int)(m[i].size() % KECCAK_RATE);
        meta[i] = (int)all.size();
        meta[PFX_COUNT + i] = (int)m[i].size();
        all.insert(all.end(), m[i].begin(), m[i].end());
    }
    if (!c->pfx.ensure(sizeof(PrefixState) * PFX_COUNT) || !c->pfx_bytes.ensure(all.size()) ||
        !c->pfx_meta.ensure(meta.size() * sizeof(int)))
        return fail(c, MASTIC_ENOMEM, "out of device memory (prefix states)");
    HIPCHK(c, hipMemcpyAsync(c->pfx_bytes.p, all.data(), all.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->pfx_meta.p, meta.data(), meta.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_prefix_states, dim3(1), dim3(64), 0, c->stream, c->pfx_bytes.as<uint8_t>(),
                       c->pfx_meta.as<int>(), c->pfx_meta.as<int>() + PFX_COUNT, (int)PFX_COUNT,
                       c->pfx.as<PrefixState>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->pfx_host, c->pfx.p, sizeof(PrefixState) * PFX_COUNT, hipMemcpyDeviceToHost,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pfx_key = std::move(key);
    return 0;
}

// ---------------------------------------------------------------- tree
// Decode Mastic.encode_agg_param (mastic.py:413-435) and build the evaluated
// prefix tree of eval_with_siblings (vidpf.py:213-261): the children of every
// node on a candidate-prefix path, level by level in BFS (= lexicographic)
// order, which is the binder order of prep_init (mastic.py:263-275).
static int build_tree(mastic_ctx* c, const uint8_t* enc, size_t len, Tree** out) {
    std::vector<uint8_t> keyv(enc, enc + len);
    auto it = c->trees.find(keyv);
    if (it != c->trees.end()) {
        *out = it->second;
        return 0;
    }
    std::unique_ptr<Tree> owner(new Tree());  // the failure paths below free it and its device copy
    Tree* const t = owner.get();
    std::string perr;
    const int prc = tree_parse(c->p.bits, enc, len, t, &perr);
    if (prc != TREE_OK) return fail(c, prc == TREE_ENOMEM ? MASTIC_ENOMEM : MASTIC_EINVAL, "%s", perr.c_str());
    const size_t total = t->nodes;
    const size_t npar = t->parent_node.size();
    // one device allocation and one upload: [child_path | child_exp | child_pfx | parent_node]
    const size_t o_exp = total * 32, o_pfx = o_exp + total * 4, o_par = o_pfx + total * 4;
    const size_t bytes = o_par + std::max<size_t>(npar, 1) * 4;
    if (!t->dev.ensure(bytes)) return fail(c, MASTIC_ENOMEM, "out of device memory (tree)");
    uint8_t* d = t->dev.as<uint8_t>();
    t->d_path = (uint32_t*)d;
    t->d_exp = (int32_t*)(d + o_exp);
    t->d_pfx = (int32_t*)(d + o_pfx);
    t->d_parent = (int32_t*)(d + o_par);
    // staged through a pinned buffer and copied on the main stream (the
    // kernels that read the tree queue behind it); the previous upload must
    // have left the staging buffer first
    bool staged = false;
    if (c->tree_ev || hipEventCreateWithFlags(&c->tree_ev, hipEventDisableTiming) == hipSuccess) {
        if (c->tree_stage_bytes && hipEventSynchronize(c->tree_ev) != hipSuccess)
            return fail(c, MASTIC_EHIP, "tree upload failed");
        if (c->tree_stage_bytes < bytes) {
            if (c->tree_stage) (void)hipHostFree(c->tree_stage);
            c->tree_stage = nullptr;
            c->tree_stage_bytes = 0;
            const size_t want = std::max(bytes, (size_t)4 << 20);
            if (hipHostMalloc(&c->tree_stage, want, hipHostMallocDefault) == hipSuccess)
                c->tree_stage_bytes = want;
            else
                (void)hipGetLastError();
        }
        if (c->tree_stage_bytes >= bytes) {
            uint8_t* h = (uint8_t*)c->tree_stage;
            std::memcpy(h, t->child_path.data(), total * 32);
            std::memcpy(h + o_exp, t->child_exp.data(), total * 4);
            std::memcpy(h + o_pfx, t->child_pfx.data(), total * 4);
            if (npar) std::memcpy(h + o_par, t->parent_node.data(), npar * 4);
            if (hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                hipEventRecord(c->tree_ev, c->stream) != hipSuccess)
                return fail(c, MASTIC_EHIP, "tree upload failed");
            staged = true;
        }
    }
    if (!staged) {  // no pinned memory: synchronous uploads from the host vectors
        hipError_t e1 = hipMemcpy(t->d_path, t->child_path.data(), total * 32, hipMemcpyHostToDevice);
        hipError_t e2 = hipMemcpy(t->d_exp, t->child_exp.data(), total * 4, hipMemcpyHostToDevice);
        hipError_t e3 = hipMemcpy(t->d_pfx, t->child_pfx.data(), total * 4, hipMemcpyHostToDevice);
        hipError_t e4 = npar ? hipMemcpy(t->d_parent, t->parent_node.data(), npar * 4, hipMemcpyHostToDevice)
                             : hipSuccess;
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess)
            return fail(c, MASTIC_EHIP, "tree upload failed");
    }
    if (c->trees.size() > 64) {
        // queued kernels may still read the cached trees: their device
        // buffers are retired (freed at the next idle point of the ctx's
        // streams, mastic_ctx::bury), not freed here
        for (auto& kv : c->trees) {
            c->retire(kv.second->dev);
            delete kv.second;
        }
        c->trees.clear();
    }
    c->trees[keyv] = owner.release();
    *out = t;
    return 0;
}

// ---------------------------------------------------------------- work layout
struct WorkLayout {
    size_t words = 0;  // per report (plane count)
    size_t key, nonce, cw_seed, cw_ctrl, cw_w, cw_proof, lps, seed, peer, rk_ext, rk_conv, sp_onehot, sp_payload,
        rootsum, beta, eval_proof, proof, qr, jr, jr_part, jr_seed, verifier, status, cs[2], fr_w[2], onehot[3],
        payload[3];
};

static WorkLayout work_layout(const McParams& p, const Tree* t) {
    WorkLayout w;
    size_t o = 0;
    auto take = [&](size_t n) {
        size_t r = o;
        o += n;
        return r;
    };
    const size_t wl = (size_t)p.value_len * p.w32;
    w.key = take(4);
    w.nonce = take(4);
    w.cw_seed = take((size_t)p.bits * 4);
    w.cw_ctrl = take(p.bits);
    w.cw_w = take((size_t)p.bits * wl);
    w.cw_proof = take((size_t)p.bits * 8);
    w.lps = take((size_t)p.proof_len * p.w32);
    w.seed = take(8);
    w.peer = take(8);
    w.rk_ext = take(44);
    w.rk_conv = take(44);
    w.sp_onehot = take(50);
    w.sp_payload = take(50);
    w.rootsum = take(wl);
    w.beta = take(wl);
    w.eval_proof = take(8);
    w.proof = take((size_t)p.proof_len * p.w32);
    w.qr = take((size_t)p.query_rand_len * p.w32);
    w.jr = take((size_t)std::max(p.joint_rand_len, 1) * p.w32);
    w.jr_part = take(8);
    w.jr_seed = take(8);
    w.verifier = take((size_t)p.verifier_len * p.w32);
    w.status = take(1);
    for (int s = 0; s < 2; s++) {
        w.cs[s] = take((size_t)t->max_level_nodes * 5);
        w.fr_w[s] = take((size_t)std::max(t->max_exp, 1) * wl);
    }
    for (int k = 0; k < NSLOT; k++) {
        w.onehot[k] = take((size_t)t->max_level_nodes * 8);
        w.payload[k] = take((size_t)t->max_parents * wl);
    }
    w.words = o;
    return w;
}

static Planes make_planes(uint32_t* base, const WorkLayout& w, int n, int stride) {
    Planes pl;
    pl.n = n;
    pl.stride = stride;
    auto P = [&](size_t off) { return base + off * stride; };
    pl.key = P(w.key);
    pl.nonce = P(w.nonce);
    pl.cw_seed = P(w.cw_seed);
    pl.cw_ctrl = P(w.cw_ctrl);
    pl.cw_w = P(w.cw_w);
    pl.cw_proof = P(w.cw_proof);
    pl.lps = P(w.lps);
    pl.seed = P(w.seed);
    pl.peer = P(w.peer);
    pl.rk_ext = P(w.rk_ext);
    pl.rk_conv = P(w.rk_conv);
    pl.sp_onehot = P(w.sp_onehot);
    pl.sp_payload = P(w.sp_payload);
    pl.rootsum = P(w.rootsum);
    pl.beta = P(w.beta);
    pl.eval_proof = P(w.eval_proof);
    pl.proof = P(w.proof);
    pl.qr = P(w.qr);
    pl.jr = P(w.jr);
    pl.jr_part = P(w.jr_part);
    pl.jr_seed = P(w.jr_seed);
    pl.verifier = P(w.verifier);
    pl.status = (int32_t*)P(w.status);
    return pl;
}

// Event i of a pool that grows on demand.
static hipEvent_t event_at(std::vector<hipEvent_t>& pool, size_t i, unsigned flags) {
    while (pool.size() <= i) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, flags) != hipSuccess) return nullptr;
        pool.push_back(e);
    }
    return pool[i];
}
static hipEvent_t get_sync_event(mastic_ctx* c, size_t i) { return event_at(c->sync_ev, i, hipEventDisableTiming); }
static hipEvent_t get_event(mastic_ctx* c, size_t i) { return event_at(c->tm[c->tcur].ev, i, hipEventDefault); }

static int copy_planes(mastic_ctx* c, DevBuf& dst, size_t dst_stride, size_t dst_off, const uint32_t* src,
                       size_t src_stride, size_t n, size_t planes, hipStream_t s) {
    if (planes == 0) return 0;
    HIPCHK(c, hipMemcpy2DAsync(dst.as<uint32_t>() + dst_off, dst_stride * 4, src, src_stride * 4, n * 4, planes,
                               hipMemcpyDeviceToDevice, s));
    return 0;
}

// ---------------------------------------------------------------- prep_init
// The level kernel of each variant (level_kernel.hpp eval_aes_body; schedule.hpp
// LEVEL_VARIANTS lists the legal ones): the launch path and the LDS attribute
// loop of mastic_ctx_create both go through here.
typedef void (*LevelKernel)(McParams, Planes, AesArgs);
template <class F>
static LevelKernel level_kernel(int variant) {
    switch (variant) {
    case LV_GEN | LV_FC: return k_eval_aes<F, true, true>;
    case LV_FC_PAY: return k_eval_aes<F, true, true, false, true>;
    case 0: return k_eval_aes<F, false, false>;
    case LV_GEN: return k_eval_aes<F, true, false>;
    case LV_SPLIT: return k_eval_aes<F, false, false, true>;
    case LV_GEN | LV_SPLIT: return k_eval_aes<F, true, false, true>;
    case LV_WIDE: return k_eval_aes_wide<F, false>;
    case LV_WIDE | LV_GEN: return k_eval_aes_wide<F, true>;
    case LV_WIDE | LV_SPLIT: return k_eval_aes_wide<F, false, true>;
    case LV_WIDE | LV_GEN | LV_SPLIT: return k_eval_aes_wide<F, true, true>;
    }
    return nullptr;
}

// One chunk of reports [base, base + n) of a prep_init, in work area W, and
// its launch plan (schedule.hpp plan_chunk), which run() executes step by
// step.  lc: the frontier cache (or null); on a hit the parents are read from
// cin (the aggregator's node slot); the last level's nodes go to cout (the
// spare slot).  ss: the chunk's sponge stream.  tail: the stream of the
// chunk's last part (finalize, FLP, result and cache copies): the sponge
// stream when chunks are pipelined (the next chunk's evaluation, in the other
// half of the work arena, then overlaps this chunk's last sponges), else the
// main stream.  sev: next sync event of this chunk (consecutive pipelined
// chunks use disjoint ones); evi: next timing event of the call.
struct Chunk {
    mastic_ctx* c;
    mastic_reports* rep;
    const Tree* t;
    const WorkLayout& wl;
    const ChunkPlan& plan;
    int agg_id, n, stride;
    size_t base;
    uint32_t* W;
    hipStream_t ss, tail;
    LevelCache* lc;
    bool hit;
    const uint32_t* cin;
    uint32_t* cout;
    int in_nw, out_nw;  // words per node of cin / cout (CacheUse)
    size_t& evi;
    size_t sev;
    Planes pl;
    // A single-chunk call with the frontier cache keeps both binder sponges
    // and the root sum in the cache's planes (same stride): a hit resumes and
    // updates them in place, a miss fills them; no copies in or out.
    bool direct;
    // tiled level buffers (absorb_kernels.hpp AbsorbArgs): words per report group,
    // and between consecutive words of a report
    int oh_gstride, pay_gstride;
    static constexpr int bin_rstride = 64;
    int groups() const { return (n + 63) / 64; }  // report groups (rows beyond n are padding)
    int wlw() const { return c->p.value_len * c->p.w32; }
    uint32_t* plane(size_t off) const { return W + off * (size_t)stride; }
    // level binder buffers: the ring slots (with the frontier cache too: a
    // hit resumes both sponges from their cached states, so no level's
    // proofs or payload differences outlive the call)
    uint32_t* oh_buf(int lv) const { return plane(wl.onehot[lv % NSLOT]); }
    uint32_t* pay_buf(int lv) const { return plane(wl.payload[lv % NSLOT]); }
    hipStream_t stream(int role) const { return role == ST_MAIN ? c->stream : role == ST_THIRD ? c->stream3 : ss; }

    // Clears the header planes, then k_unpack and the row tiles.
    int unpack() {
        const McParams& p = c->p;
        // Every level plane (child seeds, frontier payloads, proof / payload-
        // difference ring, out shares, staged last-level payloads) is written
        // before it is read: level l reads only level l-1's nodes / expanded
        // nodes, which level l-1 wrote, and each candidate prefix is one child of
        // level L.  So only the per-report header planes (keys, correction words,
        // sponge states, FLP planes, status) are cleared -- 8 KB per report at C2
        // instead of the whole 9.7 MB work area (119 GB of fill per C2 step).  A
        // frontier-cache hit writes every header plane it reads except the
        // status plane: it clears just that.
        if (hit)
            HIPCHK(c, hipMemsetAsync(pl.status, 0, (size_t)stride * 4, c->stream));
        else {
            // Of the header, the keys, nonces and correction words (k_unpack: every
            // report row, every level the call reads) and the AES key schedules and
            // sponge states (k_setup: every row) are written in full before any
            // read, so only their padding rows are cleared; the planes between
            // (leader proof share, seeds: by aggregator and circuit) and from the
            // root sum on (accumulated root sum and FLP, result and status planes)
            // are cleared whole.  C2: 409 of 2,107 header words per report.
            // (work_layout order: key, nonce, cw_* | lps, seed, peer | rk_*, sp_* | rootsum .. status)
            HIPCHK(c, hipMemsetAsync(W + wl.lps * (size_t)stride, 0, (wl.rk_ext - wl.lps) * (size_t)stride * 4, c->stream));
            HIPCHK(c, hipMemsetAsync(W + wl.rootsum * (size_t)stride, 0, (wl.cs[0] - wl.rootsum) * (size_t)stride * 4,
                                     c->stream));
            if (stride > n)
                HIPCHK(c, hipMemset2DAsync(W + n, (size_t)stride * 4, 0, (size_t)(stride - n) * 4, wl.lps, c->stream));
            // level 0 reads its parent (the root) payload from fr_w[1]: zeros
            HIPCHK(c, hipMemsetAsync(W + wl.fr_w[1] * (size_t)stride, 0, (size_t)p.value_len * p.w32 * stride * 4, c->stream));
        }
        const size_t ps = mc_public_share_size(p), is = mc_input_share_size(p, agg_id);
        const uint8_t* pub = rep->pub.as<uint8_t>() + ps * base;
        const uint8_t* in_b = (agg_id == 0 ? rep->in0 : rep->in1).as<uint8_t>() + is * base;
        const int l_lo = hit ? t->L - 1 : 0, l_hi = t->L + 1;  // a hit recomputes level L-1's payloads: its CW
        // Rows of >= 16 KB to unpack per report (C4, C5), 8-byte aligned
        // (BITS a multiple of 32): the correction words and the leader proof
        // share, the bulk of a report's bytes, go through coalesced row tiles;
        // k_unpack keeps the nonce, key, control bits and seeds.  Same-box A/B
        // (profiles/r05_v37_ab_row_tile_unpack.txt): C5 +2.2 %, C4 +0.5 %;
        // the 1M sweep's rows (<= 5.9 KB) gained nothing in wall time (+0.1 %)
        // while its level kernels, started earlier under the previous chunk's
        // sponges, measured 1.3 % longer, so small rows keep one lane per report.
        const size_t nctrl = (2 * (size_t)p.bits + 7) / 8;
        const size_t row_bytes = (size_t)(l_hi - l_lo) * (16 + (size_t)p.value_len * p.enc + 32) +
                                 (agg_id == 0 ? (size_t)p.proof_len * p.enc : 0);
        // (grid y of every row-tile launch below: 64 words per workgroup row)
        const size_t max_words = std::max<size_t>((size_t)p.value_len * p.w32 * (l_hi - l_lo),
                                                  agg_id == 0 ? (size_t)p.proof_len * p.w32 : 0);
        const bool tiles = row_bytes >= 16384 && (((uintptr_t)pub | (uintptr_t)in_b | ps | is | nctrl) & 7) == 0 &&
                           (max_words + 63) / 64 < 65535;
        hipLaunchKernelGGL(k_unpack, dim3((n + 255) / 256), dim3(256), 0, c->stream, p, pl, agg_id,
                           rep->nonces.as<uint8_t>() + 16 * base, pub, in_b, l_lo, l_hi, tiles ? 1 : 0,
                           rep->wire_flags.as<uint8_t>() + base);
        if (tiles) {
            const int wlw_ = wlw(), nl = l_hi - l_lo;
            auto rows = [&](const uint8_t* src, size_t row_bytes, int nwords, uint32_t* dst) {
                if (nwords <= 0) return;
                hipLaunchKernelGGL(k_rows_to_planes, dim3((unsigned)((n + 63) / 64), (unsigned)((nwords + 63) / 64)),
                                   dim3(256), 0, c->stream, src, row_bytes, n, nwords, dst, stride);
            };
            const uint8_t* seg = pub + nctrl;
            rows(seg + 16 * (size_t)l_lo, ps, 4 * nl, pl.cw_seed + (size_t)4 * l_lo * stride);
            seg += 16 * (size_t)p.bits;
            rows(seg + (size_t)l_lo * p.value_len * p.enc, ps, wlw_ * nl, pl.cw_w + (size_t)wlw_ * l_lo * stride);
            seg += (size_t)p.bits * p.value_len * p.enc;
            rows(seg + 32 * (size_t)l_lo, ps, 8 * nl, pl.cw_proof + (size_t)8 * l_lo * stride);
            if (agg_id == 0) rows(in_b + 16, is, p.proof_len * p.w32, pl.lps);
        }
        HIPCHK(c, hipGetLastError());
        return 0;
    }

    // k_setup (AES key schedules, sponge states) unless the arena still holds
    // this batch's (mastic_ctx::rk); a hit's sponge states and root sum from the cache.
    int setup() {
        const bool whole = base == 0 && (size_t)n == rep->n && W == c->work.p;
        const bool rk_ok = hit && whole && c->rk.valid && c->rk.rep_id == rep->id &&
                           c->rk.rep_gen == rep->generation() && c->rk.n == (size_t)n && c->rk.stride == stride &&
                           c->rk.W == (const void*)W && c->rk.pfx_key == c->pfx_key;
        if (!rk_ok) {
            hipLaunchKernelGGL(k_setup, dim3((stride + 255) / 256), dim3(256), 0, c->stream, pl,
                               (const PrefixState*)c->pfx.p, hit ? 0 : 1);
            c->rk = {whole, rep->id, rep->generation(), (size_t)n, stride, (const void*)W, c->pfx_key};
        }
        HIPCHK(c, hipGetLastError());
        if (hit && !direct) {
            // levels 0..L-1 from the cache (its planes' columns base .. base + n).
            // The binder messages are BFS-ordered (mastic.py:263-275), so the
            // cached call's message is a prefix of this one's: both sponges resume
            // from their states at the end of the cached call (mid-block,
            // unpadded; k_finalize pads a register copy); and the root sum of the
            // cached level-0 evaluation (counter check).
            auto from_cache = [&](uint32_t* dst, const uint32_t* src, size_t planes) {
                return hipMemcpy2DAsync(dst, (size_t)stride * 4, src + base, lc->S * 4, (size_t)n * 4, planes,
                                        hipMemcpyDeviceToDevice, c->stream);
            };
            HIPCHK(c, from_cache(pl.sp_onehot, lc->sp.as<uint32_t>(), 50));
            HIPCHK(c, from_cache(pl.sp_payload, lc->sp.as<uint32_t>() + (size_t)50 * lc->S, 50));
            HIPCHK(c, from_cache(pl.rootsum, lc->rootsum.as<uint32_t>(), (size_t)wlw()));
        }
        return 0;
    }

    // One timing sextuple [aes0, aes1, proof0, proof1, absorb0, absorb1] of a
    // step (mastic_last_timing3 decodes strides of six): the first four are
    // recorded here on stream s, with `kernel` launched inside pair `slot`
    // (0 aes, 1 proof; -1: no kernel, both pairs empty); the absorb pair goes to
    // the step's sponge launch.
    template <class Fn>
    int timed_step(hipStream_t s, int slot, Fn&& kernel, hipEvent_t* e4, hipEvent_t* e5) {
        for (int i = 0; i < 4; i++) {
            HIPCHK(c, hipEventRecord(get_event(c, evi++), s));
            if (i == 2 * slot) kernel();
            if (i == 2 * slot + 1) HIPCHK(c, hipGetLastError());
        }
        *e4 = get_event(c, evi++);
        *e5 = get_event(c, evi++);
        return 0;
    }

    // The planned sponges [sp0, sp1) of a step whose end `ready` marks, each on
    // its stream after `ready`; (e4, e5): the absorb pair of the step's timing
    // sextuple.  Their ends are marked in c->sp_done.  The fill positions carry
    // across pieces as across levels (the plan tracks them).
    int launch_sponges(int sp0, int sp1, hipEvent_t ready, hipEvent_t e4, hipEvent_t e5) {
        for (int i = sp0; i < sp1; i++) {
            const SpongeLaunch& s = plan.sponges[i];
            const hipStream_t as = stream(s.stream);
            // the sponge's previous piece ran on another stream
            if (s.prev >= 0) HIPCHK(c, hipStreamWaitEvent(as, c->sp_done[s.prev], 0));
            hipEvent_t m4 = s.marks == MK_STEP ? e4 : nullptr, m5 = s.marks == MK_STEP ? e5 : nullptr;
            // a sponge piece that has no level-kernel launch of its own: an event
            // sextuple whose kernel pairs are empty
            if (s.marks == MK_PIECE && timed_step(as, -1, [] {}, &m4, &m5)) return MASTIC_EHIP;
            AbsorbArgs ab;
            ab.which0 = s.which0;
            ab.seg[0] = oh_buf(s.level) + (size_t)s.piece.node0 * 8 * bin_rstride;
            ab.gstride[0] = oh_gstride;
            ab.nbytes[0] = s.piece.nodes * 32;
            ab.f[0] = s.f_oh;
            ab.seg[1] = pay_buf(s.level) + (size_t)s.piece.parent0 * wlw() * bin_rstride;
            ab.gstride[1] = pay_gstride;
            ab.rstride = bin_rstride;
            ab.nbytes[1] = s.level > 0 ? s.piece.parents * wlw() * 4 : 0;
            ab.f[1] = s.f_pl;
            // The priority and debug arguments of AbsorbArgs and AesArgs were
            // experiment knobs; their A/Bs are settled and the executor pins the
            // values.  The fields stay in the argument structs (absorb_kernels.hpp,
            // level_kernel.hpp) because taking them out moves the kernels'
            // register allocation (DESIGN.md "Retired knobs").
            ab.prio = 3;
            ab.dbg = 0;
            if (as != c->stream) HIPCHK(c, hipStreamWaitEvent(as, ready, 0));
            if (m4) HIPCHK(c, hipEventRecord(m4, as));
            if (plan.pair)
                hipLaunchKernelGGL(k_absorb_pair, dim3((groups() * 64 * 2 + 255) / 256, (unsigned)s.nwh), dim3(256), 0, as,
                                   pl, ab);
            else
                hipLaunchKernelGGL(k_absorb, dim3((groups() * 64 + 255) / 256, (unsigned)s.nwh), dim3(256), 0, as, pl, ab);
            if (m5) HIPCHK(c, hipEventRecord(m5, as));
            HIPCHK(c, hipGetLastError());
            const hipEvent_t done = c->sp_done[i] = get_sync_event(c, sev++);
            HIPCHK(c, hipEventRecord(done, as));
            // measurement schedule (mastic_set_serial_sponges): the main stream waits
            // for this launch, so it runs alone on the chip (standalone sponge rate)
            if (c->serial_sponges && as != c->stream) HIPCHK(c, hipStreamWaitEvent(c->stream, done, 0));
            for (int w = s.which0; w < s.which0 + s.nwh; w++) (w ? c->pl_done : c->oh_done)[s.level] = done;
        }
        if (sp0 == sp1) {
            // no sponge follows (level 0 of a miss, a hit's level kernel): empty marks
            if (c->sponge_delay_us > 0) {
                // test hook: the sponge stream is still busy when these (empty)
                // marks are recorded there; nothing on the main stream waits for them
                const unsigned long long ticks =
                    (unsigned long long)c->sponge_delay_us * (unsigned long long)c->wall_khz / 1000;
                c->sponge_delay_us = 0;
                hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, ss, ticks);
                HIPCHK(c, hipGetLastError());
            }
            HIPCHK(c, hipEventRecord(e4, ss));
            HIPCHK(c, hipEventRecord(e5, ss));
        }
        return 0;
    }

    // One planned level-kernel launch (a whole level, or one parent range of a
    // segmented last level) on the main stream: the pointers of AesArgs from the
    // launch's level, parent range and proof job.
    template <class F>
    void launch_level(const LevelLaunch& v) {
        const int l = v.level, wlw = this->wlw();
        const size_t p0 = (size_t)v.p0;
        uint32_t* cs_level = plane(wl.cs[l & 1]);
        AesArgs a;
        a.level = l;
        a.agg_id = agg_id;
        a.n_parents = v.cnt;
        a.split = v.split;
        a.split_blocks = v.split_blocks;
        a.ppw = v.ppw;
        a.parent_node = t->d_parent + t->poff[l] + p0;
        a.child_exp = t->d_exp + t->off[l] + 2 * p0;
        a.child_pfx = t->d_pfx + t->off[l] + 2 * p0;
        // by child node / parent ordinal of the range: planes of the work
        // buffer, rows of the (tiled) payload-difference buffer
        a.cs_in = hit ? cin + base : plane(wl.cs[(l + 1) & 1]);
        a.cs_out = cs_level + 2 * p0 * 5 * stride;
        a.fr_w_in = plane(wl.fr_w[(l + 1) & 1]) + p0 * wlw * stride;
        a.in_stride = hit ? (int)lc->S : stride;
        a.fr_w_out = plane(wl.fr_w[l & 1]);
        a.payload = pay_buf(l) + p0 * wlw * bin_rstride;
        a.out = c->res[agg_id].out.as<uint32_t>() + base;  // columns base .. base + n of the result planes
        a.out_stride = (int)c->res[agg_id].stride;
        a.force_slow_blk = c->force_slow_blk;
        // frontier cache: stage this level's convert seeds (last level); on a
        // hit recompute the parents' payloads from the cached ones into the
        // (otherwise unused) parent-payload planes
        a.cache_out = (lc && l == t->L) ? cout + base + 2 * p0 * (size_t)out_nw * lc->S : nullptr;
        a.cache_stride = lc ? (int)lc->S : 0;
        a.wp_buf = plane(wl.fr_w[(l + 1) & 1]);
        // a payloads-format slot holds the parents' next seeds and payloads: nothing to recompute
        a.in_nw = hit ? in_nw : SEED_NODE_WORDS;
        a.out_nw = out_nw;
        a.recompute_wp = (hit && in_nw == SEED_NODE_WORDS) ? 1 : 0;
        a.fuse_proofs = v.fuse_proofs;
        a.cur_path_bytes = (l + 1 + 7) / 8;
        a.cur_child_path = t->d_path + (t->off[l] + 2 * p0) * 8;
        a.cur_onehot = oh_buf(l);
        a.aes_waves = v.aes_waves;
        a.par_waves = v.par_waves;
        a.proof_prio = a.aes_prio = a.dbg_skip = 0;  // pinned (launch_sponges)
        // the proof job: level l-1's nodes (seeds in cs_in), or an earlier range
        // of this level's (the previous launch's cs_out)
        const size_t n0 = (size_t)v.pv_node0;
        a.pv_level = v.pv_level;
        a.pv_nodes = v.pv_nodes;
        a.pv_npw = v.pv_npw;
        a.pv_path_bytes = (v.pv_level + 1 + 7) / 8;
        a.pv_child_path = v.pv_level >= 0 ? t->d_path + (t->off[v.pv_level] + n0) * 8 : nullptr;
        a.pv_onehot = v.pv_level >= 0 ? oh_buf(v.pv_level) + n0 * 8 * bin_rstride : nullptr;
        a.pv_cs = v.pv_level == l ? cs_level + n0 * 5 * stride : a.cs_in;
        a.oh_gstride = oh_gstride;
        a.pay_gstride = pay_gstride;
        a.bin_rstride = bin_rstride;
        a.np = (const PrefixState*)c->pfx.p + PFX_NODE;
        a.np_f = c->pfx_f[PFX_NODE];
        // the FC kernel that knows the payloads node format, where a slot of this launch has it
        const bool pay = (v.variant & LV_FC) && (a.in_nw > SEED_NODE_WORDS || (a.cache_out && a.out_nw > SEED_NODE_WORDS));
        hipLaunchKernelGGL(level_kernel<F>(pay ? LV_FC_PAY : v.variant), dim3(groups(), v.gy), dim3(64 * EVAL_WAVES), EVAL_LDS_BYTES,
                           c->stream, c->p, pl, a);
    }

    // The planned launches in order: each level kernel on the main stream, then
    // its sponges; then the final step (the last level's remaining node proofs,
    // or marks only) and its sponges.  Timing: one event sextuple per step.
    template <class F>
    int run_plan() {
        c->sp_done.assign(plan.sponges.size(), nullptr);
        c->oh_done.assign(t->L + 1, nullptr);
        c->pl_done.assign(t->L + 1, nullptr);
        hipEvent_t e4, e5;
        for (const LevelLaunch& v : plan.launches) {
            if (v.wait_level >= 0) {
                // proof / payload ring of NSLOT slots: this launch overwrites that level's
                const hipEvent_t oh = c->oh_done[v.wait_level], pay = c->pl_done[v.wait_level];
                HIPCHK(c, hipStreamWaitEvent(c->stream, oh, 0));
                if (pay && pay != oh) HIPCHK(c, hipStreamWaitEvent(c->stream, pay, 0));
            }
            if (int rc = timed_step(c->stream, 0, [&] { launch_level<F>(v); }, &e4, &e5)) return rc;
            hipEvent_t aes_done = get_sync_event(c, sev++);
            HIPCHK(c, hipEventRecord(aes_done, c->stream));
            if (int rc = launch_sponges(v.sp0, v.sp1, aes_done, e4, e5)) return rc;
        }
        const int l = t->L;
        ProofArgs pa;
        pa.level = l;
        pa.n_nodes = plan.final_nn;
        pa.npw = plan.final_npw;
        pa.path_bytes = (l + 1 + 7) / 8;
        pa.child_path = t->d_path + (t->off[l] + (size_t)plan.final_n0) * 8;
        pa.cs = plane(wl.cs[l & 1]) + (size_t)plan.final_n0 * 5 * stride;
        pa.onehot = oh_buf(l) + (size_t)plan.final_n0 * 8 * bin_rstride;
        pa.oh_gstride = oh_gstride;
        pa.bin_rstride = bin_rstride;
        pa.np = (const PrefixState*)c->pfx.p + PFX_NODE;
        pa.f = c->pfx_f[PFX_NODE];
        auto node_proofs = [&] {
            hipLaunchKernelGGL(k_node_proof, dim3(groups(), (pa.n_nodes + 4 * pa.npw - 1) / (4 * pa.npw)), dim3(256), 0,
                               c->stream, c->p, pl, pa);
        };
        // (a fused last level: its proofs came from the level kernel's AES waves)
        if (int rc = timed_step(c->stream, plan.fuse_last ? -1 : 1, node_proofs, &e4, &e5)) return rc;
        hipEvent_t np_done = get_sync_event(c, sev++);
        HIPCHK(c, hipEventRecord(np_done, c->stream));
        const int n_sponges = (int)plan.sponges.size();  // the last one is the final step's
        return launch_sponges(n_sponges - 1, n_sponges, np_done, e4, e5);
    }

    // FLP side stream, k_finalize, then the cache and result copies on the tail stream.
    template <class F>
    int finish() {
        const McParams& p = c->p;
        const PrefixState* pfx = (const PrefixState*)c->pfx.p;
        hipEvent_t flp_done = nullptr;
        if (t->weight_check) {
            // The FLP randomness and query (mastic.py:234-256) read only header
            // planes and level 0's root sum: on their own stream once the last
            // level kernel is done, beside the last level's sponges (a few
            // latency-bound chains that leave most of the chip idle: C5's last
            // payload chain runs ~34 ms) instead of after them.  (Right after
            // level 0 they slowed the level kernels beside them by as much as
            // they saved: C4 -1.8 %, profiles/r05_v36_ab_flp_side_stream.txt.)
            hipEvent_t lv_done = get_sync_event(c, sev++);
            HIPCHK(c, hipEventRecord(lv_done, c->stream));
            HIPCHK(c, hipStreamWaitEvent(c->stream4, lv_done, 0));
            FlpArgs fl{agg_id, t->L};
            hipLaunchKernelGGL(k_flp_rand<F>, dim3((stride + 255) / 256), dim3(256), 0, c->stream4, p, pl, fl, pfx);
            hipLaunchKernelGGL(k_flp_query<F>, dim3((stride + 255) / 256), dim3(256), 0, c->stream4, p, pl,
                               flp_consts<F>(p));
            HIPCHK(c, hipGetLastError());
            flp_done = get_sync_event(c, sev++);
            HIPCHK(c, hipEventRecord(flp_done, c->stream4));
        }
        // the tail follows the last piece of either sponge
        const hipEvent_t oh = c->oh_done[t->L], pay = c->pl_done[t->L];
        if (tail != stream(plan.last_stream)) HIPCHK(c, hipStreamWaitEvent(tail, oh, 0));
        if (pay && pay != oh) HIPCHK(c, hipStreamWaitEvent(tail, pay, 0));  // split schedule, segmented last level
        FinalArgs fa{agg_id, plan.f_oh, plan.f_pl};
        hipLaunchKernelGGL(k_finalize<F>, dim3((stride + 255) / 256), dim3(256), 0, tail, p, pl, fa, pfx);
        HIPCHK(c, hipGetLastError());
        // the status, verifier and joint-rand planes copied below are the FLP's
        if (flp_done) HIPCHK(c, hipStreamWaitEvent(tail, flp_done, 0));
        if (lc && !direct) {
            // work planes of this chunk -> cache planes (columns base .. base + n)
            auto to_cache = [&](uint32_t* dst, const uint32_t* src, size_t planes) {
                return hipMemcpy2DAsync(dst + base, lc->S * 4, src, (size_t)stride * 4, (size_t)n * 4, planes,
                                        hipMemcpyDeviceToDevice, tail);
            };
            // frontier cache for the next level (the last level's nodes are in the
            // spare slot already, written by its level kernel): the root sum
            if (!hit) HIPCHK(c, to_cache(lc->rootsum.as<uint32_t>(), pl.rootsum, (size_t)wlw()));
            // both sponges after levels 0..L (the tail waited for them above)
            HIPCHK(c, to_cache(lc->sp.as<uint32_t>(), pl.sp_onehot, 50));
            HIPCHK(c, to_cache(lc->sp.as<uint32_t>() + (size_t)50 * lc->S, pl.sp_payload, 50));
        }
        // results -> the agg_id slot (plane stride = all reports; the level
        // kernel wrote the out shares there)
        Result& R = c->res[agg_id];
        int rc = 0;
        rc |= copy_planes(c, R.eval_proof, R.stride, base, pl.eval_proof, stride, n, 8, tail);
        rc |= copy_planes(c, R.status, R.stride, base, (const uint32_t*)pl.status, stride, n, 1, tail);
        if (t->weight_check) {
            rc |= copy_planes(c, R.verifier, R.stride, base, pl.verifier, stride, n, (size_t)p.verifier_len * p.w32,
                              tail);
            if (p.joint_rand_len > 0) {
                rc |= copy_planes(c, R.jr_part, R.stride, base, pl.jr_part, stride, n, 8, tail);
                rc |= copy_planes(c, R.jr_seed, R.stride, base, pl.jr_seed, stride, n, 8, tail);
            }
        }
        return rc;
    }

    // Runs one chunk: unpack, key setup, the planned launches, finish.  The plan
    // also says how many sync and timing events the chunk takes: prep_init spaces
    // pipelined chunks' sync events by the former, and mastic_last_timing3
    // decodes the latter in strides of six, so a step that consumed another
    // number than planned is an error here, not a miscount there.  The check
    // is a tripwire for a plan and an executor that have drifted apart: it runs
    // after the chunk's work is queued, so it cannot keep a pipelined chunk
    // that overran its range from sharing sync events with its neighbour, only
    // fail the call (whose results are then never marked ready).  The C ABI has
    // no code for an internal error; MASTIC_EHIP with this text is the nearest.
    template <class F>
    int run() {
        const size_t evi0 = evi, sev0 = sev;
        pl = make_planes(W, wl, n, stride);
        direct = lc && base == 0 && (size_t)n == rep->n && lc->S == (size_t)stride;
        if (direct) {
            pl.sp_onehot = lc->sp.as<uint32_t>();
            pl.sp_payload = lc->sp.as<uint32_t>() + (size_t)50 * lc->S;
            pl.rootsum = lc->rootsum.as<uint32_t>();
        }
        oh_gstride = t->max_level_nodes * 8 * 64;
        pay_gstride = t->max_parents * wlw() * 64;
        int rc = unpack();
        if (rc || (rc = setup()) || (rc = run_plan<F>()) || (rc = finish<F>())) return rc;
        if (evi - evi0 != (size_t)plan.n_timing || sev - sev0 != (size_t)plan.n_sync)
            return fail(c, MASTIC_EHIP, "chunk used %zu timing and %zu sync events, its plan says %d and %d",
                        evi - evi0, sev - sev0, plan.n_timing, plan.n_sync);
        return 0;
    }
};

// Free HBM now (none: the query failed).
static std::optional<size_t> free_hbm() {
    size_t freeb = 0, total = 0;
    if (hipMemGetInfo(&freeb, &total) != hipSuccess) return std::nullopt;
    return freeb;
}

static uint64_t default_budget(mastic_ctx* c) {
    return default_budget(c->m, c->m.budget ? std::nullopt : free_hbm());
}

// Results and cache slots: HBM is held by the work arena (sized to the budget
// when the results were smaller) and by retired buffers, so the recovery frees
// both; the arena is re-allocated afterwards, within what is left (a
// 2M-report sweep's out shares reach 32 GB per aggregator).
static constexpr mastic_ctx::Reclaim RECLAIM_ALL{true, true, false, false};
// The work arena itself: only the retired buffers (cache slots, evicted trees) can make room.
static constexpr mastic_ctx::Reclaim RECLAIM_BURIED{false, false, true, true};

// The result buffers of a call over n reports.  One that must grow retires the
// old buffer (mastic_ctx::retire) and allocates with headroom, like DevBuf::grow.
static int size_results(mastic_ctx* c, Result& R, const Tree* t, size_t n) {
    const McParams& p = c->p;
    R.ready = false;
    R.n = n;
    R.stride = round_up(std::max<size_t>(n, 1), 64);
    R.weight_check = t->weight_check;
    R.n_prefixes = t->n_prefixes;
    const size_t S = R.stride;
    auto rgrow = [&](DevBuf& d, size_t want) {
        if (want <= d.bytes && d.p) return true;
        const size_t old = d.bytes;
        c->retire(d);
        d.own = true;
        return c->reclaim_ensure(d, std::max(want, old + old / 2), want, RECLAIM_ALL);
    };
    if (!rgrow(R.eval_proof, S * 8 * 4) || !rgrow(R.status, S * 4) ||
        !rgrow(R.out, S * 4 * std::max<size_t>(1, agg_rows(p, R) * p.w32)) ||
        !rgrow(R.verifier, S * 4 * (size_t)p.verifier_len * p.w32) || !rgrow(R.jr_part, S * 32) ||
        !rgrow(R.jr_seed, S * 32))
        return fail(c, MASTIC_ENOMEM, "out of device memory (results for %zu reports)", n);
    HIPCHK(c, hipMemsetAsync(R.jr_part.p, 0, S * 32, c->stream));
    HIPCHK(c, hipMemsetAsync(R.jr_seed.p, 0, S * 32, c->stream));
    return 0;
}

// What a call does with the frontier cache.
struct CacheUse {
    LevelCache* lc = nullptr;       // null: the call evaluates without the cache
    bool hit = false;               // it evaluates only its last level
    const uint32_t* cin = nullptr;  // a hit's parents: this aggregator's node slot
    uint32_t* cout = nullptr;       // the last level's nodes: the spare node slot
    int in_nw = SEED_NODE_WORDS;    // words per node of cin (the format of the call that wrote it)
    int out_nw = SEED_NODE_WORDS;   // words per node this call writes into cout
};

// Frontier cache: decide hit / miss and size the slots.  Runs before the work
// arena is sized, so the HBM budget sees the cache.
static CacheUse cache_slots(mastic_ctx* c, int agg_id, const Tree* t, const mastic_reports* rep,
                            const std::vector<uint8_t>& lkey) {
    CacheUse u;
    if (!c->frontier_cache) {
        c->lc[agg_id].drop();
        return u;
    }
    LevelCache* lc = &c->lc[agg_id];
    const size_t S1 = round_up(rep->n, 64) + (size_t)c->m.stride_pad;
    u.hit = frontier_hit(*lc, *t, rep->id, rep->generation(), rep->n, S1, lkey);
    if (lc->S != S1) {
        c->retire(lc->sp);
        c->retire(lc->rootsum);
        c->retire(lc->nd, S1);
        lc->S = S1;
    }
    if (c->fc_spare.S != S1) c->retire(c->fc_spare, S1);
    const size_t wlw = (size_t)c->p.value_len * c->p.w32;
    const size_t nl = (size_t)2 * t->n_parents[t->L];
    bool ok = c->reclaim_ensure(lc->sp, 0, 100 * S1 * 4, RECLAIM_ALL) &&
              c->reclaim_ensure(lc->rootsum, 0, wlw * S1 * 4, RECLAIM_ALL);
    // The format this call writes (memplan.hpp choose_node_words); auto asks for the free HBM.
    std::optional<size_t> free_bytes;
    bool queried = false;
    auto free_now = [&] {
        if (!queried) free_bytes = free_hbm();
        queried = true;
        return free_bytes;
    };
    const size_t held = c->lc[0].nd.buf.bytes + c->lc[1].nd.buf.bytes + c->fc_spare.buf.bytes;
    const bool by_rule = c->fc_nodes == FC_NODES_AUTO;
    size_t nw = (size_t)choose_node_words(c->fc_nodes, nl, wlw, S1, by_rule ? free_now() : std::nullopt, held);
    NodeSlot& spare = c->fc_spare;
    if (ok && !spare.holds(nl, nw)) {
        // the spare may be a former slot that queued kernels still read:
        // retire it, and free the retired buffers first
        const size_t old_words = spare.words;
        c->retire(spare, S1);
        if (c->idle()) c->bury();
        if (nw > SEED_NODE_WORDS) {
            // the wide format is an optimisation: one attempt, no draining of the
            // streams or release of the work arena for it; else seeds width
            const size_t words = spare_slot_words(nl, nw, old_words, free_now(), S1, by_rule, held);
            if (!c->inject_alloc_failure() && spare.buf.ensure(words * S1 * 4))
                spare.words = words;
            else
                nw = SEED_NODE_WORDS;
        }
        if (nw == SEED_NODE_WORDS) {
            const size_t words = spare_slot_words(nl, nw, old_words, free_now(), S1);
            ok = c->reclaim_ensure(spare.buf, 0, words * S1 * 4, RECLAIM_ALL);
            if (ok) spare.words = words;
        }
    }
    if (!ok) {  // not enough HBM for the cache: evaluate without it
        lc->release();
        return CacheUse();
    }
    if (!u.hit) lc->drop();  // refilled by this call
    u.lc = lc;
    u.cin = u.hit ? lc->nd.buf.as<uint32_t>() : nullptr;
    u.cout = spare.buf.as<uint32_t>();
    u.in_nw = u.hit ? lc->node_words : SEED_NODE_WORDS;
    u.out_nw = (int)nw;
    return u;
}

// The work arena of a call: used as it is, or re-allocated (memplan.hpp
// plan_arena).  *by_budget: the reports per chunk the call's budget allows.
static int size_arena(mastic_ctx* c, size_t n, size_t per_report, bool cache_on, size_t* by_budget) {
    const bool fits = arena_fits(c->m, n, per_report, c->work.bytes);
    const uint64_t budget =
        call_budget(c->m, n, per_report, fits, cache_on, (fits || c->m.budget) ? std::nullopt : free_hbm());
    const ArenaPlan a = plan_arena(c->m, n, per_report, c->work.bytes, budget, cache_on);
    *by_budget = a.by_budget;
    if (a.action == ArenaPlan::TOO_SMALL)
        return fail(c, MASTIC_ENOMEM, "work buffers of 64 reports exceed the memory budget");
    if (a.action == ArenaPlan::USE) return 0;
    c->rk.valid = false;  // the arena may be re-allocated (possibly at the same address)
    if (!c->reclaim_ensure(c->work, a.arena, a.want, RECLAIM_BURIED))
        return fail(c, MASTIC_ENOMEM, "out of device memory (work %zu bytes)", a.want);
    return 0;
}

extern "C" int mastic_prep_init(mastic_ctx* c, mastic_reports* rep, const uint8_t* verify_key, size_t vk_len,
                                const uint8_t* app_ctx, size_t ctx_len, int agg_id, const uint8_t* enc_agg_param,
                                size_t agg_param_len) {
    DeviceScope ds_(c);
    if (!c || !rep || rep->ctx != c) return fail(c, MASTIC_EINVAL, "bad ctx/reports");
    if (agg_id != 0 && agg_id != 1) return fail(c, MASTIC_EINVAL, "invalid aggregator ID");
    if ((agg_id == 0 && !rep->in0.p) || (agg_id == 1 && !rep->in1.p))
        return fail(c, MASTIC_EINVAL, "reports hold no input shares for this aggregator");
    if (!verify_key && vk_len) return fail(c, MASTIC_EINVAL, "verify key required");
    static const uint8_t empty_vk[1] = {0};
    if (!verify_key) verify_key = empty_vk;
    c->tcur = agg_id;
    Tree* t = nullptr;
    int rc = build_tree(c, enc_agg_param, agg_param_len, &t);
    if (rc) return rc;
    if ((rc = build_prefixes(c, app_ctx, ctx_len, verify_key, vk_len))) return rc;
    const McParams& p = c->p;
    WorkLayout wl = work_layout(p, t);
    const size_t n = rep->n;
    Result& R = c->res[agg_id];
    if ((rc = size_results(c, R, t, n))) return rc;
    if (n == 0) {
        R.ready = true;
        return 0;
    }
    const size_t pad = (size_t)c->m.stride_pad;
    std::vector<uint8_t> lkey(1, (uint8_t)vk_len);
    lkey.insert(lkey.end(), verify_key, verify_key + vk_len);
    lkey.insert(lkey.end(), app_ctx, app_ctx + ctx_len);
    const CacheUse cu = cache_slots(c, agg_id, t, rep, lkey);
    LevelCache* const lc = cu.lc;
    const bool hit = cu.hit;
    size_t by_budget = 0;
    if ((rc = size_arena(c, n, wl.words * 4, lc != nullptr, &by_budget))) return rc;
    // the chunks (memplan.hpp), and the launch plans (schedule.hpp) of a full chunk and, if shorter, of the last one
    const ChunkSizes cs = plan_chunks(c->m, n, wl.words * 4, c->work.bytes, by_budget);
    const size_t chunk = cs.chunk;
    const bool pipe = cs.pipe;
    ChunkPlan* plans[2] = {&c->plans[0], &c->plans[cs.n_last != cs.n_full]};
    for (int i = 0; i <= (cs.n_last != cs.n_full); i++)
        plan_chunk(c->k, p, *t, (int)(i ? cs.n_last : cs.n_full), hit, lc != nullptr, pipe, c->pfx_f[PFX_ONEHOT],
                   c->pfx_f[PFX_PAYLOAD], plans[i]);
    // sync events one chunk uses: pipelined chunks alternate between two disjoint ranges of them
    const size_t nsev = (size_t)std::max(plans[0]->n_sync, plans[1]->n_sync);
    size_t evi = 0;
    hipEvent_t t0 = get_event(c, evi++), t1 = get_event(c, evi++);
    HIPCHK(c, hipEventRecord(t0, c->stream));
    hipEvent_t half_free[2] = {get_sync_event(c, 2 * nsev), get_sync_event(c, 2 * nsev + 1)};
    for (size_t b = 0, k = 0; b < n; b += chunk, k++) {
        const int nn = (int)std::min(chunk, n - b), stride = (int)(round_up(nn, 64) + pad);
        const int h = pipe ? (int)(k & 1) : 0;
        if (pipe && k >= 2) HIPCHK(c, hipStreamWaitEvent(c->stream, half_free[h], 0));
        uint32_t* W = c->work.as<uint32_t>() + h * cs.half;
        // pipelined chunks alternate between two sponge streams: a chunk's
        // sponges must not queue behind the previous chunk's trailing ones
        hipStream_t ss = (pipe && h) ? c->stream3 : c->stream2, tail = pipe ? ss : c->stream;
        Chunk ck{c, rep, t, wl, *plans[b + chunk >= n], agg_id, nn, stride, b, W, ss, tail, lc, hit, cu.cin, cu.cout,
                 cu.in_nw, cu.out_nw, evi, h * nsev};
        rc = with_field(p, [&](auto f) { return ck.template run<typename decltype(f)::type>(); });
        if (rc) {
            if (lc) lc->drop();
            return rc;
        }
        if (pipe) HIPCHK(c, hipEventRecord(half_free[h], ss));
    }
    if (pipe) {
        // later work on the main stream (results, aggregate, the next call) sees every chunk's tail
        hipEvent_t done = get_sync_event(c, 2 * nsev + 2), done3 = get_sync_event(c, 2 * nsev + 3);
        HIPCHK(c, hipEventRecord(done, c->stream2));
        HIPCHK(c, hipEventRecord(done3, c->stream3));
        HIPCHK(c, hipStreamWaitEvent(c->stream, done, 0));
        HIPCHK(c, hipStreamWaitEvent(c->stream, done3, 0));
    }
    if (lc) {
        // the spare slot now holds this call's last level: it becomes the
        // aggregator's slot, and the old slot (read by this call's hit) the
        // spare, overwritten only by later calls' kernels (stream order)
        lc->nd.swap(c->fc_spare);  // (both of this call's stride: cache_slots)
        frontier_commit(*lc, *t, rep->id, rep->generation(), n, lkey, cu.out_nw);
    }
    c->last_hit = hit;
    auto fmt = [](int nw) { return nw > SEED_NODE_WORDS ? FC_NODES_PAYLOADS : FC_NODES_SEEDS; };
    c->last_nodes_in = hit ? fmt(cu.in_nw) : -1;
    c->last_nodes_out = lc ? fmt(cu.out_nw) : -1;
    HIPCHK(c, hipEventRecord(t1, c->stream));
    c->tm[c->tcur].n_eval = -(int)evi;  // timing pending (resolved by mastic_last_timing)
    R.ready = true;
    return 0;
}

// Report-major wire rows of plane segments into dst (device), on c->stream.
static int gather_rows(mastic_ctx* c, const RowSegs& sg, size_t n, size_t stride, void* dst) {
    const size_t words = (size_t)sg.words[0] + sg.words[1] + sg.words[2];
    if (n == 0 || words == 0) return 0;
    const size_t total = n * words;
    // grid-stride kernel: at most 2^20 workgroups (2^28 work-items) per launch
    const size_t blocks = std::min<size_t>((total + 255) / 256, (size_t)1 << 20);
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)blocks), dim3(256), 0, c->stream, sg, (int)n, (int)stride,
                       (uint32_t*)dst);
    HIPCHK(c, hipGetLastError());
    return 0;
}

// The prep shares of result slot R as wire rows (mastic.py:543-552):
// eval_proof || [jr_part] || [verifier].
static RowSegs prep_share_segs(const McParams& p, const Result& R) {
    RowSegs sg{};
    sg.seg[0] = R.eval_proof.as<uint32_t>();
    sg.words[0] = 8;
    if (R.weight_check) {
        int k = 1;
        if (p.joint_rand_len > 0) {
            sg.seg[k] = R.jr_part.as<uint32_t>();
            sg.words[k++] = 8;
        }
        sg.seg[k] = R.verifier.as<uint32_t>();
        sg.words[k] = p.verifier_len * p.w32;
    }
    return sg;
}

extern "C" int mastic_prep_result(mastic_ctx* c, int agg_id, uint8_t* prep_shares, uint8_t* jr_seeds,
                                  uint8_t* out_shares, int32_t* status) {
    DeviceScope ds_(c);
    Result* const Rp = ready_result(c, agg_id);
    if (!Rp) return MASTIC_EINVAL;
    Result& R = *Rp;
    c->tcur = agg_id;
    const McParams& p = c->p;
    const size_t n = R.n, S = R.stride;
    // Every output is encoded on the GPU into a staging buffer (planes ->
    // report-major wire bytes) and copied out once: no per-report host loop.
    auto emit = [&](const RowSegs& sg, void* host) -> int {
        const size_t bytes = n * 4 * ((size_t)sg.words[0] + sg.words[1] + sg.words[2]);
        if (!host || bytes == 0) return 0;
        if (!c->stage.grow(bytes)) return fail(c, MASTIC_ENOMEM, "out of device memory (result staging)");
        if (gather_rows(c, sg, n, S, c->stage.p)) return -1;
        HIPCHK(c, hipMemcpyAsync(host, c->stage.p, bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    };
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->bury();  // the stream is idle (it joined the sponge stream before k_finalize)
    if (n == 0) return 0;
    if (emit(prep_share_segs(p, R), prep_shares)) return -1;
    if (jr_seeds && !(R.weight_check && p.joint_rand_len > 0)) {
        memset(jr_seeds, 0, 32 * n);  // no joint rand in this call
    } else if (emit(RowSegs{{R.jr_seed.as<uint32_t>(), nullptr, nullptr}, {8, 0, 0}}, jr_seeds)) {
        return -1;
    }
    const int ow = (int)(agg_rows(p, R) * p.w32);
    if (emit(RowSegs{{R.out.as<uint32_t>(), nullptr, nullptr}, {ow, 0, 0}}, out_shares)) return -1;
    if (emit(RowSegs{{(const uint32_t*)R.status.p, nullptr, nullptr}, {1, 0, 0}}, status)) return -1;
    return 0;
}

extern "C" int mastic_decide_results(mastic_ctx* c, const uint8_t* app_ctx, size_t ctx_len, uint8_t* accept_out,
                                     uint8_t* decide_out) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    Result &R0 = c->res[0], &R1 = c->res[1];
    if (!R0.ready || !R1.ready) return fail(c, MASTIC_EINVAL, "decide needs both aggregators' prep_init results");
    if (R0.n != R1.n || R0.weight_check != R1.weight_check || R0.n_prefixes != R1.n_prefixes)
        return fail(c, MASTIC_EINVAL, "the two prep_init results are for different batches / agg params");
    const size_t n = R0.n, S = R0.stride;
    if (n == 0) return 0;
    int rc = build_prefixes(c, app_ctx, ctx_len, nullptr, 0);
    if (rc) return rc;
    const McParams& p = c->p;
    const size_t psz = mc_prep_share_size(p, R0.weight_check);
    // both prep shares as wire rows (k_decide's input), decide, accept
    const size_t need = 2 * n * psz + 32 * n + 2 * n + 256 + S * 4 * (size_t)std::max(1, p.verifier_len * p.w32);
    if (!c->stage.grow(need)) return fail(c, MASTIC_ENOMEM, "out of device memory (decide staging)");
    uint8_t* ps0 = c->stage.as<uint8_t>();
    uint8_t* ps1 = ps0 + n * psz;
    uint8_t* msg = ps1 + n * psz;
    uint8_t* code = msg + 32 * n;
    uint8_t* acc = code + n;
    uint32_t* ver = (uint32_t*)(((uintptr_t)(acc + n) + 255) & ~(uintptr_t)255);  // FLP scratch planes
    if (gather_rows(c, prep_share_segs(p, R0), n, S, ps0)) return -1;
    if (gather_rows(c, prep_share_segs(p, R1), n, S, ps1)) return -1;
    HIPCHK(c, hipMemsetAsync(msg, 0, 32 * n, c->stream));
    if ((rc = launch_decide(c, n, S, R0.weight_check, ps0, ps1, psz, ver, msg, code))) return rc;
    hipLaunchKernelGGL(k_accept, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (int)n, (int)S,
                       (int)(R0.weight_check && p.joint_rand_len > 0), code, (const int32_t*)R0.status.p,
                       (const int32_t*)R1.status.p, msg, R0.jr_seed.as<uint32_t>(), R1.jr_seed.as<uint32_t>(), acc);
    HIPCHK(c, hipGetLastError());
    if (accept_out) HIPCHK(c, hipMemcpyAsync(accept_out, acc, n, hipMemcpyDeviceToHost, c->stream));
    if (decide_out) HIPCHK(c, hipMemcpyAsync(decide_out, code, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->bury();
    return 0;
}

// Eval-proof Merkle tree (proof-aggregation mode, decide_kernels.hpp k_proof_tree_*)
// over the last prep_init result of agg_id.
extern "C" int mastic_proof_tree(mastic_ctx* c, int agg_id, const uint8_t* app_ctx, size_t ctx_len,
                                 uint8_t* nodes_out, size_t n_nodes) {
    DeviceScope ds_(c);
    Result* const Rp = ready_result(c, agg_id);
    if (!Rp) return MASTIC_EINVAL;
    Result& R = *Rp;
    const size_t n = R.n;
    size_t total = 0;
    for (size_t m = n; m > 0; m = (m == 1) ? 0 : (m + 1) / 2) total += m;
    if (n_nodes != total) return fail(c, MASTIC_EINVAL, "proof tree has incorrect size");
    if (n == 0) return 0;
    if (n > (size_t)INT32_MAX / 2) return fail(c, MASTIC_EINVAL, "batch too large for a proof tree");
    int rc = build_prefixes(c, app_ctx, ctx_len, nullptr, 0);
    if (rc) return rc;
    DevBuf nodes;
    if (!nodes.ensure(total * 32)) return fail(c, MASTIC_ENOMEM, "out of device memory (proof tree)");
    uint32_t* d = nodes.as<uint32_t>();
    hipLaunchKernelGGL(k_proof_tree_leaves, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       R.eval_proof.as<uint32_t>(), (int)n, (int)R.stride, d);
    size_t off = 0;
    for (size_t m = n; m > 1; m = (m + 1) / 2) {
        const size_t mo = (m + 1) / 2;
        hipLaunchKernelGGL(k_proof_tree_level, dim3((unsigned)((mo + 255) / 256)), dim3(256), 0, c->stream,
                           (const PrefixState*)c->pfx.p, d + off * 8, (int)m, d + (off + m) * 8);
        off += m;
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(nodes_out, d, total * 32, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int mastic_last_timing(mastic_ctx* c, double* eval_ms, int* eval_launches, double* absorb_ms,
                                  int* absorb_launches, double* total_ms) {
    return mastic_last_timing3(c, eval_ms, eval_launches, nullptr, nullptr, absorb_ms, absorb_launches, total_ms);
}

extern "C" int mastic_last_timing3(mastic_ctx* c, double* aes_ms, int* aes_launches, double* proof_ms,
                                   int* proof_launches, double* absorb_ms, int* absorb_launches, double* total_ms) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->tm[c->tcur].n_eval < 0) {
        // some timing marks sit on the sponge streams without the main stream
        // waiting for them (a single-chunk hit's empty sponge marks, recorded
        // on the sponge stream while its sponges run on the main stream):
        // wait for the marks themselves (an unwaited mark gave "device not
        // ready" in a 4-rank run sharing one GPU)
        for (int i = 0; i < -c->tm[c->tcur].n_eval; i++) HIPCHK(c, hipEventSynchronize(c->tm[c->tcur].ev[i]));
        // events: [t0, t1] then per level [aes0, aes1, proof0, proof1, absorb0, absorb1]
        const size_t evi = (size_t)(-c->tm[c->tcur].n_eval);
        double ta = 0, tp = 0, tb = 0;
        int n = 0;
        float ms = 0;
        for (size_t i = 2; i + 6 <= evi; i += 6) {
            HIPCHK(c, hipEventElapsedTime(&ms, c->tm[c->tcur].ev[i], c->tm[c->tcur].ev[i + 1]));
            ta += ms;
            HIPCHK(c, hipEventElapsedTime(&ms, c->tm[c->tcur].ev[i + 2], c->tm[c->tcur].ev[i + 3]));
            tp += ms;
            HIPCHK(c, hipEventElapsedTime(&ms, c->tm[c->tcur].ev[i + 4], c->tm[c->tcur].ev[i + 5]));
            tb += ms;
            n++;
        }
        HIPCHK(c, hipEventElapsedTime(&ms, c->tm[c->tcur].ev[0], c->tm[c->tcur].ev[1]));
        c->tm[c->tcur].t_total = ms;
        c->tm[c->tcur].t_eval = ta;
        c->tm[c->tcur].t_proof = tp;
        c->tm[c->tcur].t_absorb = tb;
        c->tm[c->tcur].n_eval = n;
        c->tm[c->tcur].n_absorb = n;
    }
    if (aes_ms) *aes_ms = c->tm[c->tcur].t_eval;
    if (aes_launches) *aes_launches = c->tm[c->tcur].n_eval;
    if (proof_ms) *proof_ms = c->tm[c->tcur].t_proof;
    if (proof_launches) *proof_launches = c->tm[c->tcur].n_absorb;
    if (absorb_ms) *absorb_ms = c->tm[c->tcur].t_absorb;
    if (absorb_launches) *absorb_launches = c->tm[c->tcur].n_absorb;
    if (total_ms) *total_ms = c->tm[c->tcur].t_total;
    return 0;
}

extern "C" int mastic_tree_stats(mastic_ctx* c, const uint8_t* enc, size_t len, uint64_t* nodes, uint64_t* interior,
                                 uint64_t* max_level_nodes) {
    DeviceScope ds_(c);
    Tree* t = nullptr;
    int rc = build_tree(c, enc, len, &t);
    if (rc) return rc;
    if (nodes) *nodes = t->nodes;
    if (interior) *interior = t->interior;
    if (max_level_nodes) *max_level_nodes = (uint64_t)t->max_level_nodes;
    return 0;
}

extern "C" int mastic_work_bytes(mastic_ctx* c, const uint8_t* enc, size_t len, uint64_t* per_report) {
    DeviceScope ds_(c);
    Tree* t = nullptr;
    int rc = build_tree(c, enc, len, &t);
    if (rc) return rc;
    if (per_report) *per_report = (uint64_t)work_layout(c->p, t).words * 4;
    return 0;
}

extern "C" int mastic_prep_init_batch(mastic_ctx* c, const uint8_t* verify_key, size_t vk_len, const uint8_t* app_ctx,
                                      size_t ctx_len, int agg_id, const uint8_t* enc_agg_param, size_t agg_param_len,
                                      size_t n, const uint8_t* nonces, const uint8_t* public_shares,
                                      const uint8_t* input_shares, uint8_t* prep_shares_out, uint8_t* jr_seeds_out,
                                      uint8_t* out_shares_out, int32_t* status_out) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    if (agg_id != 0 && agg_id != 1) return fail(c, MASTIC_EINVAL, "invalid aggregator ID");
    mastic_reports* rep = nullptr;
    int rc = mastic_reports_create(c, n, &rep);
    if (rc) return rc;
    rc = mastic_reports_upload(rep, nonces, public_shares, agg_id == 0 ? input_shares : nullptr,
                               agg_id == 1 ? input_shares : nullptr);
    if (!rc) rc = mastic_prep_init(c, rep, verify_key, vk_len, app_ctx, ctx_len, agg_id, enc_agg_param, agg_param_len);
    if (!rc) rc = mastic_prep_result(c, agg_id, prep_shares_out, jr_seeds_out, out_shares_out, status_out);
    mastic_reports_destroy(rep);
    return rc;
}

// ---------------------------------------------------------------- decide
extern "C" int mastic_decide_batch(mastic_ctx* c, const uint8_t* app_ctx, size_t ctx_len, const uint8_t* enc,
                                   size_t len, size_t n, const uint8_t* ps0, const uint8_t* ps1, uint8_t* msgs_out,
                                   uint8_t* valid_out) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    Tree* t = nullptr;
    int rc = build_tree(c, enc, len, &t);
    if (rc) return rc;
    if (n == 0) return 0;
    if ((rc = build_prefixes(c, app_ctx, ctx_len, nullptr, 0))) return rc;
    const McParams& p = c->p;
    const size_t psz = mc_prep_share_size(p, t->weight_check);
    const size_t stride = round_up(n, 64);
    DevBuf a, b, ver, msg, st;
    if (!a.ensure(psz * n) || !b.ensure(psz * n) || !ver.ensure(stride * 4 * (size_t)p.verifier_len * p.w32) ||
        !msg.ensure(32 * n) || !st.ensure(n))
        return fail(c, MASTIC_ENOMEM, "out of device memory (decide)");
    HIPCHK(c, hipMemcpyAsync(a.p, ps0, psz * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.p, ps1, psz * n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(msg.p, 0, 32 * n, c->stream));
    if ((rc = launch_decide(c, n, stride, (int)t->weight_check, a.as<uint8_t>(), b.as<uint8_t>(), psz, ver.as<uint32_t>(),
                            msg.as<uint8_t>(), st.as<uint8_t>())))
        return rc;
    if (msgs_out && t->weight_check && p.joint_rand_len > 0)
        HIPCHK(c, hipMemcpyAsync(msgs_out, msg.p, 32 * n, hipMemcpyDeviceToHost, c->stream));
    if (valid_out) HIPCHK(c, hipMemcpyAsync(valid_out, st.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
