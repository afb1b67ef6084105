// Resident batches (mastic_reports): create, view, up / download, wire check, shard, compaction.
#pragma once
// ---------------------------------------------------------------- reports
extern "C" int mastic_reports_create(mastic_ctx* c, size_t n, mastic_reports** out) {
    DeviceScope ds_(c);
    if (!c || !out) return MASTIC_EINVAL;
    std::unique_ptr<mastic_reports> r(new mastic_reports());
    r->ctx = c;
    r->n = n;
    const McParams& p = c->p;
    if (!r->nonces.ensure(16 * n) || !r->pub.ensure((size_t)mc_public_share_size(p) * n) || !r->wire_flags.ensure(n))
        return fail(c, MASTIC_ENOMEM, "out of device memory (reports)");
    // (null stream, like the blocking copies of upload / shard that follow it there and are done before
    // the first kernel that touches the flags is queued on the ctx's stream)
    if (hipMemset(r->wire_flags.p, 0, r->wire_flags.bytes) != hipSuccess)
        return fail(c, MASTIC_EHIP, "reports: clearing the wire flags failed");
    *out = r.release();
    return 0;
}

extern "C" int mastic_reports_view(mastic_reports* rep, size_t first, size_t count, mastic_reports** out) {
    DeviceScope ds_(rep ? rep->ctx : nullptr);
    if (!rep || !out) return MASTIC_EINVAL;
    mastic_ctx* c = rep->ctx;
    if (first > rep->n || count > rep->n - first) return fail(c, MASTIC_EINVAL, "view out of range");
    const McParams& p = c->p;
    mastic_reports* r = new mastic_reports();
    r->ctx = c;
    r->n = count;
    r->gen = rep->gen;  // one contents generation for the batch and all its views
    const size_t ps = mc_public_share_size(p), i0 = mc_input_share_size(p, 0), i1 = mc_input_share_size(p, 1);
    r->nonces.view(rep->nonces, 16 * first, 16 * count);
    r->pub.view(rep->pub, ps * first, ps * count);
    r->in0.view(rep->in0, i0 * first, i0 * count);
    r->in1.view(rep->in1, i1 * first, i1 * count);
    r->wire_flags.view(rep->wire_flags, first, count);
    *out = r;
    return 0;
}

extern "C" void mastic_reports_destroy(mastic_reports* r) {
    DeviceScope ds_(r ? r->ctx : nullptr);
    delete r;
}
extern "C" size_t mastic_reports_count(const mastic_reports* r) { return r ? r->n : 0; }

// Range check of the wire field elements of the segments just written (pub:
// the public shares, in0: the leader input shares), queued on the ctx's
// stream ahead of any prep_init over the batch.
static int validate_wire(mastic_ctx* c, mastic_reports* r, bool pub, bool in0) {
    if (r->n == 0 || (!pub && !in0)) return 0;
    const dim3 grid((unsigned)((r->n + 3) / 4));
    const uint8_t* dp = pub ? r->pub.as<uint8_t>() : nullptr;
    const uint8_t* di = in0 ? r->in0.as<uint8_t>() : nullptr;
    with_field(c->p, [&](auto f) {
        using F = typename decltype(f)::type;
        hipLaunchKernelGGL(k_validate_wire<F>, grid, dim3(256), 0, c->stream, c->p, (int)r->n, dp, di,
                           r->wire_flags.as<uint8_t>());
    });
    HIPCHK(c, hipGetLastError());
    return 0;
}

extern "C" int mastic_reports_upload(mastic_reports* r, const uint8_t* nonces, const uint8_t* pub,
                                     const uint8_t* in0, const uint8_t* in1) {
    DeviceScope ds_(r ? r->ctx : nullptr);
    if (!r) return MASTIC_EINVAL;
    mastic_ctx* c = r->ctx;
    const McParams& p = c->p;
    const size_t n = r->n;
    r->touch();
    if (nonces) HIPCHK(c, hipMemcpy(r->nonces.p, nonces, 16 * n, hipMemcpyHostToDevice));
    if (pub) HIPCHK(c, hipMemcpy(r->pub.p, pub, (size_t)mc_public_share_size(p) * n, hipMemcpyHostToDevice));
    if (in0) {
        if (!r->in0.ensure((size_t)mc_input_share_size(p, 0) * n)) return fail(c, MASTIC_ENOMEM, "out of device memory");
        HIPCHK(c, hipMemcpy(r->in0.p, in0, (size_t)mc_input_share_size(p, 0) * n, hipMemcpyHostToDevice));
    }
    if (in1) {
        if (!r->in1.ensure((size_t)mc_input_share_size(p, 1) * n)) return fail(c, MASTIC_ENOMEM, "out of device memory");
        HIPCHK(c, hipMemcpy(r->in1.p, in1, (size_t)mc_input_share_size(p, 1) * n, hipMemcpyHostToDevice));
    }
    return validate_wire(c, r, pub != nullptr, in0 != nullptr);
}

extern "C" int mastic_reports_download(mastic_reports* r, uint8_t* nonces, uint8_t* pub, uint8_t* in0, uint8_t* in1) {
    DeviceScope ds_(r ? r->ctx : nullptr);
    if (!r) return MASTIC_EINVAL;
    mastic_ctx* c = r->ctx;
    const McParams& p = c->p;
    const size_t n = r->n;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nonces) HIPCHK(c, hipMemcpy(nonces, r->nonces.p, 16 * n, hipMemcpyDeviceToHost));
    if (pub) HIPCHK(c, hipMemcpy(pub, r->pub.p, (size_t)mc_public_share_size(p) * n, hipMemcpyDeviceToHost));
    if (in0) {
        if (!r->in0.p) return fail(c, MASTIC_EINVAL, "no leader input shares");
        HIPCHK(c, hipMemcpy(in0, r->in0.p, (size_t)mc_input_share_size(p, 0) * n, hipMemcpyDeviceToHost));
    }
    if (in1) {
        if (!r->in1.p) return fail(c, MASTIC_EINVAL, "no helper input shares");
        HIPCHK(c, hipMemcpy(in1, r->in1.p, (size_t)mc_input_share_size(p, 1) * n, hipMemcpyDeviceToHost));
    }
    return 0;
}

template <class F>
static int shard_impl(mastic_ctx* c, mastic_reports* rep, const uint8_t* alphas, const uint8_t* betas,
                      const uint8_t* nonces, const uint8_t* rands) {
    typedef typename F::E E;
    const McParams& p = c->p;
    const size_t n = rep->n;
    const size_t ab = (p.bits + 7) / 8, bsz = (size_t)p.meas_len * p.enc, rs = mc_rand_size(p);
    if (!rep->in0.ensure((size_t)mc_input_share_size(p, 0) * n) || !rep->in1.ensure((size_t)mc_input_share_size(p, 1) * n))
        return fail(c, MASTIC_ENOMEM, "out of device memory (input shares)");
    DevBuf da, db, dr, tab;
    if (!da.ensure(ab * n) || !db.ensure(bsz * n) || !dr.ensure(rs * n) || !tab.ensure(sizeof(E) * p.P))
        return fail(c, MASTIC_ENOMEM, "out of device memory (shard inputs)");
    HIPCHK(c, hipMemcpy(da.p, alphas, ab * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(db.p, betas, bsz * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dr.p, rands, rs * n, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(rep->nonces.p, nonces, 16 * n, hipMemcpyHostToDevice));
    FlpConsts<F> fc = flp_consts<F>(p);
    const std::vector<E> pows = flp_alpha_inv_pows<F>(fc, p.P);
    HIPCHK(c, hipMemcpy(tab.p, pows.data(), sizeof(E) * p.P, hipMemcpyHostToDevice));
    // scratch planes per report
    const size_t wl = (size_t)p.value_len * p.w32;
    const size_t words = wl + 88 + 2 * wl + (size_t)std::max(1, p.joint_rand_len) * p.w32 + (size_t)p.arity * p.w32 +
                         2 * (size_t)p.arity * p.P * p.w32 + 2 * (size_t)p.proof_len * p.w32 + 32;
    const uint64_t budget = default_budget(c);
    size_t chunk = std::min<size_t>(round_up(n, 64), std::max<size_t>(64, (budget / (words * 4)) / 64 * 64));
    // the scratch is the ctx's work arena (kept across calls, stream-ordered
    // after earlier prep_inits): sharding a large batch leaves the arena that
    // its prep_inits then reuse instead of freeing it and allocating again
    // (large hipMallocs / hipFrees cost ~1 s per 50-100 GB on MI355X)
    DevBuf& scratch = c->work;
    c->rk.valid = false;  // the scratch overwrites the arena's key-schedule planes
    if (!scratch.ensure(words * 4 * chunk)) return fail(c, MASTIC_ENOMEM, "out of device memory (shard scratch)");
    for (size_t b = 0; b < n; b += chunk) {
        const int nn = (int)std::min(chunk, n - b);
        const int S = (int)round_up(nn, 64);
        ShardArgs a;
        a.n = nn;
        a.stride = S;
        a.alphas = da.as<uint8_t>() + ab * b;
        a.betas = db.as<uint8_t>() + bsz * b;
        a.nonces = rep->nonces.as<uint8_t>() + 16 * b;
        a.rands = dr.as<uint8_t>() + rs * b;
        a.pub = rep->pub.as<uint8_t>() + (size_t)mc_public_share_size(p) * b;
        a.in0 = rep->in0.as<uint8_t>() + (size_t)mc_input_share_size(p, 0) * b;
        a.in1 = rep->in1.as<uint8_t>() + (size_t)mc_input_share_size(p, 1) * b;
        uint32_t* w = scratch.as<uint32_t>();
        size_t o = 0;
        auto take = [&](size_t k) {
            uint32_t* r = w + o * S;
            o += k;
            return r;
        };
        a.beta = take(wl);
        a.rke = take(44);
        a.rkc = take(44);
        a.bs = take(2 * wl);
        a.jr = take((size_t)std::max(1, p.joint_rand_len) * p.w32);
        a.prand = take((size_t)p.arity * p.w32);
        a.vals = take((size_t)p.arity * p.P * p.w32);
        a.coef = take((size_t)p.arity * p.P * p.w32);
        a.proof = take((size_t)p.proof_len * p.w32);
        a.hps = take((size_t)p.proof_len * p.w32);
        a.misc = take(32);
        hipLaunchKernelGGL(k_shard<F>, dim3((nn + 255) / 256), dim3(256), 0, c->stream, p, a,
                           (const PrefixState*)c->pfx.p, fc, tab.as<E>());
        HIPCHK(c, hipGetLastError());
    }
    if (int rc = validate_wire(c, rep, true, true)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

extern "C" int mastic_reports_shard(mastic_reports* rep, const uint8_t* app_ctx, size_t ctx_len,
                                    const uint8_t* alphas, const uint8_t* betas, const uint8_t* nonces,
                                    const uint8_t* rands) {
    DeviceScope ds_(rep ? rep->ctx : nullptr);
    if (!rep) return MASTIC_EINVAL;
    mastic_ctx* c = rep->ctx;
    rep->touch();
    if (rep->n == 0) {
        // an empty batch holds both aggregators' (zero) input shares, so that
        // prep_init accepts it and its views (e.g. a rank of a split job that
        // gets no reports)
        if (!rep->in0.ensure(0) || !rep->in1.ensure(0)) return fail(c, MASTIC_ENOMEM, "out of device memory");
        return 0;
    }
    if (!alphas || !nonces || !rands || (!betas && c->p.meas_len > 0)) return fail(c, MASTIC_EINVAL, "null input");
    int rc = build_prefixes(c, app_ctx, ctx_len, nullptr, 0);
    if (rc) return rc;
    return with_field(c->p, [&](auto f) {
        return shard_impl<typename decltype(f)::type>(c, rep, alphas, betas, nonces, rands);
    });
}

extern "C" int mastic_shard_batch(mastic_ctx* c, const uint8_t* app_ctx, size_t ctx_len, size_t n,
                                  const uint8_t* alphas, const uint8_t* betas, const uint8_t* nonces,
                                  const uint8_t* rands, uint8_t* pub_out, uint8_t* in0_out, uint8_t* in1_out) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    mastic_reports* rep = nullptr;
    int rc = mastic_reports_create(c, n, &rep);
    if (rc) return rc;
    rc = mastic_reports_shard(rep, app_ctx, ctx_len, alphas, betas, nonces, rands);
    if (!rc) rc = mastic_reports_download(rep, nullptr, pub_out, in0_out, in1_out);
    mastic_reports_destroy(rep);
    return rc;
}

// ---------------------------------------------------------------- compaction
// mastic_reports_compact: the plan is compact_plan.hpp, the kernel
// rows_kernels.hpp.  Everything runs on the ctx's main stream.  That orders it
// after every queued reader of the batch's buffers, because all of them run
// there: k_unpack, k_rows_to_planes and k_validate_wire (Chunk::unpack and
// validate_wire launch on c->stream whatever stream the chunk's sponges use),
// k_shard and the replay set's kernels.  Streams 2 to 4 run binder sponges and
// the FLP query, which read the work arena only, so no event is needed.
static int compact_segment(mastic_ctx* c, uint8_t* seg, size_t rb, const CompactIndex& ix, const uint32_t* d_idx,
                           uint8_t* stage, size_t stage_bytes) {
    const size_t S = compact_stage_rows(stage_bytes, rb);
    for (const CompactLaunch& l : compact_launches(ix, S)) {
        if (l.op == CP_COPY_BACK) {
            HIPCHK(c, hipMemcpyAsync(seg + l.first * rb, stage, l.count * rb, hipMemcpyDeviceToDevice, c->stream));
            continue;
        }
        uint8_t* dst = l.op == CP_GATHER_STAGE ? stage : seg + l.first * rb;
        // (one launch's grid.x is bounded; a tile above it goes out in pieces, in order)
        const size_t piece = std::max<size_t>(1, (size_t)(ROWS_MAX_GRID * ROWS_THREADS / rows_slots_per_row(rb)));
        for (size_t o = 0; o < l.count; o += piece) {
            const size_t cnt = std::min(piece, l.count - o);
            hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)rows_grid(rb, cnt)), dim3(ROWS_THREADS), 0, c->stream,
                               (const uint8_t*)seg, dst + o * rb, rb, d_idx, l.first + o, cnt, rows_slots_per_row(rb));
            HIPCHK(c, hipGetLastError());
        }
    }
    return 0;
}

extern "C" int mastic_reports_compact(mastic_reports* rep, const uint8_t* keep, size_t staging_bytes, size_t* n_kept) {
    DeviceScope ds_(rep ? rep->ctx : nullptr);
    if (!rep) return MASTIC_EINVAL;
    mastic_ctx* c = rep->ctx;
    if (!rep->nonces.own || !rep->pub.own || !rep->wire_flags.own)
        return fail(c, MASTIC_EINVAL, "compact: the batch is a view (compact the batch that owns the memory)");
    if (!keep) return fail(c, MASTIC_EINVAL, "compact: null keep mask");
    if (rep->n > 0xffffffffull) return fail(c, MASTIC_EINVAL, "compact: too many reports");
    const CompactIndex ix = compact_index(keep, rep->n);
    if (n_kept) *n_kept = ix.n_kept;
    if (ix.n_kept == rep->n) return 0;  // nothing dropped: same contents, same generation
    if (ix.moved() > 0) {
        const McParams& p = c->p;
        struct Seg {
            DevBuf* b;
            size_t rb;
        } segs[5] = {{&rep->nonces, 16},
                     {&rep->pub, (size_t)mc_public_share_size(p)},
                     {&rep->in0, (size_t)mc_input_share_size(p, 0)},
                     {&rep->in1, (size_t)mc_input_share_size(p, 1)},
                     {&rep->wire_flags, 1}};
        size_t widest = 0;
        for (const Seg& s : segs)
            if (s.b->p) widest = std::max(widest, s.rb);
        const size_t sb = compact_staging_bytes(staging_bytes, widest, ix.moved());
        // both allocations before any row moves: MASTIC_ENOMEM leaves the batch as it was
        DevBuf d_idx, stage;
        if (c->inject_alloc_failure() || !d_idx.ensure(4 * ix.n_kept) || !stage.ensure(sb))
            return fail(c, MASTIC_ENOMEM, "out of device memory (compact: %zu B staging, %zu B index)", sb,
                        4 * ix.n_kept);
        int rc = 0;
        if (hipMemcpyAsync(d_idx.p, ix.src.data(), 4 * ix.n_kept, hipMemcpyHostToDevice, c->stream) != hipSuccess)
            rc = fail(c, MASTIC_EHIP, "compact: the index upload failed");
        for (const Seg& s : segs)
            if (!rc && s.b->p)
                rc = compact_segment(c, s.b->as<uint8_t>(), s.rb, ix, d_idx.as<uint32_t>(), stage.as<uint8_t>(), sb);
        // (also on failure: the index and the staging buffer are freed on return)
        if (hipStreamSynchronize(c->stream) != hipSuccess && !rc)
            rc = fail(c, MASTIC_EHIP, "compact: the row moves failed; the batch must be uploaded again");
        if (rc) {
            rep->touch();
            return rc;
        }
    }
    rep->touch();
    rep->n = ix.n_kept;
    return 0;
}
