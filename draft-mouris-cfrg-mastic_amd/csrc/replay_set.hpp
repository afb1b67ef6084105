#pragma once
// ---------------------------------------------------------------- replay set
// The nonces an aggregator has admitted, in HBM (nonce_set.hpp: layout, hash
// and sizing rules; nonce_set_kernels.hpp: the kernels).  Every call blocks,
// runs on the ctx's main stream and leaves the table holding arena ids only.
struct mastic_nonce_set {
    mastic_ctx* ctx = nullptr;
    NsHashKey hk{};
    uint64_t count = 0;       // keys in the arena
    uint64_t slots = 0;       // of `table`
    uint64_t arena_keys = 0;  // capacity of `arena`
    bool broken = false;      // a probe came full circle or a launch failed mid-admit: every later call fails
    DevBuf table, arena;
    DevBuf words;             // NS_WORDS words: error flag, fresh counter
    DevBuf stage;             // the host nonces of an admit / query
    DevBuf fresh, slot_of;    // per nonce of the batch (resolve -> commit)
    NsTable dev(const DevBuf& t, const DevBuf& a, uint64_t nslots) const {
        return NsTable{t.as<uint32_t>(), a.as<uint4>(), (uint32_t)nslots, (uint32_t)count, hk};
    }
};

// Every allocation of a set takes the ctx's allocation-failure hook
// (mastic_set_test_hooks); one that is large enough already is none.
static bool ns_alloc(mastic_ctx* c, DevBuf& b, size_t want) {
    if (want <= b.bytes && b.p) return true;
    return !c->inject_alloc_failure() && b.ensure(want);
}

static int ns_broken(mastic_nonce_set* s, const char* what) {
    s->broken = true;
    (void)hipStreamSynchronize(s->ctx->stream);
    return fail(s->ctx, MASTIC_EHIP, "nonce set: %s; the set is unusable", what);
}

// Make the table and the arena fit `keys` keys (the growth rules of
// nonce_set.hpp).  Both new buffers are allocated before anything is touched,
// so MASTIC_ENOMEM leaves the set as it was; the old ones are dropped once the
// copy and the rehash that read them are done.
static int ns_reserve(mastic_nonce_set* s, uint64_t keys) {
    mastic_ctx* c = s->ctx;
    const uint64_t slots = ns_grown_slots(s->slots, keys);
    const uint64_t cap = ns_grown_arena(s->arena_keys, slots, keys);
    if (slots == s->slots && cap == s->arena_keys) return 0;
    DevBuf table, arena;
    if ((slots != s->slots && !ns_alloc(c, table, 4 * slots)) || (cap != s->arena_keys && !ns_alloc(c, arena, 16 * cap)))
        return fail(c, MASTIC_ENOMEM, "out of device memory (nonce set of %llu keys)", (unsigned long long)keys);
    uint32_t w[NS_WORDS] = {};
    if (arena.p && s->count)
        HIPCHK(c, hipMemcpyAsync(arena.p, s->arena.p, 16 * s->count, hipMemcpyDeviceToDevice, c->stream));
    if (table.p) {
        HIPCHK(c, hipMemsetAsync(table.p, 0, 4 * slots, c->stream));
        if (s->count) {
            HIPCHK(c, hipMemsetAsync(s->words.p, 0, 4 * NS_WORDS, c->stream));
            hipLaunchKernelGGL(k_ns_rehash, dim3((unsigned)((s->count + 255) / 256)), dim3(256), 0, c->stream,
                               s->dev(table, arena.p ? arena : s->arena, slots), (uint32_t)s->count,
                               s->words.as<uint32_t>());
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(w, s->words.p, sizeof w, hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (w[NS_ERR]) return ns_broken(s, "a rehash probe came full circle");
    if (table.p) {
        s->table.swap(table);
        s->slots = slots;
    }
    if (arena.p) {
        s->arena.swap(arena);
        s->arena_keys = cap;
    }
    return 0;
}

// Admit the n nonces at d_batch (device memory, 16-byte aligned).
static int ns_admit(mastic_nonce_set* s, const uint4* d_batch, size_t n, uint8_t* fresh_out, size_t* n_fresh) {
    mastic_ctx* c = s->ctx;
    if (n_fresh) *n_fresh = 0;
    if (n == 0) return 0;
    if (n > NS_MAX_KEYS || s->count + n > NS_MAX_KEYS) return fail(c, MASTIC_EINVAL, "nonce set: too many nonces");
    // all growth (table, arena, rehash, scratch) before the first insert: a failure
    // here leaves the set's contents as they were (at most its buffers larger)
    int rc = ns_reserve(s, s->count + n);
    if (rc) return rc;
    if (!ns_alloc(c, s->fresh, n) || !ns_alloc(c, s->slot_of, 4 * n))
        return fail(c, MASTIC_ENOMEM, "out of device memory (nonce set scratch for %zu nonces)", n);
    const dim3 grid((unsigned)((n + 255) / 256));
    const NsTable t = s->dev(s->table, s->arena, s->slots);
    uint32_t* words = s->words.as<uint32_t>();
    uint32_t w[NS_WORDS] = {};
    HIPCHK(c, hipMemsetAsync(words, 0, 4 * NS_WORDS, c->stream));
    hipLaunchKernelGGL(k_ns_insert, grid, dim3(256), 0, c->stream, t, d_batch, (uint32_t)n, words);
    hipLaunchKernelGGL(k_ns_resolve, grid, dim3(256), 0, c->stream, t, d_batch, (const uint4*)nullptr, (uint32_t)n,
                       s->fresh.as<uint8_t>(), s->slot_of.as<uint32_t>(), words);
    hipLaunchKernelGGL(k_ns_commit, grid, dim3(256), 0, c->stream, s->table.as<uint32_t>(), s->arena.as<uint4>(),
                       (uint32_t)s->count, d_batch, (uint32_t)n, s->fresh.as<uint8_t>(), s->slot_of.as<uint32_t>(),
                       words);
    // from the first launch on the table may hold batch ids: a failure leaves no usable set
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(w, words, sizeof w, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        (fresh_out && hipMemcpyAsync(fresh_out, s->fresh.p, n, hipMemcpyDeviceToHost, c->stream) != hipSuccess) ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return ns_broken(s, "an admit's launches failed");
    if (w[NS_ERR] || w[NS_FRESH] > n) return ns_broken(s, "an admit's probe came full circle");
    s->count += w[NS_FRESH];
    if (n_fresh) *n_fresh = w[NS_FRESH];
    return 0;
}

// The host nonces of an admit / query, copied to the set's staging buffer.
static int ns_stage(mastic_nonce_set* s, const uint8_t* nonces, size_t n) {
    mastic_ctx* c = s->ctx;
    if (!nonces) return fail(c, MASTIC_EINVAL, "nonce set: null nonces");
    if (n > NS_MAX_KEYS) return fail(c, MASTIC_EINVAL, "nonce set: too many nonces");
    if (!ns_alloc(c, s->stage, 16 * n)) return fail(c, MASTIC_ENOMEM, "out of device memory (nonce staging)");
    HIPCHK(c, hipMemcpy(s->stage.p, nonces, 16 * n, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int mastic_nonce_set_create(mastic_ctx* c, size_t capacity_hint, const uint8_t hash_key[16],
                                       mastic_nonce_set** out) {
    DeviceScope ds_(c);
    if (!c || !out) return MASTIC_EINVAL;
    *out = nullptr;
    if (capacity_hint > NS_MAX_KEYS) return fail(c, MASTIC_EINVAL, "nonce set: capacity hint too large");
    uint8_t key[16];
    if (hash_key)
        memcpy(key, hash_key, 16);
    else if (getentropy(key, sizeof key) != 0)
        return fail(c, MASTIC_EHIP, "nonce set: no entropy for the hash key");
    std::unique_ptr<mastic_nonce_set> s(new mastic_nonce_set());
    s->ctx = c;
    memcpy(&s->hk.k0, key, 8);
    memcpy(&s->hk.k1, key + 8, 8);
    if (!ns_alloc(c, s->words, 4 * NS_WORDS)) return fail(c, MASTIC_ENOMEM, "out of device memory (nonce set)");
    const int rc = ns_reserve(s.get(), capacity_hint);
    if (rc) return rc;
    *out = s.release();
    return 0;
}

extern "C" void mastic_nonce_set_destroy(mastic_nonce_set* s) {
    DeviceScope ds_(s ? s->ctx : nullptr);
    if (!s) return;
    (void)hipStreamSynchronize(s->ctx->stream);
    delete s;
}

extern "C" size_t mastic_nonce_set_count(const mastic_nonce_set* s) { return s ? (size_t)s->count : 0; }

#define NS_USABLE(s)                                                                                      \
    do {                                                                                                  \
        if (!(s)) return MASTIC_EINVAL;                                                                   \
        if ((s)->broken) return fail((s)->ctx, MASTIC_EHIP, "nonce set: unusable after an earlier failure"); \
    } while (0)

extern "C" int mastic_nonce_set_admit(mastic_nonce_set* s, const uint8_t* nonces, size_t n, uint8_t* fresh_out,
                                      size_t* n_fresh) {
    DeviceScope ds_(s ? s->ctx : nullptr);
    NS_USABLE(s);
    if (n == 0) return ns_admit(s, nullptr, 0, fresh_out, n_fresh);
    const int rc = ns_stage(s, nonces, n);
    return rc ? rc : ns_admit(s, s->stage.as<uint4>(), n, fresh_out, n_fresh);
}

extern "C" int mastic_nonce_set_admit_reports(mastic_nonce_set* s, mastic_reports* rep, uint8_t* fresh_out,
                                              size_t* n_fresh) {
    DeviceScope ds_(s ? s->ctx : nullptr);
    NS_USABLE(s);
    if (!rep || rep->ctx != s->ctx) return fail(s->ctx, MASTIC_EINVAL, "nonce set: the reports belong to another ctx");
    return ns_admit(s, rep->nonces.as<uint4>(), rep->n, fresh_out, n_fresh);
}

extern "C" int mastic_nonce_set_contains(mastic_nonce_set* s, const uint8_t* nonces, size_t n, uint8_t* found_out) {
    DeviceScope ds_(s ? s->ctx : nullptr);
    NS_USABLE(s);
    if (n == 0) return 0;
    mastic_ctx* c = s->ctx;
    if (!found_out) return fail(c, MASTIC_EINVAL, "nonce set: null output");
    int rc = ns_stage(s, nonces, n);
    if (rc) return rc;
    if (!ns_alloc(c, s->fresh, n)) return fail(c, MASTIC_ENOMEM, "out of device memory (nonce set scratch)");
    uint32_t w[NS_WORDS] = {};
    HIPCHK(c, hipMemsetAsync(s->words.p, 0, 4 * NS_WORDS, c->stream));
    hipLaunchKernelGGL(k_ns_resolve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       s->dev(s->table, s->arena, s->slots), (const uint4*)nullptr, s->stage.as<uint4>(), (uint32_t)n,
                       s->fresh.as<uint8_t>(), (uint32_t*)nullptr, s->words.as<uint32_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(w, s->words.p, sizeof w, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(found_out, s->fresh.p, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (w[NS_ERR]) return ns_broken(s, "a query's probe came full circle");
    return 0;
}

extern "C" int mastic_nonce_set_export(mastic_nonce_set* s, uint8_t* nonces_out, size_t capacity, size_t* n_out) {
    DeviceScope ds_(s ? s->ctx : nullptr);
    NS_USABLE(s);
    mastic_ctx* c = s->ctx;
    if (n_out) *n_out = (size_t)s->count;
    if (capacity < s->count) return fail(c, MASTIC_EINVAL, "nonce set: export buffer too small");
    if (s->count == 0) return 0;
    if (!nonces_out) return fail(c, MASTIC_EINVAL, "nonce set: null output");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(nonces_out, s->arena.p, 16 * s->count, hipMemcpyDeviceToHost));
    return 0;
}
