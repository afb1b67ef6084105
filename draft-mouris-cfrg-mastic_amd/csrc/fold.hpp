// The folds of out shares into agg shares.  Every decision (chunks, passes, copies, sizes, the group id
// check) is group_fold.hpp's; this file allocates, copies and launches.  Staging: mastic_ctx::fold.
#pragma once
// Fold of the out shares of the last prep_init of agg_id into dagg (device).
static int aggregate_impl(mastic_ctx* c, int agg_id, const uint8_t* valid, uint32_t* dagg) {
    Result& R = c->res[agg_id];
    const McParams& p = c->p;
    const size_t rows = agg_rows(p, R);
    const uint8_t* dv = nullptr;
    if (valid && R.n) {
        if (!c->fold.valid.grow(R.n)) return fail(c, MASTIC_ENOMEM, "out of device memory");
        HIPCHK(c, hipMemcpyAsync(c->fold.valid.p, valid, R.n, hipMemcpyHostToDevice, c->stream));
        dv = c->fold.valid.as<uint8_t>();
    }
    if (!rows) return 0;
    const FoldPlan pl = plan_fold(p.w32, R.n, rows, c->k.n_cus);
    uint32_t* dst = dagg;
    if (pl.chunks > 1) {
        if (!c->fold.part.ensure(pl.partial_bytes)) return fail(c, MASTIC_ENOMEM, "out of device memory");
        dst = c->fold.part.as<uint32_t>();
    }
    with_field(p, [&](auto f) {
        using F = typename decltype(f)::type;
        hipLaunchKernelGGL(k_fold<F>, dim3((unsigned)rows, (unsigned)pl.chunks), dim3(256), 0, c->stream,
                           R.out.as<uint32_t>(), (int)R.n, (int)R.stride, dv, (int)pl.chunk, dst);
    });
    HIPCHK(c, hipGetLastError());
    return pl.chunks > 1 ? launch_fold_shares(c, dst, pl.chunks, rows, dagg) : 0;
}

extern "C" int mastic_aggregate(mastic_ctx* c, int agg_id, const uint8_t* valid, uint8_t* agg_share) {
    DeviceScope ds_(c);
    const Result* const R = ready_result(c, agg_id);
    if (!R) return MASTIC_EINVAL;
    const McParams& p = c->p;
    const size_t rows = agg_rows(p, *R);
    if (!c->fold.out.grow(std::max<size_t>(rows, 1) * p.w32 * 4)) return fail(c, MASTIC_ENOMEM, "out of device memory");
    int rc = aggregate_impl(c, agg_id, valid, c->fold.out.as<uint32_t>());
    if (rc) return rc;
    if (agg_share && rows)
        HIPCHK(c, hipMemcpyAsync(agg_share, c->fold.out.p, rows * p.w32 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// (ABI 6: the only name of this function; mastic_aggregate_device, whose
// argument count changed between ABI 3, 4 and 5, is gone)
extern "C" int mastic_aggregate_device_on_stream(mastic_ctx* c, int agg_id, const uint8_t* valid,
                                                 void* dev_agg_share, void* caller_stream) {
    DeviceScope ds_(c);
    const Result* const R = ready_result(c, agg_id);
    if (!R) return MASTIC_EINVAL;
    if (agg_rows(c->p, *R) && !dev_agg_share) return fail(c, MASTIC_EINVAL, "null agg share buffer");
    // the buffer may have been allocated / filled by work queued on the
    // caller's stream (e.g. a torch allocation's fill): the fold writes it
    // only after that work
    int rc = order_after(c, caller_stream);
    if (!rc) rc = aggregate_impl(c, agg_id, valid, (uint32_t*)dev_agg_share);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's stream (e.g. RCCL's) reads it next
    return 0;
}

// One agg share per batch bucket in one pass over the out shares.  Every
// decision (the id check, passes, copies, chunks, sizes) is group_fold.hpp's.
extern "C" int mastic_aggregate_grouped(mastic_ctx* c, int agg_id, const uint32_t* group, size_t n_groups,
                                        const uint8_t* valid, uint8_t* agg_shares, uint64_t* counts) {
    DeviceScope ds_(c);
    const Result* const Rp = ready_result(c, agg_id);
    if (!Rp) return MASTIC_EINVAL;
    const Result& R = *Rp;
    const McParams& p = c->p;
    const size_t n = R.n;
    const size_t rows = agg_rows(p, R);
    if (n_groups == 0 || n_groups > MASTIC_MAX_GROUPS)
        return fail(c, MASTIC_EINVAL, "n_groups must be 1 .. %d", MASTIC_MAX_GROUPS);
    if (n_groups * rows > (size_t)INT_MAX) return fail(c, MASTIC_EINVAL, "n_groups * rows exceeds INT_MAX");
    if (n && !group) return fail(c, MASTIC_EINVAL, "null group ids");
    if (rows && !agg_shares) return fail(c, MASTIC_EINVAL, "null agg shares buffer");
    std::vector<uint64_t> cnt(n_groups);
    const long long bad = check_groups(group, n, n_groups, valid, cnt.data());
    if (bad >= 0)
        return fail(c, MASTIC_EINVAL, "report %lld: group id %u is not below n_groups = %zu", bad, group[bad], n_groups);
    const GroupFoldPlan pl = plan_group_fold(p.w32, n, rows, n_groups, c->k.n_cus, 0, 0);
    const size_t out_bytes = n_groups * rows * p.w32 * 4;
    if (rows) {
        // all device memory first (each allocation takes the fail_allocs hook):
        // nothing is launched before the last of them succeeded
        auto alloc = [&](DevBuf& b, size_t bytes) { return !c->inject_alloc_failure() && b.grow(bytes); };
        if ((n && !alloc(c->fold.grp_ids, n * 4)) || (n && valid && !alloc(c->fold.valid, n)) ||
            (pl.partial_bytes && !alloc(c->fold.grp_part, pl.partial_bytes)) || !alloc(c->fold.grp_out, out_bytes))
            return fail(c, MASTIC_ENOMEM, "out of device memory (grouped fold)");
        uint32_t* stage = c->fold.grp_out.as<uint32_t>();
        if (pl.chunks == 0) {
            HIPCHK(c, hipMemsetAsync(stage, 0, out_bytes, c->stream));
        } else {
            const uint8_t* dv = nullptr;
            HIPCHK(c, hipMemcpyAsync(c->fold.grp_ids.p, group, n * 4, hipMemcpyHostToDevice, c->stream));
            if (valid) {
                HIPCHK(c, hipMemcpyAsync(c->fold.valid.p, valid, n, hipMemcpyHostToDevice, c->stream));
                dv = c->fold.valid.as<uint8_t>();
            }
            const dim3 grid(pl.grid_x, pl.grid_y);
            for (uint32_t k = 0; k < pl.passes; k++) {
                const uint32_t g0 = k * pl.groups_per_pass;
                const uint32_t gpp = std::min<uint32_t>(pl.groups_per_pass, (uint32_t)n_groups - g0);
                uint32_t* dst = stage + (size_t)g0 * rows * p.w32;
                uint32_t* part = pl.chunks > 1 ? c->fold.grp_part.as<uint32_t>() : dst;
                with_field(p, [&](auto f) {
                    using F = typename decltype(f)::type;
                    hipLaunchKernelGGL(k_fold_grouped<F>, grid, dim3(256), pl.lds_bytes, c->stream,
                                       R.out.as<uint32_t>(), (int)n, (int)R.stride, c->fold.grp_ids.as<uint32_t>(), dv,
                                       (int)pl.chunk, g0, (int)gpp, (int)pl.copies, part);
                });
                HIPCHK(c, hipGetLastError());
                if (pl.chunks > 1)
                    if (int rc = launch_fold_shares(c, part, pl.chunks, (size_t)gpp * rows, dst)) return rc;
            }
        }
        HIPCHK(c, hipMemcpyAsync(agg_shares, stage, out_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (counts) std::copy(cnt.begin(), cnt.end(), counts);
    return 0;
}

extern "C" int mastic_fold_shares(mastic_ctx* c, const void* dev_shares, size_t n_shares, size_t n_elems,
                                  void* dev_out, void* producer_stream) {
    DeviceScope ds_(c);
    if (!c || (!dev_shares && n_shares) || !dev_out) return MASTIC_EINVAL;
    if (n_elems == 0) return 0;
    // the shares were written on the caller's stream (e.g. an RCCL all-gather):
    // order the fold after that stream's work
    int rc = order_after(c, producer_stream);
    if (!rc) rc = launch_fold_shares(c, (const uint32_t*)dev_shares, n_shares, n_elems, (uint32_t*)dev_out);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
