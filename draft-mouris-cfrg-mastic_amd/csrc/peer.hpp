// One aggregator of two: mastic_decide_peer, the decide of this aggregator's
// result in HBM against the other aggregator's prep shares from the wire
// (decide_kernels.hpp k_decide_peer).  The messages that carry those shares
// and the round's state machine are Python's (mastic_amd/aggregator.py).
#pragma once

constexpr bool DECIDE_PEER_USE_LDS = true;

// How k_decide_peer reads the peer's rows: through LDS where a workgroup's 256
// rows fit, i.e. up to DECIDE_PEER_LDS_WORDS words (252 bytes); wider rows
// always take the per-lane loads (DESIGN.md "Deciding against a peer" has the
// measurement of both, the wide rows included).
static bool decide_peer_lds(size_t psz) {
#ifdef MASTIC_EXPERIMENT_KNOBS
    if (const char* e = getenv("MASTIC_DECIDE_PEER_LDS"))
        return e[0] != '0' && psz / 4 <= (size_t)DECIDE_PEER_LDS_WORDS;
#endif
    return DECIDE_PEER_USE_LDS && psz / 4 <= (size_t)DECIDE_PEER_LDS_WORDS;
}

extern "C" int mastic_decide_peer(mastic_ctx* c, int agg_id, const uint8_t* app_ctx, size_t ctx_len,
                                  const uint8_t* peer_prep_shares, const uint8_t* peer_ok, size_t n,
                                  uint8_t* accept_out, uint8_t* decide_out, uint8_t* prep_msgs_out) {
    DeviceScope ds_(c);
    Result* const Rp = ready_result(c, agg_id);
    if (!Rp) return MASTIC_EINVAL;
    const Result& R = *Rp;
    if (n != R.n) return fail(c, MASTIC_EINVAL, "the peer's prep shares are for %zu reports, the result has %zu", n, R.n);
    if (n == 0) return 0;
    if (!peer_prep_shares) return fail(c, MASTIC_EINVAL, "no peer prep shares");
    int rc = build_prefixes(c, app_ctx, ctx_len, nullptr, 0);
    if (rc) return rc;
    const McParams& p = c->p;
    const size_t S = R.stride, psz = mc_prep_share_size(p, R.weight_check);
    const bool check_jr = R.weight_check && p.joint_rand_len > 0;
    // staging: prep messages (16-byte aligned rows) | peer rows (8-byte aligned) | peer_ok | code | accept | FLP scratch planes
    const size_t need = 32 * n + n * psz + 3 * n + 256 + S * 4 * (size_t)std::max(1, p.verifier_len * p.w32);
    if (!c->stage.grow(need)) return fail(c, MASTIC_ENOMEM, "out of device memory (decide staging)");
    uint8_t* msg = c->stage.as<uint8_t>();
    uint8_t* rows = msg + 32 * n;
    uint8_t* ok = rows + n * psz;
    uint8_t* code = ok + n;
    uint8_t* acc = code + n;
    uint32_t* ver = (uint32_t*)(((uintptr_t)(acc + n) + 255) & ~(uintptr_t)255);
    HIPCHK(c, hipMemcpyAsync(rows, peer_prep_shares, n * psz, hipMemcpyHostToDevice, c->stream));
    if (peer_ok) HIPCHK(c, hipMemcpyAsync(ok, peer_ok, n, hipMemcpyHostToDevice, c->stream));
    const PeerOwn own{R.eval_proof.as<uint32_t>(), R.jr_part.as<uint32_t>(), R.verifier.as<uint32_t>(),
                      R.jr_seed.as<uint32_t>(), (const int32_t*)R.status.p};
    const bool lds = decide_peer_lds(psz);
    const size_t lds_bytes = lds ? (size_t)256 * decide_peer_pitch((int)(psz / 4)) * 4 : 0;
    with_field(p, [&](auto f) {
        using F = typename decltype(f)::type;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), lds_bytes, c->stream, p, (int)n,
                               (int)S, R.weight_check, agg_id, own, (const uint8_t*)rows, (int)psz,
                               (const uint8_t*)(peer_ok ? ok : nullptr), ver, (const PrefixState*)c->pfx.p, msg, code,
                               acc);
        };
        if (lds)
            launch(k_decide_peer<F, true>);
        else
            launch(k_decide_peer<F, false>);
    });
    HIPCHK(c, hipGetLastError());
    if (accept_out) HIPCHK(c, hipMemcpyAsync(accept_out, acc, n, hipMemcpyDeviceToHost, c->stream));
    if (decide_out) HIPCHK(c, hipMemcpyAsync(decide_out, code, n, hipMemcpyDeviceToHost, c->stream));
    if (prep_msgs_out && check_jr) HIPCHK(c, hipMemcpyAsync(prep_msgs_out, msg, 32 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->bury();
    return 0;
}
