// Host side of the MI355X Mastic aggregator, the C ABI of include/mastic_hip.h:
// the library's one translation unit (every kernel is instantiated once).  No
// CPU compute path exists: every cryptographic operation runs in the kernels
// of the device headers (kernels.hpp is their index; DESIGN.md "Device
// sources") and shard.hpp.  Each subsystem's executor is a header of
// definitions included below, once (DESIGN.md "Host sources" maps them); here
// are the ctx's creation and teardown and the small setters and getters.
#include "mastic_hip.h"

#include <dlfcn.h>
#include <rccl/rccl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <system_error>
#include <thread>
#include <type_traits>
#include <vector>

#include "comm_agree.hpp"
#include "compact_plan.hpp"
#include "host_tree.hpp"
#include "kernels.hpp"
#include "memplan.hpp"
#include "nonce_set_kernels.hpp"
#include "rows_kernels.hpp"
#include "schedule.hpp"
#include "shard.hpp"

static_assert(SCHED_EVAL_WAVES == EVAL_WAVES && SCHED_EVAL_PROOF_WAVES == EVAL_PROOF_WAVES &&
                  SCHED_SPONGE_RATE == KECCAK_RATE,
              "schedule.hpp and the kernels disagree on a shared constant");

#include "ctx.hpp"
#include "prep.hpp"
#include "peer.hpp"
#include "fold.hpp"
#include "comm.hpp"
#include "reports.hpp"
#include "replay_set.hpp"

extern "C" int mastic_synchronize(mastic_ctx* c) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->bury();
    return 0;
}

// ---------------------------------------------------------------- ctx
extern "C" int mastic_ctx_create(const mastic_params* up, mastic_ctx** out) {
    if (!up || !out) return MASTIC_EINVAL;
    *out = nullptr;
    McParams p;
    if (mc_derive((int)up->circuit, (int)up->bits, (int)up->length, (int)up->sum_vec_bits, up->max_measurement,
                  (int)up->chunk_length, &p))
        return MASTIC_EINVAL;
    if (p.bits > TREE_MAX_BITS) return MASTIC_EINVAL;  // node paths are at most 256 bits (host_tree.hpp)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MASTIC_ENODEV;
    if (up->device < 0 || up->device >= ndev) return MASTIC_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, up->device) != hipSuccess) return MASTIC_ENODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return MASTIC_ENODEV;
    if (hipSetDevice(up->device) != hipSuccess) return MASTIC_ENODEV;
    mastic_ctx* c = new mastic_ctx();
    c->user = *up;
    c->p = p;
    c->device = up->device;
    c->k.n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, up->device) == hipSuccess && khz > 0)
            c->wall_khz = khz;
    }
#ifdef MASTIC_EXPERIMENT_KNOBS
    // A/B and timing experiments only (tools/ab_*.sh build the library with
    // -DMASTIC_EXPERIMENT_KNOBS; the shipped library reads none of these):
    // the knobs that are still open and have no mastic_set_* entry point.
    {
        const char* e = getenv("MASTIC_ABSORB_SINGLE");
        if (e) c->k.absorb_mode = e[0] == '1' ? 1 : (e[0] == '2' ? 2 : 0);
        const char* esm = getenv("MASTIC_ABSORB_SINGLE_MIN");
        if (esm) c->k.absorb_single_min = (size_t)std::max(0, atoi(esm));
        const char* spd = getenv("MASTIC_STRIDE_PAD");
        if (spd) c->m.stride_pad = std::max(0, std::min(1 << 20, atoi(spd))) / 64 * 64;
        const char* wa = getenv("MASTIC_WORK_ARENA_GB");
        if (wa) c->m.work_arena = c->m.work_arena_fc = (size_t)std::max(0, atoi(wa)) << 30;
        const char* cp = getenv("MASTIC_CHUNK_PIPELINE");
        if (cp) c->m.chunk_pipeline = cp[0] != '0';
        const char* fp = getenv("MASTIC_FUSE_PROOFS");
        if (fp) c->k.fuse_proofs = atoi(fp) > 0;
        const char* cr = getenv("MASTIC_CHUNK_REPORTS");
        if (cr) c->m.chunk_max = (size_t)std::max(0, atoi(cr));
        const char* spl = getenv("MASTIC_SPLIT_SPONGES");
        if (spl) c->k.split_sponges = spl[0] == '1' ? 1 : 0;
        const char* sgb = getenv("MASTIC_SEG_BALANCE");
        if (sgb) c->k.seg_balance = sgb[0] != '0';
    }
#endif
    // the level kernel's LDS (table + key schedules) is dynamic, above the
    // 64 KiB default: every variant the plan may launch, of both fields
    auto lds = [](const void* fn, int bytes) {
        return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
    };
    bool attrs = true;
    for (int v : LEVEL_VARIANTS)
        attrs = attrs && lds((const void*)level_kernel<F64>(v), EVAL_LDS_BYTES) &&
                lds((const void*)level_kernel<F128>(v), EVAL_LDS_BYTES);
    attrs = attrs && lds((const void*)level_kernel<F64>(LV_FC_PAY), EVAL_LDS_BYTES) &&
            lds((const void*)level_kernel<F128>(LV_FC_PAY), EVAL_LDS_BYTES);
    // the binder sponges are the latency-critical chain: their stream gets the
    // highest priority so their workgroups are dispatched first
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (!attrs || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipStreamCreateWithPriority(&c->stream3, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream4, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return MASTIC_EHIP;
    }
    *out = c;
    return 0;
}

extern "C" void mastic_ctx_destroy(mastic_ctx* c) {
    DeviceScope ds_(c);
    if (!c) return;
    (void)c->idle();
    delete c;
}

extern "C" const char* mastic_last_error(const mastic_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

extern "C" int mastic_set_frontier_cache(mastic_ctx* c, int on, int* last_hit) {
    DeviceScope ds_(c);
    if (!c) return MASTIC_EINVAL;
    if (on >= 0) {
        c->frontier_cache = on != 0;
        if (!on) {
            // queued kernels may still read the cache slots: retire them (freed
            // at the next idle point of the ctx's streams), no synchronisation
            for (auto& x : c->lc) {
                for (DevBuf* b : {&x.sp, &x.rootsum, &x.nd.buf}) c->retire(*b);
                x.release();
            }
            c->retire(c->fc_spare);
        }
    }
    if (last_hit) *last_hit = c->last_hit ? 1 : 0;
    return 0;
}

extern "C" int mastic_set_frontier_cache_nodes(mastic_ctx* c, int mode, int* last_in, int* last_out) {
    if (!c || mode > FC_NODES_AUTO) return MASTIC_EINVAL;
    const int prev = c->fc_nodes;
    // the slots keep their formats (a hit reads either), so the cache stays as it is
    if (mode >= 0) c->fc_nodes = mode;
    if (last_in) *last_in = c->last_nodes_in;
    if (last_out) *last_out = c->last_nodes_out;
    return prev;
}

extern "C" int mastic_set_test_hooks(mastic_ctx* c, int force_slow_blk, int fail_allocs) {
    if (!c) return MASTIC_EINVAL;
    const int pending = c->fail_allocs;
    c->force_slow_blk = force_slow_blk < 0 ? -1 : force_slow_blk;
    c->fail_allocs = std::max(0, fail_allocs);
    return pending;
}

extern "C" int mastic_set_serial_sponges(mastic_ctx* c, int on) {
    if (!c) return MASTIC_EINVAL;
    const int prev = c->serial_sponges ? 1 : 0;
    if (on >= 0) c->serial_sponges = on != 0;
    return prev;
}

extern "C" int mastic_set_last_level_segments(mastic_ctx* c, int k) {
    if (!c || k < 0) return MASTIC_EINVAL;
    const int prev = c->k.last_level_segments;
    c->k.last_level_segments = k;
    return prev;
}

extern "C" int mastic_set_test_sponge_delay(mastic_ctx* c, int delay_us) {
    if (!c || delay_us < 0 || delay_us > 10000000) return MASTIC_EINVAL;
    c->sponge_delay_us = delay_us;
    return 0;
}

extern "C" int mastic_abi_version(void) { return MASTIC_ABI_VERSION; }

extern "C" int mastic_set_memory_budget(mastic_ctx* c, uint64_t bytes) {
    if (!c) return MASTIC_EINVAL;
    c->m.budget = bytes;
    return 0;
}

extern "C" int mastic_get_sizes(const mastic_ctx* c, mastic_sizes* s) {
    if (!c || !s) return MASTIC_EINVAL;
    const McParams& p = c->p;
    s->field_bytes = p.enc;
    s->value_len = p.value_len;
    s->meas_len = p.meas_len;
    s->output_len = p.output_len;
    s->proof_len = p.proof_len;
    s->verifier_len = p.verifier_len;
    s->joint_rand_len = p.joint_rand_len;
    s->query_rand_len = p.query_rand_len;
    s->prove_rand_len = p.prove_rand_len;
    s->rand_size = mc_rand_size(p);
    s->public_share_size = mc_public_share_size(p);
    s->input_share_size[0] = mc_input_share_size(p, 0);
    s->input_share_size[1] = mc_input_share_size(p, 1);
    s->prep_share_size[0] = mc_prep_share_size(p, false);
    s->prep_share_size[1] = mc_prep_share_size(p, true);
    s->algorithm_id = p.alg_id;
    return 0;
}
