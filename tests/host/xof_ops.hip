// TEST INFRASTRUCTURE -- the XOF layer on the device (tests/test_gpu_xof_ops.py;
// built by __graft_entry__.build_xof_ops into tests/host/_build/libxof_ops.so).
// csrc/keccak.hpp's permutations and sponge functions, node_proof.hpp's
// node_proof_one, finish_kernels.hpp's squeeze_elems, planes.hpp's
// k_prefix_states, absorb_kernels.hpp's k_absorb and k_absorb_pair, and
// csrc/aes.hpp's two fixed-key AES paths, each alone on chosen inputs: a
// chosen sponge state, fill position, length, counter or key, which end to end
// only an honest client's randomness and a handful of ctx lengths choose.
//
// Every buffer is a host buffer of little-endian 32-bit words, lane-major
// unless stated (lane r's record at word r * record_words).  An entry point
// allocates, uploads, launches, synchronises and downloads; it returns 0, -1
// for arguments that could make a kernel leave its buffers (the descriptors of
// common.hpp have no hardware bound), or the hipError_t (xof_ops_aes: -2 if
// the AesPerm table was not at LDS address 0).  No kernel of this library
// traps or asserts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "absorb_kernels.hpp"
#include "aes.hpp"
#include "finish_kernels.hpp"
#include "flp.hpp"
#include "keccak.hpp"
#include "node_proof.hpp"
#include "planes.hpp"

namespace {

struct Dev {
    void* p = nullptr;
    ~Dev() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    hipError_t put(const void* src, size_t bytes) {
        hipError_t e = alloc(bytes);
        if (e == hipSuccess && bytes) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
        return e;
    }
    hipError_t zeros(size_t bytes) {
        hipError_t e = alloc(bytes);
        if (e == hipSuccess) e = hipMemset(p, 0, bytes ? bytes : 4);
        return e;
    }
    hipError_t get(void* dst, size_t bytes) const { return hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost); }
    uint32_t* w() const { return (uint32_t*)p; }
};

hipError_t finish() {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}

constexpr size_t MAX_LANES = 1u << 16;
constexpr int BLOCK = 128;  // 70 lanes: one full wave and a partly filled one

// the prefix states of `count` byte strings, as the product makes them
// (pfx_f[count]: their fill positions; *bad is set if one is not in 0..167)
hipError_t prefix_states(Dev& out, const uint8_t* bytes, const int* offs, const int* lens, int count, int* pfx_f,
                         bool* bad) {
    size_t total = 0;
    for (int i = 0; i < count; i++) total = total > (size_t)offs[i] + lens[i] ? total : (size_t)offs[i] + lens[i];
    Dev db, dofs, dl;
    hipError_t e = db.put(bytes, total);
    if (e == hipSuccess) e = dofs.put(offs, sizeof(int) * count);
    if (e == hipSuccess) e = dl.put(lens, sizeof(int) * count);
    if (e == hipSuccess) e = out.zeros(sizeof(PrefixState) * count);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_prefix_states, dim3(1), dim3(64), 0, 0, (const uint8_t*)db.p, (const int*)dofs.p,
                       (const int*)dl.p, count, (PrefixState*)out.p);
    e = finish();
    std::vector<PrefixState> ps(count);
    if (e == hipSuccess) e = out.get(ps.data(), sizeof(PrefixState) * count);
    if (e != hipSuccess) return e;
    *bad = false;
    for (int i = 0; i < count; i++) {
        pfx_f[i] = ps[i].f;
        if (ps[i].f < 0 || ps[i].f >= KECCAK_RATE) *bad = true;
    }
    return hipSuccess;
}

bool prefixes_ok(const int* offs, const int* lens, int count) {
    if (count <= 0 || count > 4096) return false;
    for (int i = 0; i < count; i++)
        if (offs[i] < 0 || lens[i] < 0 || lens[i] > 4096 || offs[i] > (1 << 24)) return false;
    return true;
}

}  // namespace

// ------------------------------------------------------------- A: permutations
// V = 0: keccak_p12<12, true>, 1: <12, false>; one lane = one state (50 words)
template <int V>
__global__ __launch_bounds__(BLOCK) void k_perm(int n, const uint32_t* in, uint32_t* out) {
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    KState s;
#pragma unroll
    for (int i = 0; i < 25; i++) s.a[i] = u32x2{in[(size_t)r * 50 + 2 * i], in[(size_t)r * 50 + 2 * i + 1]};
    keccak_p12<12, V == 0>(s);
#pragma unroll
    for (int i = 0; i < 25; i++) {
        out[(size_t)r * 50 + 2 * i] = s.a[i].lo;
        out[(size_t)r * 50 + 2 * i + 1] = s.a[i].hi;
    }
}
// two lanes = one state: lane 2k the low halves, lane 2k + 1 the high halves,
// as k_absorb_pair loads them
template <bool SWZ>
__global__ __launch_bounds__(BLOCK) void k_perm_pair(int n, const uint32_t* in, uint32_t* out) {
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const int r = t >> 1, h = t & 1;
    if (r >= n) return;  // both lanes of a pair leave together
    KHalf s;
#pragma unroll
    for (int i = 0; i < 25; i++) s.a[i] = in[(size_t)r * 50 + 2 * i + h];
    keccak_p12_pair<12, SWZ>(s, h != 0);
#pragma unroll
    for (int i = 0; i < 25; i++) out[(size_t)r * 50 + 2 * i + h] = s.a[i];
}

// states[n][50] -> out[n][50]; variant 0 fused theta, 1 unfused, 2 pair (DPP), 3 pair (LDS crossbar)
extern "C" int xof_ops_perm(int variant, size_t n, const uint32_t* states, uint32_t* out) {
    if (variant < 0 || variant > 3 || n == 0 || n > MAX_LANES || !states || !out) return -1;
    Dev di, dout;
    hipError_t e = di.put(states, n * 200);
    if (e == hipSuccess) e = dout.zeros(n * 200);
    if (e != hipSuccess) return (int)e;
    const dim3 g1((unsigned)((n + BLOCK - 1) / BLOCK)), g2((unsigned)((2 * n + BLOCK - 1) / BLOCK));
    switch (variant) {
        case 0: hipLaunchKernelGGL(k_perm<0>, g1, dim3(BLOCK), 0, 0, (int)n, di.w(), dout.w()); break;
        case 1: hipLaunchKernelGGL(k_perm<1>, g1, dim3(BLOCK), 0, 0, (int)n, di.w(), dout.w()); break;
        case 2: hipLaunchKernelGGL(k_perm_pair<false>, g2, dim3(BLOCK), 0, 0, (int)n, di.w(), dout.w()); break;
        default: hipLaunchKernelGGL(k_perm_pair<true>, g2, dim3(BLOCK), 0, 0, (int)n, di.w(), dout.w()); break;
    }
    e = finish();
    if (e == hipSuccess) e = dout.get(out, n * 200);
    return (int)e;
}

// ------------------------------------------------------------- B: one-lane sponge
// One workgroup row (blockIdx.y) = one configuration (prefix, body length);
// lane r absorbs the first nbytes bytes of its column of the body planes after
// the prefix (the harness zeroes the bytes of the last word past nbytes, which
// sponge_absorb_words requires of its loader), then pads and squeezes twice
// from the same state: domain 0x01 / 8 words and domain 0x02 / 4 words.
__global__ __launch_bounds__(BLOCK) void k_sponge(const PrefixState* pfx, const int* cfg, int lanes, int S,
                                                  const uint32_t* body, uint32_t* out) {
    const int c = blockIdx.y;
    const int r = threadIdx.x;
    if (r >= lanes) return;
    const int id = __builtin_amdgcn_readfirstlane(cfg[2 * c]);
    const int nb = __builtin_amdgcn_readfirstlane(cfg[2 * c + 1]);
    KState s;
    int f;
    load_prefix(pfx, id, s, f);
    f = __builtin_amdgcn_readfirstlane(f);
    const int nw = (nb + 3) >> 2;
    const uint32_t last = (nb & 3) ? (1u << (8 * (nb & 3))) - 1u : ~0u;
    f = sponge_absorb_words(s, f, nb, [&](int m) {
        const uint32_t w = body[(size_t)m * S + r];
        return m == nw - 1 ? w & last : w;
    });
    uint32_t* o = out + ((size_t)c * lanes + r) * 12;
    KState s2 = s;
    sponge_pad(s, f, 0x01);
    sponge_squeeze_words(s, 8, [&](int j, uint32_t w) { o[j] = w; });
    sponge_pad(s2, f, 0x02);
    sponge_squeeze_words(s2, 4, [&](int j, uint32_t w) { o[8 + j] = w; });
}

// prefixes: npfx byte strings (bytes, offs, lens); cfg[ncfg][2] = (prefix index,
// body bytes); body[maxw][S] word planes, S >= lanes -> out[ncfg][lanes][12];
// pfx_f[npfx] = the fill positions k_prefix_states found
extern "C" int xof_ops_sponge(int npfx, const uint8_t* bytes, const int* offs, const int* lens, size_t ncfg,
                              const int* cfg, int lanes, int S, int maxw, const uint32_t* body, uint32_t* out,
                              int* pfx_f) {
    if (!prefixes_ok(offs, lens, npfx) || ncfg == 0 || ncfg > 65535 || lanes <= 0 || lanes > BLOCK || S < lanes ||
        maxw <= 0 || maxw > 4096)
        return -1;
    for (size_t c = 0; c < ncfg; c++)
        if (cfg[2 * c] < 0 || cfg[2 * c] >= npfx || cfg[2 * c + 1] < 0 || cfg[2 * c + 1] > 4 * maxw) return -1;
    Dev dp, dc, db, dout;
    bool bad = false;
    hipError_t e = prefix_states(dp, bytes, offs, lens, npfx, pfx_f, &bad);
    if (e == hipSuccess && bad) return -1;  // f in 0..167 before a sponge function sees it
    if (e == hipSuccess) e = dc.put(cfg, ncfg * 8);
    if (e == hipSuccess) e = db.put(body, (size_t)maxw * S * 4);
    if (e == hipSuccess) e = dout.zeros(ncfg * lanes * 48);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_sponge, dim3(1, (unsigned)ncfg), dim3(BLOCK), 0, 0, (const PrefixState*)dp.p,
                       (const int*)dc.p, lanes, S, db.w(), dout.w());
    e = finish();
    if (e == hipSuccess) e = dout.get(out, ncfg * lanes * 48);
    return (int)e;
}

// ------------------------------------------------------------- C: next_vec from a chosen state
// squeeze_elems<F> + pl_store_lane<F>, as k_flp_rand calls them; one lane = one state
template <class F>
__global__ __launch_bounds__(BLOCK) void k_squeeze(int n, int S, int count, const uint32_t* in, uint32_t* out) {
    typedef typename F::E E;
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n) return;
    KState s;
#pragma unroll
    for (int i = 0; i < 25; i++) s.a[i] = u32x2{in[(size_t)r * 50 + 2 * i], in[(size_t)r * 50 + 2 * i + 1]};
    squeeze_elems<F>(s, count, [&](int e, E x) { pl_store_lane<F>(out, e, S, r, x); });
}

// states[n][50] are squeezed as they stand (the rate words are the first
// block's stream).  planes[rows][S] comes in pre-filled and goes back whole:
// element e of lane r is words planes[(e * W32 + i) * S + r]; rows >= count * W32.
extern "C" int xof_ops_squeeze(int field, size_t n, int S, int count, int rows, const uint32_t* states,
                               uint32_t* planes) {
    const int w32 = field == 64 ? 2 : 4;
    if ((field != 64 && field != 128) || n == 0 || n > MAX_LANES || S < (int)n || S > (1 << 16) || count <= 0 ||
        count > 4096 || rows < count * w32 || rows > (1 << 16))
        return -1;
    Dev di, dout;
    hipError_t e = di.put(states, n * 200);
    if (e == hipSuccess) e = dout.put(planes, (size_t)rows * S * 4);
    if (e != hipSuccess) return (int)e;
    const dim3 g((unsigned)((n + BLOCK - 1) / BLOCK));
    if (field == 64) hipLaunchKernelGGL(k_squeeze<F64>, g, dim3(BLOCK), 0, 0, (int)n, S, count, di.w(), dout.w());
    else hipLaunchKernelGGL(k_squeeze<F128>, g, dim3(BLOCK), 0, 0, (int)n, S, count, di.w(), dout.w());
    e = finish();
    if (e == hipSuccess) e = dout.get(planes, (size_t)rows * S * 4);
    return (int)e;
}

// ------------------------------------------------------------- D: node proofs
// One workgroup row = one configuration (prefix, path_bytes) with bits =
// 8 * path_bytes and level = bits - 1; lane record: seed[4], pcw[8], path[8], t.
// The harness zeroes the path bytes past path_bytes.  Both theta forms.
#define NP_REC 21
__global__ __launch_bounds__(BLOCK) void k_node_proof_case(const PrefixState* pfx, const int* cfg, int lanes,
                                                           const uint32_t* in, uint32_t* out) {
    const int c = blockIdx.y;
    const int r = threadIdx.x;
    if (r >= lanes) return;
    const int id = __builtin_amdgcn_readfirstlane(cfg[2 * c]);
    const int pb = __builtin_amdgcn_readfirstlane(cfg[2 * c + 1]);
    const int f = __builtin_amdgcn_readfirstlane(pfx[id].f);
    const uint32_t* rec = in + (size_t)r * NP_REC;
    uint32_t seed[4], pcw[8], path[8];
#pragma unroll
    for (int i = 0; i < 4; i++) seed[i] = rec[i];
#pragma unroll
    for (int i = 0; i < 8; i++) pcw[i] = rec[4 + i];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int left = pb - 4 * i;  // path bytes in this word
        const uint32_t m = left >= 4 ? ~0u : (left <= 0 ? 0u : (1u << (8 * left)) - 1u);
        path[i] = rec[12 + i] & m;
    }
    const uint32_t t = rec[20] & 1u;
    uint32_t* o = out + ((size_t)c * lanes + r) * 16;
    node_proof_one<true>(pfx + id, f, 8 * pb, 8 * pb - 1, pb, seed, path, t, pcw, [&](int j, uint32_t w) { o[j] = w; });
    node_proof_one<false>(pfx + id, f, 8 * pb, 8 * pb - 1, pb, seed, path, t, pcw,
                          [&](int j, uint32_t w) { o[8 + j] = w; });
}

// cfg[ncfg][2] = (prefix index, path_bytes in 1..32); in[lanes][21] -> out[ncfg][lanes][16]
// (words 0..7 fused theta, 8..15 unfused); pfx_f[npfx] as above
extern "C" int xof_ops_node_proof(int npfx, const uint8_t* bytes, const int* offs, const int* lens, size_t ncfg,
                                  const int* cfg, int lanes, const uint32_t* in, uint32_t* out, int* pfx_f) {
    if (!prefixes_ok(offs, lens, npfx) || ncfg == 0 || ncfg > 65535 || lanes <= 0 || lanes > BLOCK) return -1;
    for (size_t c = 0; c < ncfg; c++)
        if (cfg[2 * c] < 0 || cfg[2 * c] >= npfx || cfg[2 * c + 1] < 1 || cfg[2 * c + 1] > 32) return -1;
    Dev dp, dc, di, dout;
    bool bad = false;
    hipError_t e = prefix_states(dp, bytes, offs, lens, npfx, pfx_f, &bad);
    if (e != hipSuccess) return (int)e;
    if (bad) return -1;  // f in 0..167 before node_proof_one sees it
    e = dc.put(cfg, ncfg * 8);
    if (e == hipSuccess) e = di.put(in, (size_t)lanes * NP_REC * 4);
    if (e == hipSuccess) e = dout.zeros(ncfg * lanes * 64);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_node_proof_case, dim3(1, (unsigned)ncfg), dim3(BLOCK), 0, 0, (const PrefixState*)dp.p,
                       (const int*)dc.p, lanes, di.w(), dout.w());
    e = finish();
    if (e == hipSuccess) e = dout.get(out, ncfg * lanes * 64);
    return (int)e;
}

// ------------------------------------------------------------- E: k_absorb, k_absorb_pair
// A case is 10 ints: f0, nb0, f1, nb1, prio, reset, tot0, tot1, skip0, skip1.
// Sponge w absorbs nb_w bytes at fill position f_w from stream words
// [skip_w, skip_w + nb_w / 4) of a segment of tot_w words per report, which
// is laid out so that it ENDS with the pool's allocation: the buffer is exactly
// as large as the kernel may read.  reset = 1 starts the case from the initial
// planes, 0 continues the previous case's (a chained launch).  After every
// case both sponges' planes are kept: out[case][2][50][stride].
// layout 0: tiled (rstride 64, gstride tot * 64); 1: planes (rstride stride, gstride 64).
#define AB_REC 10
extern "C" int xof_ops_absorb(int pair, int layout, int n, int stride, size_t ncases, const int* cases,
                              const uint32_t* init, const uint32_t* pool0, const uint32_t* pool1, size_t pool_words,
                              uint32_t* out) {
    if (pair < 0 || pair > 1 || layout < 0 || layout > 1 || n <= 0 || stride <= 0 || stride % 64 || n > stride ||
        stride > 1024 || ncases == 0 || ncases > (1u << 16) || pool_words == 0 || pool_words > (1u << 26))
        return -1;
    const size_t groups = (size_t)stride / 64;
    auto seg_words = [&](int tot) { return layout == 0 ? groups * (size_t)tot * 64 : (size_t)tot * stride; };
    for (size_t c = 0; c < ncases; c++) {
        const int* k = cases + c * AB_REC;
        if (k[4] < 0 || k[4] > 3 || (k[5] != 0 && k[5] != 1) || (c == 0 && k[5] != 1)) return -1;
        for (int w = 0; w < 2; w++) {
            const int f = k[2 * w], nb = k[2 * w + 1], tot = k[6 + w], skip = k[8 + w];
            if (f < 0 || f >= KECCAK_RATE || nb < 0 || nb % 4 || nb > (1 << 16) || tot < 0 || skip < 0) return -1;
            if (nb > 0 && (skip + nb / 4 > tot || seg_words(tot) > pool_words)) return -1;
        }
    }
    const size_t plane_bytes = (size_t)2 * 50 * stride * 4;
    Dev dinit, dsp, dpool[2], dout;
    hipError_t e = dinit.put(init, plane_bytes);
    if (e == hipSuccess) e = dsp.alloc(plane_bytes);
    if (e == hipSuccess) e = dpool[0].put(pool0, pool_words * 4);
    if (e == hipSuccess) e = dpool[1].put(pool1, pool_words * 4);
    if (e == hipSuccess) e = dout.alloc(ncases * plane_bytes);
    if (e != hipSuccess) return (int)e;
    Planes pl{};
    pl.n = n;
    pl.stride = stride;
    pl.sp_onehot = dsp.w();
    pl.sp_payload = dsp.w() + (size_t)50 * stride;
    for (size_t c = 0; c < ncases && e == hipSuccess; c++) {
        const int* k = cases + c * AB_REC;
        AbsorbArgs ab{};
        for (int w = 0; w < 2; w++) {
            const int tot = k[6 + w], skip = k[8 + w];
            const size_t rstride = layout == 0 ? 64 : (size_t)stride;
            ab.f[w] = k[2 * w];
            ab.nbytes[w] = k[2 * w + 1];
            ab.gstride[w] = layout == 0 ? tot * 64 : 64;
            ab.seg[w] = dpool[w].w();
            if (ab.nbytes[w]) ab.seg[w] += pool_words - seg_words(tot) + (size_t)skip * rstride;
        }
        ab.rstride = layout == 0 ? 64 : stride;
        ab.prio = k[4];
        ab.dbg = 0;
        ab.which0 = 0;
        if (k[5]) e = hipMemcpyAsync(dsp.p, dinit.p, plane_bytes, hipMemcpyDeviceToDevice, 0);
        if (e != hipSuccess) break;
        // the grid shapes of prep.hpp's Chunk
        if (pair)
            hipLaunchKernelGGL(k_absorb_pair, dim3((unsigned)((groups * 64 * 2 + 255) / 256), 2), dim3(256), 0, 0, pl,
                               ab);
        else
            hipLaunchKernelGGL(k_absorb, dim3((unsigned)((groups * 64 + 255) / 256), 2), dim3(256), 0, 0, pl, ab);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync((char*)dout.p + c * plane_bytes, dsp.p, plane_bytes, hipMemcpyDeviceToDevice, 0);
    }
    if (e == hipSuccess) e = finish();
    if (e == hipSuccess) e = dout.get(out, ncases * plane_bytes);
    return (int)e;
}

// ------------------------------------------------------------- F: fixed-key AES
// Lane record in[lane]: key[4], seed_a[4], seed_b[4].  ctrs[nctr] are uniform.
// blocks[lanes][nblk][4] are raw AES inputs.
//
// AesLds path (k_setup's): the lane expands its own key (aes128_expand) ->
// rk[lanes][44]; ct[lanes][nblk][4] = aes128_encrypt(RkRegs);
// fk[lanes][nctr][16] = fixed_key_block (RkRegs) of seed_a | the same with
// RkLds | fixed_key_block2 (RkLds) of (seed_a, ctr[i]) and (seed_b, ctr[i + 1 mod nctr]).
__global__ __launch_bounds__(BLOCK) void k_aes_lds(int lanes, int nblk, int nctr, const uint32_t* in,
                                                   const uint32_t* blocks, const uint32_t* ctrs, uint32_t* rk_out,
                                                   uint32_t* ct, uint32_t* fk) {
    __shared__ uint32_t T[AES_LDS_WORDS];
    __shared__ uint4 RK[BLOCK * 11];
    aes_lds_fill(T, threadIdx.x, BLOCK);
    __syncthreads();
    const int r = threadIdx.x;
    if (r >= lanes) return;
    const AesLds TL{T + (r & 31)};
    const uint32_t* rec = in + (size_t)r * 12;
    uint32_t key[4], sa[4], sb[4], rk[44];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        key[i] = rec[i];
        sa[i] = rec[4 + i];
        sb[i] = rec[8 + i];
    }
    aes128_expand(TL, key, rk);
#pragma unroll
    for (int i = 0; i < 44; i++) {
        rk_out[(size_t)r * 44 + i] = rk[i];
        ((uint32_t*)RK)[r * 44 + i] = rk[i];
    }
    const RkLds rl{RK + r * 11};  // rows are read by the lane that wrote them
    for (int b = 0; b < nblk; b++) {
        uint32_t s[4];
#pragma unroll
        for (int i = 0; i < 4; i++) s[i] = blocks[((size_t)r * nblk + b) * 4 + i];
        aes128_encrypt(TL, RkRegs{rk}, s);
#pragma unroll
        for (int i = 0; i < 4; i++) ct[((size_t)r * nblk + b) * 4 + i] = s[i];
    }
    for (int c = 0; c < nctr; c++) {
        const uint32_t ca = ctrs[c], cb = ctrs[(c + 1) % nctr];
        uint32_t o[16];
        fixed_key_block(TL, RkRegs{rk}, sa, ca, o);
        fixed_key_block(TL, rl, sa, ca, o + 4);
        fixed_key_block2(TL, rl, sa, ca, sb, cb, o + 8, o + 12);
#pragma unroll
        for (int i = 0; i < 16; i++) fk[((size_t)r * nctr + c) * 16 + i] = o[i];
    }
}

// AesPerm path (the level kernel's): dynamic LDS laid out as eval_aes_body lays
// it out, the table at LDS address 0 (checked: status[0] = 1 and nothing runs
// if it is not) and the key rows after it, stored through aes_perm_key_word.
// The key schedules come from the host (rk_in[lanes][44]).
// ct[lanes][nblk][4] = aes128_encrypt; fk[lanes][nctr][36] = fixed_key_block_n<1>
// of seed_a | <2> of (seed_a, ctr i), (seed_b, ctr i+1) | <4> of seeds a, b, a, b
// at ctr i, i+1, i+2, i+3 (indices mod nctr) | fixed_key_block2 of the <2> inputs.
// Counter groups: ops[nops][5] = (kind, hi_a, hi_b, c_a, c_b) -> grp[lanes][nops][16]:
//   kind 0: ctr_group_init<1>(seed_a, hi_a), ctr_blocks_n<1>(c_a)
//   kind 1: ctr_group_init<1>(seed_a, hi_a), ctr_blocks_n<2> of c_a and c_b from that one group
//   kind 2: ctr_group_init<2>((seed_a, hi_a), (seed_b, hi_b)), ctr_blocks_n<2>((seed_a, c_a), (seed_b, c_b))
//   kind 3: no init: ctr_blocks_n<1>(c_a) from seed_a's group as the previous op left it
//   kind 4: kind 2's init, then ctr_blocks_n<4> (which the product does not call) of (seed_a, c_a),
//           (seed_b, c_b), (seed_a, c_a ^ 1), (seed_b, c_b ^ 1)
// The groups are the same two variables throughout, so an op re-initialises
// what the previous one used, as parent_payload does.
__global__ __launch_bounds__(BLOCK) void k_aes_perm(int lanes, int nblk, int nctr, int nops, const uint32_t* in,
                                                    const uint32_t* rk_in, const uint32_t* blocks,
                                                    const uint32_t* ctrs, const uint32_t* ops, uint32_t* ct,
                                                    uint32_t* fk, uint32_t* grp, uint32_t* status) {
    extern __shared__ uint4 xof_lds[];
    uint32_t* T = (uint32_t*)xof_lds;
    uint4* RK = xof_lds + AES_PERM_LDS_WORDS / 4;
    if ((uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint4*)xof_lds != 0u) {
        if (threadIdx.x == 0) status[0] = 1u;
        return;
    }
    aes_perm_fill(T, threadIdx.x, BLOCK);
    const int r = threadIdx.x;
    if (r < lanes) {
#pragma unroll
        for (int i = 0; i < 44; i++) ((uint32_t*)RK)[r * 44 + i] = aes_perm_key_word(i, rk_in[(size_t)r * 44 + i]);
    }
    __syncthreads();
    if (r >= lanes) return;
    const int lane = r & 63;
    const AesPerm TL{T, 4u * (uint32_t)(lane & 31), 128u + 4u * (uint32_t)(lane & 31)};
    const RkLds rl{RK + r * 11};
    const uint32_t* rec = in + (size_t)r * 12;
    uint32_t sa[4], sb[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        sa[i] = rec[4 + i];
        sb[i] = rec[8 + i];
    }
    for (int b = 0; b < nblk; b++) {
        asm volatile("" ::: "memory");  // key rows re-read per block, as in the level kernel
        uint32_t s[4];
#pragma unroll
        for (int i = 0; i < 4; i++) s[i] = blocks[((size_t)r * nblk + b) * 4 + i];
        aes128_encrypt(TL, rl, s);
#pragma unroll
        for (int i = 0; i < 4; i++) ct[((size_t)r * nblk + b) * 4 + i] = s[i];
    }
    for (int c = 0; c < nctr; c++) {
        asm volatile("" ::: "memory");
        const uint32_t c0 = ctrs[c], c1 = ctrs[(c + 1) % nctr], c2 = ctrs[(c + 2) % nctr], c3 = ctrs[(c + 3) % nctr];
        uint32_t o[36];
        {
            const uint32_t* const sd[1] = {sa};
            const uint32_t cv[1] = {c0};
            uint32_t* const ov[1] = {o};
            fixed_key_block_n<1>(TL, rl, sd, cv, ov);
        }
        {
            const uint32_t* const sd[2] = {sa, sb};
            const uint32_t cv[2] = {c0, c1};
            uint32_t* const ov[2] = {o + 4, o + 8};
            fixed_key_block_n<2>(TL, rl, sd, cv, ov);
        }
        {
            const uint32_t* const sd[4] = {sa, sb, sa, sb};
            const uint32_t cv[4] = {c0, c1, c2, c3};
            uint32_t* const ov[4] = {o + 12, o + 16, o + 20, o + 24};
            fixed_key_block_n<4>(TL, rl, sd, cv, ov);
        }
        fixed_key_block2(TL, rl, sa, c0, sb, c1, o + 28, o + 32);
#pragma unroll
        for (int i = 0; i < 36; i++) fk[((size_t)r * nctr + c) * 36 + i] = o[i];
    }
    AesCtrGroup ga, gb;
    ga.a = ga.p2 = gb.a = gb.p2 = 0u;
#pragma unroll
    for (int i = 0; i < 4; i++) ga.q[i] = gb.q[i] = 0u;
    for (int k = 0; k < nops; k++) {
        asm volatile("" ::: "memory");
        const uint32_t kind = ops[5 * k], ha = ops[5 * k + 1], hb = ops[5 * k + 2], ca = ops[5 * k + 3],
                       cb = ops[5 * k + 4];
        uint32_t o[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (kind == 0 || kind == 1) {
            const uint32_t* const sd[1] = {sa};
            const uint32_t hv[1] = {ha};
            AesCtrGroup* const gi[1] = {&ga};
            ctr_group_init<1>(TL, rl, sd, hv, gi);
        } else if (kind == 2 || kind == 4) {
            const uint32_t* const sd[2] = {sa, sb};
            const uint32_t hv[2] = {ha, hb};
            AesCtrGroup* const gi[2] = {&ga, &gb};
            ctr_group_init<2>(TL, rl, sd, hv, gi);
        }
        if (kind == 0 || kind == 3) {
            const AesCtrGroup* const gg[1] = {&ga};
            const uint32_t* const sd[1] = {sa};
            const uint32_t cv[1] = {ca};
            uint32_t* const ov[1] = {o};
            ctr_blocks_n<1>(TL, rl, gg, sd, cv, ov);
        } else if (kind == 1) {
            const AesCtrGroup* const gg[2] = {&ga, &ga};
            const uint32_t* const sd[2] = {sa, sa};
            const uint32_t cv[2] = {ca, cb};
            uint32_t* const ov[2] = {o, o + 4};
            ctr_blocks_n<2>(TL, rl, gg, sd, cv, ov);
        } else if (kind == 2) {
            const AesCtrGroup* const gg[2] = {&ga, &gb};
            const uint32_t* const sd[2] = {sa, sb};
            const uint32_t cv[2] = {ca, cb};
            uint32_t* const ov[2] = {o, o + 4};
            ctr_blocks_n<2>(TL, rl, gg, sd, cv, ov);
        } else {
            const AesCtrGroup* const gg[4] = {&ga, &gb, &ga, &gb};
            const uint32_t* const sd[4] = {sa, sb, sa, sb};
            const uint32_t cv[4] = {ca, cb, ca ^ 1u, cb ^ 1u};
            uint32_t* const ov[4] = {o, o + 4, o + 8, o + 12};
            ctr_blocks_n<4>(TL, rl, gg, sd, cv, ov);
        }
#pragma unroll
        for (int i = 0; i < 16; i++) grp[((size_t)r * nops + k) * 16 + i] = o[i];
    }
}

// path 0: AesLds (rk is an output, ops / grp unused), 1: AesPerm (rk is an input).
// in[lanes][12], blocks[lanes][nblk][4], ctrs[nctr], ops[nops][5];
// ct[lanes][nblk][4], fk[lanes][nctr][16 or 36], grp[lanes][nops][16].
extern "C" int xof_ops_aes(int path, int lanes, int nblk, int nctr, int nops, const uint32_t* in, uint32_t* rk,
                           const uint32_t* blocks, const uint32_t* ctrs, const uint32_t* ops, uint32_t* ct,
                           uint32_t* fk, uint32_t* grp) {
    if (path < 0 || path > 1 || lanes <= 0 || lanes > BLOCK || nblk <= 0 || nblk > 4096 || nctr <= 0 || nctr > 4096 ||
        nops < 0 || nops > 4096 || (path == 0 && nops != 0))
        return -1;
    // a group serves the counters that agree with its ctr_hi above bit 7; kind 3 needs a live group of seed_a
    uint32_t live = 0, have = 0;
    for (int k = 0; k < nops; k++) {
        const uint32_t kind = ops[5 * k], ha = ops[5 * k + 1], hb = ops[5 * k + 2], ca = ops[5 * k + 3],
                       cb = ops[5 * k + 4];
        if (kind > 4) return -1;
        if (kind == 3 && (!have || (live >> 8) != (ca >> 8))) return -1;
        if (kind != 3 && (ha >> 8) != (ca >> 8)) return -1;
        if (kind == 1 && (ha >> 8) != (cb >> 8)) return -1;
        if ((kind == 2 || kind == 4) && (hb >> 8) != (cb >> 8)) return -1;
        if (kind != 3) {
            live = ha;
            have = 1;
        }
    }
    const int fkw = path == 0 ? 16 : 36;
    Dev din, drk, dblk, dctr, dops, dct, dfk, dgrp, dst;
    hipError_t e = din.put(in, (size_t)lanes * 48);
    if (e == hipSuccess) e = path == 0 ? drk.zeros((size_t)lanes * 176) : drk.put(rk, (size_t)lanes * 176);
    if (e == hipSuccess) e = dblk.put(blocks, (size_t)lanes * nblk * 16);
    if (e == hipSuccess) e = dctr.put(ctrs, (size_t)nctr * 4);
    if (e == hipSuccess) e = dops.put(ops, (size_t)nops * 20);
    if (e == hipSuccess) e = dct.zeros((size_t)lanes * nblk * 16);
    if (e == hipSuccess) e = dfk.zeros((size_t)lanes * nctr * fkw * 4);
    if (e == hipSuccess) e = dgrp.zeros((size_t)lanes * nops * 64);
    if (e == hipSuccess) e = dst.zeros(4);
    if (e != hipSuccess) return (int)e;
    if (path == 0) {
        hipLaunchKernelGGL(k_aes_lds, dim3(1), dim3(BLOCK), 0, 0, lanes, nblk, nctr, din.w(), dblk.w(), dctr.w(),
                           drk.w(), dct.w(), dfk.w());
    } else {
        const size_t lds = (size_t)AES_PERM_LDS_WORDS * 4 + (size_t)BLOCK * 176;
        e = hipFuncSetAttribute((const void*)k_aes_perm, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL(k_aes_perm, dim3(1), dim3(BLOCK), lds, 0, lanes, nblk, nctr, nops, din.w(), drk.w(),
                           dblk.w(), dctr.w(), dops.w(), dct.w(), dfk.w(), dgrp.w(), dst.w());
    }
    e = finish();
    uint32_t st = 0;
    if (e == hipSuccess) e = dst.get(&st, 4);
    if (e == hipSuccess && st != 0) return -2;  // the table was not at LDS address 0
    if (e == hipSuccess && path == 0) e = drk.get(rk, (size_t)lanes * 176);
    if (e == hipSuccess) e = dct.get(ct, (size_t)lanes * nblk * 16);
    if (e == hipSuccess) e = dfk.get(fk, (size_t)lanes * nctr * fkw * 4);
    if (e == hipSuccess && nops) e = dgrp.get(grp, (size_t)lanes * nops * 64);
    return (int)e;
}
