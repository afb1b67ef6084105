// Aggregation: out shares summed over reports (k_fold), per group
// (k_fold_grouped), and agg shares summed over ranks (k_fold_shares).
#pragma once
#include "flp.hpp"
#include "group_fold.hpp"

// ------------------------------------------------------------- fold
// agg_share[i] = sum over valid reports of out[i]  (agg_update + merge).
// Workgroup (row, y) sums reports [y * chunk, (y + 1) * chunk) of one output
// element into agg_words[y][row]; with gridDim.y > 1 the per-chunk partials
// are then merged by k_fold_shares.  Four independent accumulators keep four
// loads in flight per lane (a level of a sweep has few rows and ~1M reports:
// one workgroup per row walking all reports was load-latency bound, ~7 ms).
template <class F>
__global__ __launch_bounds__(256) void k_fold(const uint32_t* out, int n, int stride, const uint8_t* valid, int chunk,
                                              uint32_t* agg_words) {
    typedef typename F::E E;
    __shared__ E red[256];
    const int row = blockIdx.x;
    const int r0 = blockIdx.y * chunk;
    const int r1 = min(n, r0 + chunk);
    auto get = [&](int r) {
        const E x = pl_load<F>(out, row, stride, r);
        return (valid && !valid[r]) ? F::zero() : x;
    };
    E a0 = F::zero(), a1 = F::zero(), a2 = F::zero(), a3 = F::zero();
    int r = r0 + (int)threadIdx.x;
    for (; r + 768 < r1; r += 1024) {
        const E x0 = get(r), x1 = get(r + 256), x2 = get(r + 512), x3 = get(r + 768);
        a0 = F::add(a0, x0);
        a1 = F::add(a1, x1);
        a2 = F::add(a2, x2);
        a3 = F::add(a3, x3);
    }
    for (; r < r1; r += 256) a0 = F::add(a0, get(r));
    const E acc = F::add(F::add(a0, a1), F::add(a2, a3));
    agg_words += (size_t)blockIdx.y * gridDim.x * F::W32;
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = F::add(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        E x = red[0];
        for (int i = 0; i < F::W32; i++) agg_words[(size_t)row * F::W32 + i] = F::word(x, i);
    }
}

// agg[g][i] = sum over the valid reports of group g of out[i]: the fold of
// mastic_aggregate_grouped (plan, accumulation scheme and why: group_fold.hpp).
// Workgroup (row, y) streams reports [y * chunk, (y + 1) * chunk) of one output
// element as k_fold does and adds each element's 32-bit words into the 64-bit
// LDS counters of its group, cnt[(g * W32 + word) * copies + copy]; groups
// outside [g0, g0 + gpp) (another pass, MASTIC_GROUP_NONE, a masked report)
// add nothing.  Then one lane per group sums the copies, recombines the words
// mod p and stores part[y][g][row] (gridDim.y == 1: the pass's slice of the
// result itself).
template <class F>
__global__ __launch_bounds__(256) void k_fold_grouped(const uint32_t* out, int n, int stride, const uint32_t* group,
                                                      const uint8_t* valid, int chunk, uint32_t g0, int gpp,
                                                      int copies, uint32_t* part) {
    typedef typename F::E E;
    extern __shared__ unsigned long long gf_cnt[];
    const int slots = gpp * F::W32 * copies;
    for (int i = (int)threadIdx.x; i < slots; i += 256) gf_cnt[i] = 0;
    __syncthreads();
    const int row = blockIdx.x;
    const int r0 = blockIdx.y * chunk;
    const int r1 = min(n, r0 + chunk);
    const uint32_t cp = threadIdx.x & (uint32_t)(copies - 1);
    auto gid = [&](int r) {
        const uint32_t g = group[r];
        return (valid && !valid[r]) ? 0xFFFFFFFFu : g - g0;  // MASTIC_GROUP_NONE - g0 >= gpp as well
    };
    auto put = [&](uint32_t g, E x) {
        if (g >= (uint32_t)gpp) return;
#pragma unroll
        for (int i = 0; i < F::W32; i++)
            atomicAdd(&gf_cnt[(g * F::W32 + i) * copies + cp], (unsigned long long)F::word(x, i));
    };
    int r = r0 + (int)threadIdx.x;
    for (; r + 768 < r1; r += 1024) {
        const E x0 = pl_load<F>(out, row, stride, r), x1 = pl_load<F>(out, row, stride, r + 256),
                x2 = pl_load<F>(out, row, stride, r + 512), x3 = pl_load<F>(out, row, stride, r + 768);
        const uint32_t i0 = gid(r), i1 = gid(r + 256), i2 = gid(r + 512), i3 = gid(r + 768);
        put(i0, x0);
        put(i1, x1);
        put(i2, x2);
        put(i3, x3);
    }
    for (; r < r1; r += 256) put(gid(r), pl_load<F>(out, row, stride, r));
    __syncthreads();
    part += (size_t)blockIdx.y * gpp * gridDim.x * F::W32;
    for (int g = (int)threadIdx.x; g < gpp; g += 256) {
        uint64_t s[F::W32];
#pragma unroll
        for (int i = 0; i < F::W32; i++) {
            s[i] = 0;
            for (int c = 0; c < copies; c++) s[i] += gf_cnt[(g * F::W32 + i) * copies + c];
        }
        const E x = limbs_to_elem<F>(s);
#pragma unroll
        for (int i = 0; i < F::W32; i++) part[((size_t)g * gridDim.x + row) * F::W32 + i] = F::word(x, i);
    }
}

// out[e] = sum_s in[s][e] (mod p): merges the agg shares gathered from the
// ranks of a multi-GPU job (RCCL's sum is not GF(p) addition).
template <class F>
__global__ __launch_bounds__(256) void k_fold_shares(const uint32_t* in, int n_shares, int n_elems, uint32_t* out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_elems) return;
    typename F::E acc = F::zero();
    for (int s = 0; s < n_shares; s++) {
        uint32_t w[F::W32];
        for (int i = 0; i < F::W32; i++) w[i] = in[((size_t)s * n_elems + e) * F::W32 + i];
        acc = F::add(acc, F::from_words(w));
    }
    for (int i = 0; i < F::W32; i++) out[(size_t)e * F::W32 + i] = F::word(acc, i);
}
