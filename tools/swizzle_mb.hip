// Microbenchmark: the LDS crossbar as the partner exchange of the 2-lane
// sponge (keccak.hpp keccak_p12_pair).  ds_swizzle_b32 in quad-perm mode
// [1,0,3,2] swaps the two lanes of a pair like v_mov_b32_dpp quad_perm does,
// but on the LDS data path: no VALU issue slot, no LDS memory, counted in
// lgkmcnt.  Whether it pays depends on two numbers nobody had measured on
// this chip, and on what they do to the latency-critical sponge chain:
//   thr      wave-instructions per cycle and CU, S swizzle waves each issuing
//            12 independent exchanges per wait (S = 4, 8, 16)
//   lat      cycles per link of a dependent chain  exchange -> xor -> exchange
//            (issue-to-use latency + one VALU op), for swizzle and for DPP
//   +rd      the same beside 12 waves issuing conflict-free ds_read_b32 the
//            way the level kernel's AES waves do (16 lookups, one wait; one
//            address op and one 3-input XOR per lookup: 2 VALU slots per
//            lookup against the level kernel's 1.75); their own lookup rate
//            with and without the swizzle waves is reported too
//   chain    keccak_p12_pair with DPP and with swizzle exchanges, one wave per
//            SIMD (C2's sponge occupancy), ns and cycles per permutation
//            and whether both bodies give the same state
// VALU instructions per permutation are static (the rounds are unrolled):
// count them in k_chain's loop body of a --cuda-device-only -S build; the
// numbers for this tree are in profiles/r07_resource_usage.txt.
// Not part of the product.  Build: hipcc --offload-arch=gfx950 -O3 -o swizzle_mb swizzle_mb.hip
#include "../draft-mouris-cfrg-mastic_amd/csrc/keccak.hpp"
#include <stdio.h>
#include <stdlib.h>

#define WAVES 16
#define TAB_WORDS (64 * 64)  // 64 rows of 64 lanes: lane l always reads bank l mod 32

// roles: waves [0, readers) read, waves [readers, readers + swz) exchange
// MODE 0 throughput (12 independent swizzles per wait), 1 swizzle chain, 2 DPP chain
template <int MODE>
__global__ __launch_bounds__(64 * WAVES) void k_swz(uint32_t* out, unsigned long long* cyc, int iters, int readers,
                                                    int swz, int riters, int stop_on_done) {
    __shared__ uint32_t tab[TAB_WORDS];
    __shared__ uint32_t done;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int i = threadIdx.x; i < TAB_WORDS; i += 64 * WAVES) tab[i] = 0x9e3779b9u * (uint32_t)(i + 1);
    if (threadIdx.x == 0) done = 0;
    __syncthreads();
    const size_t slot = (size_t)blockIdx.x * 64 * WAVES + threadIdx.x;
    const size_t wslot = (size_t)blockIdx.x * WAVES + wave;
    uint32_t acc = 0;
    unsigned long long t0 = 0, t1 = 0, n = 0;
    if (wave < readers) {
        uint32_t x[16];
#pragma unroll
        for (int k = 0; k < 16; k++) x[k] = threadIdx.x * 2654435761u + k * 40503u + blockIdx.x;
        const uint32_t l4 = 4u * (uint32_t)lane;
        t0 = clock64();
        for (int it = 0; it < riters; it++) {
            uint32_t v[16];
#pragma unroll
            for (int k = 0; k < 16; k++)  // byte address: row (6 bits of the state) * 256 + lane * 4 < 16 KiB
                v[k] = *(const uint32_t*)((const char*)tab + ((x[k] & 0x3f00u) | l4));
#pragma unroll
            for (int k = 0; k < 16; k++) x[k] = xor3_u32(v[k], x[(k + 1) & 15], (uint32_t)it);
            n += 16;
            if (stop_on_done && __hip_atomic_load(&done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) >= (uint32_t)swz)
                break;
        }
        t1 = clock64();
#pragma unroll
        for (int k = 0; k < 16; k++) acc ^= x[k];
    } else if (wave < readers + swz) {
        uint32_t v[12];
#pragma unroll
        for (int k = 0; k < 12; k++) v[k] = threadIdx.x * 7919u + k;
        t0 = clock64();
        for (int it = 0; it < iters; it++) {
            if (MODE == 0) {
                uint32_t q[12];
#pragma unroll
                for (int k = 0; k < 12; k++) q[k] = pair_swap<true>(v[k]);
#pragma unroll
                for (int k = 0; k < 12; k++) v[k] = q[k] + (uint32_t)k;
            } else {
#pragma unroll
                for (int k = 0; k < 12; k++) v[0] = (MODE == 1 ? pair_swap<true>(v[0]) : pair_swap<false>(v[0])) ^ v[k];
            }
            n += 12;
        }
        t1 = clock64();
#pragma unroll
        for (int k = 0; k < 12; k++) acc ^= v[k];
        if (lane == 0) atomicAdd(&done, 1u);
    }
    out[slot] = acc;
    if (lane == 0) {
        cyc[2 * wslot] = t1 - t0;
        cyc[2 * wslot + 1] = n;
    }
}

// one wave per SIMD: `perms` dependent permutations per lane pair
template <bool SWZ>
__global__ __launch_bounds__(256) void k_chain(uint32_t* out, unsigned long long* cyc, int perms) {
    KHalf s;
#pragma unroll
    for (int i = 0; i < 25; i++) s.a[i] = threadIdx.x * 0x9e3779b9u + blockIdx.x + i;
    const bool hi = threadIdx.x & 1;
    const unsigned long long t0 = clock64();
    for (int p = 0; p < perms; p++) {
        asm volatile("; perm begin" ::: "memory");
        keccak_p12_pair<12, SWZ>(s, hi);
        asm volatile("; perm end" ::: "memory");
    }
    const unsigned long long t1 = clock64();
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < 25; i++) acc ^= s.a[i];
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = acc;
    if ((threadIdx.x & 63) == 0) cyc[(size_t)blockIdx.x * 4 + (threadIdx.x >> 6)] = t1 - t0;
}

struct Timer {
    hipEvent_t a, b;
    Timer() { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
    void start() { (void)hipEventRecord(a); }
    float stop() {
        (void)hipEventRecord(b);
        (void)hipEventSynchronize(b);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, a, b);
        return ms;
    }
};

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

int main(int argc, char** argv) {
    const int iters = argc > 1 ? atoi(argv[1]) : 20000;
    const int grid = 256;  // one workgroup per CU
    uint32_t* out;
    unsigned long long *cyc, *hcyc;
    CHECK(hipMalloc(&out, (size_t)grid * 64 * WAVES * 4));
    CHECK(hipMalloc(&cyc, (size_t)grid * WAVES * 2 * 8));
    hcyc = (unsigned long long*)malloc((size_t)grid * WAVES * 2 * 8);
    Timer tm;
    struct V { const char* name; int mode, readers, swz, stop; };
    const V vs[] = {{"thr S=4", 0, 0, 4, 0},       {"thr S=8", 0, 0, 8, 0},       {"thr S=16", 0, 0, 16, 0},
                    {"lat swizzle", 1, 0, 4, 0},   {"lat dpp", 2, 0, 4, 0},       {"rd alone", 0, 12, 0, 0},
                    {"thr S=4 +rd", 0, 12, 4, 1},  {"lat swizzle +rd", 1, 12, 4, 1}, {"lat dpp +rd", 2, 12, 4, 1}};
    for (const V& v : vs) {
        // readers beside exchange waves run until those are done (bounded); alone, a fixed count
        const int riters = v.stop ? iters * 16 : iters;
        for (int pass = 0; pass < 2; pass++) {  // pass 0 warms up
            CHECK(hipMemset(cyc, 0, (size_t)grid * WAVES * 2 * 8));
            tm.start();
            switch (v.mode) {
                case 0: hipLaunchKernelGGL((k_swz<0>), dim3(grid), dim3(64 * WAVES), 0, 0, out, cyc, iters, v.readers, v.swz, riters, v.stop); break;
                case 1: hipLaunchKernelGGL((k_swz<1>), dim3(grid), dim3(64 * WAVES), 0, 0, out, cyc, iters, v.readers, v.swz, riters, v.stop); break;
                default: hipLaunchKernelGGL((k_swz<2>), dim3(grid), dim3(64 * WAVES), 0, 0, out, cyc, iters, v.readers, v.swz, riters, v.stop); break;
            }
            const float ms = tm.stop();
            CHECK(hipGetLastError());
            if (pass == 0) continue;
            CHECK(hipMemcpy(hcyc, cyc, (size_t)grid * WAVES * 2 * 8, hipMemcpyDeviceToHost));
            // per CU: instructions of a role / the role's longest wave time (cycles of clock64)
            double x_rate = 0, x_link = 0, r_rate = 0;
            for (int g = 0; g < grid; g++) {
                double xn = 0, xc = 0, rn = 0, rc = 0;
                for (int w = 0; w < WAVES; w++) {
                    const double c = (double)hcyc[2 * ((size_t)g * WAVES + w)], n = (double)hcyc[2 * ((size_t)g * WAVES + w) + 1];
                    if (w < v.readers) { rn += n; if (c > rc) rc = c; }
                    else if (w < v.readers + v.swz) { xn += n; if (c > xc) xc = c; x_link += c / n; }
                }
                if (xc > 0) x_rate += xn / xc;
                if (rc > 0) r_rate += rn / rc;
            }
            printf("{\"variant\": \"%s\", \"ms\": %.3f", v.name, ms);
            if (v.swz) printf(", \"exchanges_per_clk_per_cu\": %.4f, \"clk_per_exchange_per_wave\": %.2f", x_rate / grid,
                              x_link / ((double)grid * v.swz));
            if (v.readers) printf(", \"lookups_per_clk_per_cu\": %.4f", r_rate / grid);
            printf("}\n");
            fflush(stdout);
        }
    }
    const int perms = iters / 20 > 0 ? iters / 20 : 1;
    uint32_t* hout[2] = {(uint32_t*)malloc((size_t)grid * 256 * 4), (uint32_t*)malloc((size_t)grid * 256 * 4)};
    for (int swzf = 0; swzf < 2; swzf++) {
        for (int pass = 0; pass < 2; pass++) {
            tm.start();
            if (swzf) hipLaunchKernelGGL((k_chain<true>), dim3(grid), dim3(256), 0, 0, out, cyc, perms);
            else hipLaunchKernelGGL((k_chain<false>), dim3(grid), dim3(256), 0, 0, out, cyc, perms);
            const float ms = tm.stop();
            CHECK(hipGetLastError());
            if (pass == 0) continue;
            CHECK(hipMemcpy(hcyc, cyc, (size_t)grid * 4 * 8, hipMemcpyDeviceToHost));
            CHECK(hipMemcpy(hout[swzf], out, (size_t)grid * 256 * 4, hipMemcpyDeviceToHost));
            double c = 0;
            for (int i = 0; i < grid * 4; i++) c += (double)hcyc[i];
            printf("{\"variant\": \"chain %s\", \"ms\": %.3f, \"ns_per_perm\": %.1f, \"clk_per_perm\": %.0f}\n",
                   swzf ? "swizzle" : "dpp", ms, ms * 1e6 / perms, c / ((double)grid * 4) / perms);
            fflush(stdout);
        }
    }
    // both bodies compute the same permutation
    bool same = true;
    for (size_t i = 0; i < (size_t)grid * 256; i++) same = same && hout[0][i] == hout[1][i];
    printf("{\"chain_outputs_equal\": %s}\n", same ? "true" : "false");
    free(hout[0]);
    free(hout[1]);
    (void)hipFree(out);
    (void)hipFree(cyc);
    free(hcyc);
    return 0;
}
