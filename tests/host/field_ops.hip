// TEST INFRASTRUCTURE -- csrc/field.hpp on the device (tests/test_gpu_field_ops.py;
// built by __graft_entry__.build_field_ops into tests/host/_build/libfield_ops.so).
// One kernel applies add, sub, mul, neg and finv element-wise, so the gfx950
// code generation of the __int128 arithmetic is compared with Python integers
// directly instead of only through end-to-end vectors.
//
// Elements are little-endian 64-bit words: one per element for Field64, two
// ({lo, hi}) for Field128.  out holds five arrays of n elements:
// add(a, b), sub(a, b), mul(a, b), neg(a), finv(a).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.hpp"

template <class F> struct Words;
template <> struct Words<F64> {
    static constexpr int W = 1;
    __device__ static F64::E load(const uint64_t* p) { return p[0]; }
    __device__ static void store(uint64_t* p, F64::E x) { p[0] = x; }
};
template <> struct Words<F128> {
    static constexpr int W = 2;
    __device__ static F128::E load(const uint64_t* p) { return F128::E{p[0], p[1]}; }
    __device__ static void store(uint64_t* p, F128::E x) {
        p[0] = x.lo;
        p[1] = x.hi;
    }
};

template <class F>
__global__ __launch_bounds__(256) void k_field_ops(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    typedef Words<F> Wd;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const typename F::E x = Wd::load(a + i * Wd::W), y = Wd::load(b + i * Wd::W);
    const size_t plane = n * Wd::W;
    Wd::store(out + 0 * plane + i * Wd::W, F::add(x, y));
    Wd::store(out + 1 * plane + i * Wd::W, F::sub(x, y));
    Wd::store(out + 2 * plane + i * Wd::W, F::mul(x, y));
    Wd::store(out + 3 * plane + i * Wd::W, F::neg(x));
    Wd::store(out + 4 * plane + i * Wd::W, finv<F>(x));
}

// Host buffers in, host buffer out (5 * n elements).  Returns 0 or the hipError_t.
extern "C" int field_ops_run(int bits, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
    if ((bits != 64 && bits != 128) || n == 0 || n > (1u << 24)) return -1;
    const size_t in_bytes = n * (size_t)(bits / 64) * 8;
    uint64_t *da = nullptr, *db = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&da, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&db, in_bytes);
    if (e == hipSuccess) e = hipMalloc(&dout, 5 * in_bytes);
    if (e == hipSuccess) e = hipMemcpy(da, a, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(db, b, in_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)((n + 255) / 256));
        if (bits == 64)
            hipLaunchKernelGGL(k_field_ops<F64>, grid, dim3(256), 0, 0, da, db, dout, n);
        else
            hipLaunchKernelGGL(k_field_ops<F128>, grid, dim3(256), 0, 0, da, db, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, dout, 5 * in_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(da);
    (void)hipFree(db);
    (void)hipFree(dout);
    return (int)e;
}
