// TEST INFRASTRUCTURE -- csrc/flp.hpp on the device (tests/test_gpu_flp_ops.py;
// built by __graft_entry__.build_flp_ops into tests/host/_build/libflp_ops.so).
// flp_prove, flp_query and flp_decide on chosen inputs, with no XOF, VIDPF or
// C ABI context around them, so that explicit randomness (a test point on a
// root of unity, joint randomness of 0 or p-1) and dishonest encodings reach
// the device code.  One lane = one case; the constants are the product's
// (flp_consts, flp_alpha_inv_pows).
//
// Every buffer is a host buffer of little-endian field elements, case-major
// (case c's vector of `elems` elements at byte c * elems * ENC); the library
// transposes to word planes of stride round_up(n, 64), the layout flp.hpp
// reads.  A parameter set is (circuit, length, sum_vec_bits, max_measurement,
// chunk_length) as mc_derive takes them.  Entry points return 0, -1 for bad
// arguments, or the hipError_t.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "flp.hpp"
#include "params.hpp"

namespace {

struct Dev {
    void* p = nullptr;
    ~Dev() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    uint32_t* w() const { return (uint32_t*)p; }
};

size_t stride_of(size_t n) { return (n + 63) / 64 * 64; }

// case-major elements -> zero-padded word planes [elems * W32][S] on the device
hipError_t upload(Dev& d, const uint8_t* src, size_t n, size_t S, int elems, int w32) {
    const size_t rows = (size_t)(elems > 0 ? elems : 1) * w32;
    std::vector<uint32_t> pl(rows * S, 0u);
    for (size_t c = 0; c < n && elems > 0; c++)
        for (size_t k = 0; k < (size_t)elems * w32; k++) {
            const uint8_t* b = src + (c * (size_t)elems * w32 + k) * 4;
            pl[k * S + c] = (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
        }
    hipError_t e = d.alloc(pl.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d.p, pl.data(), pl.size() * 4, hipMemcpyHostToDevice);
    return e;
}

// word planes [elems * W32][S] on the device -> case-major elements
hipError_t download(const Dev& d, uint8_t* dst, size_t n, size_t S, int elems, int w32) {
    const size_t rows = (size_t)elems * w32;
    std::vector<uint32_t> pl(rows * S);
    hipError_t e = hipMemcpy(pl.data(), d.p, pl.size() * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (size_t c = 0; c < n; c++)
        for (size_t k = 0; k < rows; k++) {
            const uint32_t w = pl[k * S + c];
            uint8_t* b = dst + (c * rows + k) * 4;
            b[0] = (uint8_t)w;
            b[1] = (uint8_t)(w >> 8);
            b[2] = (uint8_t)(w >> 16);
            b[3] = (uint8_t)(w >> 24);
        }
    return hipSuccess;
}

hipError_t zeros(Dev& d, size_t words) {
    hipError_t e = d.alloc(words * 4);
    if (e == hipSuccess) e = hipMemset(d.p, 0, words * 4);
    return e;
}

int derive(int circuit, int length, int sv_bits, uint64_t max_measurement, int chunk, size_t n, McParams* p) {
    if (n == 0 || n > (1u << 16)) return -1;
    return mc_derive(circuit, 1, length, sv_bits, max_measurement, chunk, p);
}

}  // namespace

template <class F>
__global__ __launch_bounds__(256) void k_prove(McParams p, FlpConsts<F> c, const typename F::E* pows, int n, int S,
                                               const uint32_t* meas, const uint32_t* jr, const uint32_t* prand,
                                               uint32_t* vals, uint32_t* coef, uint32_t* proof) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    flp_prove<F>(p, c, pows, meas, jr, prand, vals, coef, proof, S, r);
}

template <class F>
__global__ __launch_bounds__(256) void k_query(McParams p, FlpConsts<F> c, int n, int S, const uint32_t* meas,
                                               const uint32_t* proof, const uint32_t* qr, const uint32_t* jr,
                                               uint32_t* ver, uint8_t* ok) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    ok[r] = flp_query<F>(p, c, meas, proof, qr, jr, ver, S, r) ? 1 : 0;
}

template <class F>
__global__ __launch_bounds__(256) void k_decide_only(McParams p, int n, int S, const uint32_t* ver, uint8_t* out) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    out[r] = flp_decide<F>(p, ver, S, r) ? 1 : 0;
}

template <class F>
static int prove_impl(const McParams& p, size_t n, const uint8_t* meas, const uint8_t* prove_rand,
                      const uint8_t* joint_rand, uint8_t* proof) {
    typedef typename F::E E;
    const size_t S = stride_of(n);
    const FlpConsts<F> fc = flp_consts<F>(p);
    const std::vector<E> pows = flp_alpha_inv_pows<F>(fc, p.P);
    Dev dm, dj, dr, dv, dc, dp, dt;
    hipError_t e = upload(dm, meas, n, S, p.meas_len, p.w32);
    if (e == hipSuccess) e = upload(dj, joint_rand, n, S, p.joint_rand_len, p.w32);
    if (e == hipSuccess) e = upload(dr, prove_rand, n, S, p.arity, p.w32);
    // scratch as shard_impl sizes it: [arity * P * w32] planes each
    if (e == hipSuccess) e = zeros(dv, (size_t)p.arity * p.P * p.w32 * S);
    if (e == hipSuccess) e = zeros(dc, (size_t)p.arity * p.P * p.w32 * S);
    if (e == hipSuccess) e = zeros(dp, (size_t)p.proof_len * p.w32 * S);
    if (e == hipSuccess) e = dt.alloc(sizeof(E) * p.P);
    if (e == hipSuccess) e = hipMemcpy(dt.p, pows.data(), sizeof(E) * p.P, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_prove<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, p, fc, (const E*)dt.p,
                           (int)n, (int)S, dm.w(), dj.w(), dr.w(), dv.w(), dc.w(), dp.w());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = download(dp, proof, n, S, p.proof_len, p.w32);
    return (int)e;
}

template <class F>
static int query_impl(const McParams& p, size_t n, const uint8_t* meas_share, const uint8_t* proof_share,
                      const uint8_t* query_rand, const uint8_t* joint_rand, uint8_t* verifier, uint8_t* ok) {
    const size_t S = stride_of(n);
    const FlpConsts<F> fc = flp_consts<F>(p);
    Dev dm, dp, dq, dj, dv, dok;
    hipError_t e = upload(dm, meas_share, n, S, p.meas_len, p.w32);
    if (e == hipSuccess) e = upload(dp, proof_share, n, S, p.proof_len, p.w32);
    if (e == hipSuccess) e = upload(dq, query_rand, n, S, p.query_rand_len, p.w32);
    if (e == hipSuccess) e = upload(dj, joint_rand, n, S, p.joint_rand_len, p.w32);
    if (e == hipSuccess) e = zeros(dv, (size_t)p.verifier_len * p.w32 * S);
    if (e == hipSuccess) e = zeros(dok, S);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_query<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, p, fc, (int)n, (int)S,
                           dm.w(), dp.w(), dq.w(), dj.w(), dv.w(), (uint8_t*)dok.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = download(dv, verifier, n, S, p.verifier_len, p.w32);
    if (e == hipSuccess) e = hipMemcpy(ok, dok.p, n, hipMemcpyDeviceToHost);
    return (int)e;
}

template <class F>
static int decide_impl(const McParams& p, size_t n, const uint8_t* verifier, uint8_t* out) {
    const size_t S = stride_of(n);
    Dev dv, dout;
    hipError_t e = upload(dv, verifier, n, S, p.verifier_len, p.w32);
    if (e == hipSuccess) e = zeros(dout, S);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_decide_only<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, p, (int)n, (int)S,
                           dv.w(), (uint8_t*)dout.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout.p, n, hipMemcpyDeviceToHost);
    return (int)e;
}

// out[8] = field bits, meas_len, arity (= prove_rand_len), joint_rand_len,
// query_rand_len, proof_len, verifier_len, P
extern "C" int flp_ops_sizes(int circuit, int length, int sv_bits, uint64_t max_measurement, int chunk, int* out) {
    McParams p;
    if (derive(circuit, length, sv_bits, max_measurement, chunk, 1, &p)) return -1;
    const int v[8] = {p.field, p.meas_len, p.arity, p.joint_rand_len, p.query_rand_len, p.proof_len, p.verifier_len, p.P};
    for (int i = 0; i < 8; i++) out[i] = v[i];
    return 0;
}

// meas[n][meas_len], prove_rand[n][arity], joint_rand[n][joint_rand_len] -> proof[n][proof_len]
extern "C" int flp_ops_prove(int circuit, int length, int sv_bits, uint64_t max_measurement, int chunk, size_t n,
                             const uint8_t* meas, const uint8_t* prove_rand, const uint8_t* joint_rand,
                             uint8_t* proof) {
    McParams p;
    if (derive(circuit, length, sv_bits, max_measurement, chunk, n, &p)) return -1;
    return p.field == 64 ? prove_impl<F64>(p, n, meas, prove_rand, joint_rand, proof)
                         : prove_impl<F128>(p, n, meas, prove_rand, joint_rand, proof);
}

// meas_share[n][meas_len], proof_share[n][proof_len], query_rand[n][query_rand_len],
// joint_rand[n][joint_rand_len] -> verifier[n][verifier_len], ok[n] (0: the
// test point is a root of unity), with num_shares = 2
extern "C" int flp_ops_query(int circuit, int length, int sv_bits, uint64_t max_measurement, int chunk, size_t n,
                             const uint8_t* meas_share, const uint8_t* proof_share, const uint8_t* query_rand,
                             const uint8_t* joint_rand, uint8_t* verifier, uint8_t* ok) {
    McParams p;
    if (derive(circuit, length, sv_bits, max_measurement, chunk, n, &p)) return -1;
    return p.field == 64 ? query_impl<F64>(p, n, meas_share, proof_share, query_rand, joint_rand, verifier, ok)
                         : query_impl<F128>(p, n, meas_share, proof_share, query_rand, joint_rand, verifier, ok);
}

// verifier[n][verifier_len] (the sum of the shares) -> out[n] 0/1
extern "C" int flp_ops_decide(int circuit, int length, int sv_bits, uint64_t max_measurement, int chunk, size_t n,
                              const uint8_t* verifier, uint8_t* out) {
    McParams p;
    if (derive(circuit, length, sv_bits, max_measurement, chunk, n, &p)) return -1;
    return p.field == 64 ? decide_impl<F64>(p, n, verifier, out) : decide_impl<F128>(p, n, verifier, out);
}
