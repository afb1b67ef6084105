// Test infrastructure (built by __graft_entry__.build_rows_ops, bound by
// tests/test_gpu_rows_ops.py): csrc/rows_kernels.hpp's k_gather_rows alone, out
// of place, on buffers the test chooses.  The test embeds the source rows and
// the destination range in canary bytes and picks both byte offsets, so any
// byte the kernel writes outside its rows shows up in the downloaded
// destination.
//
// rows_ops_gather returns 0, -1 for arguments that would let the kernel leave
// the buffers (checked here, before anything is launched), or the hipError_t.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rows_kernels.hpp"

namespace {
struct Dev {
    void* p = nullptr;
    ~Dev() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, (bytes + 15) / 16 * 16 + 16); }
};
}  // namespace

// src_host[src_bytes] holds the source rows from byte src_off on; dst_host
// [dst_bytes] is uploaded, receives rows 0..count-1 from byte dst_off on, and is
// downloaded again.  idx[n_idx]; the launch gathers idx[first..first+count).
extern "C" int rows_ops_gather(const uint8_t* src_host, size_t src_bytes, size_t src_off, uint8_t* dst_host,
                               size_t dst_bytes, size_t dst_off, size_t row_bytes, const uint32_t* idx, size_t n_idx,
                               size_t first, size_t count) {
    if (!src_host || !dst_host || !idx || row_bytes == 0 || count == 0) return -1;
    if (first > n_idx || count > n_idx - first) return -1;
    if (dst_off > dst_bytes || count > (dst_bytes - dst_off) / row_bytes) return -1;
    if (src_off > src_bytes) return -1;
    const size_t src_rows = (src_bytes - src_off) / row_bytes;
    for (size_t i = first; i < first + count; i++)
        if (idx[i] >= src_rows) return -1;
    if (rows_grid(row_bytes, count) > ROWS_MAX_GRID) return -1;
    Dev ds, dd, di;
    hipError_t e;
    if ((e = ds.alloc(src_bytes)) != hipSuccess || (e = dd.alloc(dst_bytes)) != hipSuccess ||
        (e = di.alloc(4 * n_idx)) != hipSuccess)
        return (int)e;
    if ((e = hipMemcpy(ds.p, src_host, src_bytes, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(dd.p, dst_host, dst_bytes, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(di.p, idx, 4 * n_idx, hipMemcpyHostToDevice)) != hipSuccess)
        return (int)e;
    hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)rows_grid(row_bytes, count)), dim3(ROWS_THREADS), 0, nullptr,
                       (const uint8_t*)ds.p + src_off, (uint8_t*)dd.p + dst_off, row_bytes, (const uint32_t*)di.p,
                       first, count, rows_slots_per_row(row_bytes));
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if ((e = hipStreamSynchronize(nullptr)) != hipSuccess) return (int)e;
    e = hipMemcpy(dst_host, dd.p, dst_bytes, hipMemcpyDeviceToHost);
    return (int)e;
}
