// device_rows.h — the row-space filter (cph_filter_create_rows): an allowed-ROW bitmap becomes the allowed-ID bitmap
// the filtered search kernels read, so they do not learn a second filter format.
//
// Thread i handles internal id i: it reads rows[i] (coalesced), then bit rows[i] of the input bitmap (a gather: the
// words are random-access, 128 KiB per million rows), the wave ballots the 64 bits and one lane writes them as two
// dwords.  The tail wave masks ids >= n, so bits behind n stay clear as cph_filter promises.  The host statement is
// host_index.h: rows_filter_host.
#pragma once
#include <hip/hip_runtime.h>

#include "device_buf.h"

namespace cph {

// in / out: (n + 31) / 32 words each; rows: [n], every entry < n (a validated row map).
__global__ __launch_bounds__(256) void rows_filter_kernel(const uint32_t* __restrict__ in, const uint32_t* __restrict__ rows,
                                                          uint64_t n, uint32_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bit = false;
    if (i < n) {
        const uint32_t r = rows[i];
        bit = (in[r >> 5] >> (r & 31)) & 1u;
    }
    const unsigned long long m = __ballot(bit);
    if ((threadIdx.x & 63) == 0) {
        const uint64_t w = i >> 5, nw = (n + 31) / 32;      // i is this wave's first id: a multiple of 64
        if (w < nw) out[w] = (uint32_t)m;
        if (w + 1 < nw) out[w + 1] = (uint32_t)(m >> 32);
    }
}

// Enqueues the conversion on `st`; d_in, d_rows and d_out live on the current device.
inline void rows_filter(const uint32_t* d_in, const uint32_t* d_rows, uint64_t n, uint32_t* d_out, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(rows_filter_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, d_in, d_rows, n, d_out);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
