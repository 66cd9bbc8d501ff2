// device_normalize.h — the cosine metric's one kernel: rows (into the index) and queries (into every search) are scaled
// to squared norm 1/2, out = x / sqrt(2 |x|^2).  Then || q~ - x~ ||^2 = 1 - cos(q, x), and every squared-L2 kernel of the
// library reports the cosine distance as it stands.  host_normalize.h states the arithmetic, bit for bit.
//
// One wave per row, four waves per workgroup, grid-stride over the rows.  Lane l sums the squares of elements l, l + 64,
// ... (coalesced loads), the wave reduces with a xor butterfly (32, 16, 8, 4, 2, 1), so every lane holds the same sum,
// and each lane divides the elements it read: a lane writes only what it alone reads, so out == in is allowed.  A bad
// row (zero, NaN, Inf, overflowing norm) is written as +0.0f, counted, and the lowest bad row number kept -- with
// ordinary vector atomics, by lane 0.  The library is built with -ffp-contract=off: no product meets its sum in an FMA.
// (__fsqrt_rn is the native, 1-ulp square root in this toolchain; sqrtf is the correctly rounded one.)
//
// The kernel streams: 1M x 128 rows move 1 GB.  It is exact, and one launch in front of a batch; it is not tuned.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_buf.h"
#include "host_normalize.h"

namespace cph {

// in: row i at in + i * in_stride, out likewise (strides in floats, >= dim); bad_count / first_bad may be null.
__global__ __launch_bounds__(256) void normalize_rows_kernel(const float* in, float* out, uint64_t n, uint32_t dim, uint32_t in_stride,
                                                             uint32_t out_stride, unsigned long long* bad_count,
                                                             unsigned long long* first_bad) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t row = (uint64_t)blockIdx.x * 4 + wave; row < n; row += (uint64_t)gridDim.x * 4) {
        const float* x = in + row * in_stride;
        float* o = out + row * out_stride;
        float p = 0.0f;
        for (uint32_t j = lane; j < dim; j += 64) {
            const float v = x[j];
            p = __fadd_rn(p, __fmul_rn(v, v));
        }
        for (int d = 32; d >= 1; d >>= 1) p = __fadd_rn(p, __shfl_xor(p, d, 64));
        const float t = sqrtf(__fadd_rn(p, p));
        const bool good = t > 0.0f && t < __builtin_inff();
        for (uint32_t j = lane; j < dim; j += 64) o[j] = good ? __fdiv_rn(x[j], t) : 0.0f;
        if (!good && lane == 0) {
            if (bad_count) atomicAdd(bad_count, 1ull);
            if (first_bad) atomicMin(first_bad, (unsigned long long)row);
        }
    }
}

// Enqueues the normalisation of n rows on `st`; the counters (when given) must hold 0 and kNoBadRow before it runs.
inline void normalize_rows(const float* in, float* out, uint64_t n, uint32_t dim, uint32_t in_stride, uint32_t out_stride,
                           unsigned long long* bad_count, unsigned long long* first_bad, hipStream_t st) {
    if (n == 0 || dim == 0) return;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 3) / 4, 256u * 32u);
    hipLaunchKernelGGL(normalize_rows_kernel, dim3(grid), dim3(256), 0, st, in, out, n, dim, in_stride, out_stride, bad_count, first_bad);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
