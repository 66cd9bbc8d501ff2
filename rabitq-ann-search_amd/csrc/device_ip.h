// device_ip.h — the inner-product metric's kernels: one in front of the squared-L2 kernels and one behind them.
// With M2 >= max |x|^2 a row is stored as x~ = [x, sqrt(M2 - |x|^2)] and a query searched as q~ = [q, 0]; then
// |q~ - x~|^2 = |q|^2 + M2 - 2 q.x, every search of the library ranks by inner product as it stands, and the epilogue
// turns each distance into score = -(q.x) = 0.5 * (d - (|q|^2 + M2)).  host_ip.h states the arithmetic, bit for bit.
//
// Rows / queries: one wave per row, four waves per workgroup, grid-stride over the rows.  Lane l sums the squares of
// elements l, l + 64, ... (coalesced loads), the wave reduces with a xor butterfly (32, 16, 8, 4, 2, 1) -- the cosine
// kernel's sum, restated here so that device_normalize.h keeps its code -- and each lane copies the elements it read;
// lane 0 writes the extra coordinate.  The input stride is dim, the output stride dim + 1: not in place.  A bad vector
// (NaN, Inf, overflowing norm) or a row over the bound is written as zeros and counted with ordinary vector atomics, by
// lane 0.  ip_max_kernel is the pass in front when M2 comes from the data: s is a non-negative finite float, so an
// unsigned max on its bits orders it.  The library is built with -ffp-contract=off: no product meets its sum in an FMA.
//
// Epilogue: one thread per entry of the [n][k] table, grid-stride; plain loads and stores, so the tables may be device
// memory or pinned, device-mapped host memory.
//
// All three stream; they are not tuned beyond coalescing.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_buf.h"
#include "host_ip.h"

namespace cph {

// s of the wave's row: every lane returns the same value.
__device__ __forceinline__ float ip_wave_sq_norm(const float* x, uint32_t dim, uint32_t lane) {
    float p = 0.0f;
    for (uint32_t j = lane; j < dim; j += 64) {
        const float v = x[j];
        p = __fadd_rn(p, __fmul_rn(v, v));
    }
    for (int d = 32; d >= 1; d >>= 1) p = __fadd_rn(p, __shfl_xor(p, d, 64));
    return p;
}

// counters = {bad rows, rows over the bound, lowest row of either kind}; row numbers are row_base + the row here.
__device__ __forceinline__ void ip_count_row(unsigned long long* counters, int kind, uint64_t row) {
    if (!counters) return;
    atomicAdd(counters + kind, 1ull);
    atomicMin(counters + 2, (unsigned long long)row);
}

// m2_bits: the bits of the largest s over the good rows (starts as 0 = +0.0f); bad rows are counted.
__global__ __launch_bounds__(256) void ip_max_kernel(const float* in, uint64_t n, uint32_t dim, uint64_t row_base, unsigned int* m2_bits,
                                                     unsigned long long* counters) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t row = (uint64_t)blockIdx.x * 4 + wave; row < n; row += (uint64_t)gridDim.x * 4) {
        const float s = ip_wave_sq_norm(in + row * dim, dim, lane);
        if (lane != 0) continue;
        if (s < __builtin_inff()) atomicMax(m2_bits, __float_as_uint(s));
        else ip_count_row(counters, 0, row_base + row);
    }
}

// in [n][dim] -> out [n][dim + 1].  c == null: rows (out[dim] = sqrt(m2 - s); s > m2 is over the bound); otherwise
// queries (out[dim] = +0, c[row] = s + m2; a bad query is the zero vector with c = m2).
__global__ __launch_bounds__(256) void ip_augment_kernel(const float* in, float* out, uint64_t n, uint32_t dim, float m2, uint64_t row_base,
                                                         float* c, unsigned long long* counters) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint64_t row = (uint64_t)blockIdx.x * 4 + wave; row < n; row += (uint64_t)gridDim.x * 4) {
        const float* x = in + row * dim;
        float* o = out + row * ((uint64_t)dim + 1);
        const float s = ip_wave_sq_norm(x, dim, lane);
        const bool bad = !(s < __builtin_inff());
        const bool over = !bad && !c && s > m2;
        const bool good = !bad && !over;
        for (uint32_t j = lane; j < dim; j += 64) o[j] = good ? x[j] : 0.0f;
        if (lane != 0) continue;
        if (c) {
            o[dim] = 0.0f;
            c[row] = good ? __fadd_rn(s, m2) : m2;
        } else {
            o[dim] = good ? sqrtf(__fsub_rn(m2, s)) : 0.0f;
        }
        if (!good) ip_count_row(counters, bad ? 0 : 1, row_base + row);
    }
}

// dist[i][j] = 0.5 * (dist[i][j] - c[i]) wherever ids[i][j] >= 0; padding entries keep their bytes.  total = n * k.
__global__ __launch_bounds__(256) void ip_epilogue_kernel(const int64_t* ids, float* dist, uint64_t total, uint32_t k, const float* c) {
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
        if (ids[e] < 0) continue;
        dist[e] = __fmul_rn(0.5f, __fsub_rn(dist[e], c[e / k]));
    }
}

inline uint32_t ip_row_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + 3) / 4, 256u * 32u); }

// Enqueue on `st`.  m2_bits must hold 0 and the counters (when given) {0, 0, kIpNoRow} before the first launch that
// adds to them.
inline void ip_max(const float* in, uint64_t n, uint32_t dim, uint64_t row_base, unsigned int* m2_bits, unsigned long long* counters,
                   hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(ip_max_kernel, dim3(ip_row_grid(n)), dim3(256), 0, st, in, n, dim, row_base, m2_bits, counters);
    HIP_CHECK(hipGetLastError());
}

inline void ip_augment(const float* in, float* out, uint64_t n, uint32_t dim, float m2, uint64_t row_base, float* c,
                       unsigned long long* counters, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(ip_augment_kernel, dim3(ip_row_grid(n)), dim3(256), 0, st, in, out, n, dim, m2, row_base, c, counters);
    HIP_CHECK(hipGetLastError());
}

inline void ip_epilogue(const int64_t* ids, float* dist, uint64_t n, uint32_t k, const float* c, hipStream_t st) {
    const uint64_t total = n * k;
    if (total == 0) return;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((total + 255) / 256, 256u * 32u);
    hipLaunchKernelGGL(ip_epilogue_kernel, dim3(grid), dim3(256), 0, st, ids, dist, total, k, c);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
