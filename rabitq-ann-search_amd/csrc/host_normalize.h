// host_normalize.h — the host statement of the cosine metric's row normalisation (device_normalize.h holds the kernel):
// no HIP call, so the CPU tests build this file with plain g++ under sanitizers.  Build it with -ffp-contract=off: every
// product and every sum below is rounded on its own.
//
// out = x / sqrt(2 |x|^2), so |out|^2 = 1/2 and || q~ - x~ ||^2 = 1 - cos(q, x): the squared-L2 kernels report the
// cosine distance of rows and queries stored this way.  The order of operations is fixed to the bit (fp32 throughout):
//     p_l  = +0;  for j = l, l + 64, l + 128, ... < dim:  p_l = p_l + (x[j] * x[j])          l = 0..63, the wave's lanes
//     s    = butterfly over the 64 p_l, xor distances 32, 16, 8, 4, 2, 1:  p_l = p_l + p_(l ^ d)   (every lane ends with s)
//     t    = sqrt(s + s);   out[j] = x[j] / t                                                 sqrt and / correctly rounded
// A row is bad when !(t > 0 && t < inf) -- a zero row, a NaN or Inf in it, a norm that overflows: all its outputs are
// +0.0f, it is counted, and the lowest bad row number is kept (kNoBadRow when there is none).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

namespace cph {

constexpr uint64_t kNoBadRow = ~0ull;

// The scale of one row: t above (NaN, 0 or inf for a bad row).
inline float normalize_scale_host(const float* x, uint32_t dim) {
    float p[64], q[64];
    for (uint32_t l = 0; l < 64; ++l) p[l] = 0.0f;
    for (uint32_t j = 0; j < dim; ++j) {
        const float sq = x[j] * x[j];
        p[j & 63] = p[j & 63] + sq;
    }
    for (uint32_t d = 32; d >= 1; d >>= 1) {
        for (uint32_t l = 0; l < 64; ++l) q[l] = p[l] + p[l ^ d];
        for (uint32_t l = 0; l < 64; ++l) p[l] = q[l];
    }
    return std::sqrt(p[0] + p[0]);
}

// x, out: [n][dim] (out == x allowed); bad_count / first_bad may be null.
inline void normalize_rows_host(const float* x, uint64_t n, uint32_t dim, float* out, uint64_t* bad_count, uint64_t* first_bad) {
    uint64_t bad = 0, first = kNoBadRow;
    for (uint64_t i = 0; i < n; ++i) {
        const float* r = x + i * dim;
        float* o = out + i * dim;
        const float t = normalize_scale_host(r, dim);
        if (t > 0.0f && t < std::numeric_limits<float>::infinity()) {
            for (uint32_t j = 0; j < dim; ++j) o[j] = r[j] / t;
        } else {
            for (uint32_t j = 0; j < dim; ++j) o[j] = 0.0f;
            ++bad;
            if (first == kNoBadRow) first = i;
        }
    }
    if (bad_count) *bad_count = bad;
    if (first_bad) *first_bad = first;
}

}  // namespace cph
