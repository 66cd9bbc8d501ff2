// host_ip.h — the host statement of the inner-product metric's arithmetic (device_ip.h holds the kernels): no HIP call,
// so the CPU tests build this file with plain g++ under sanitizers.  Build it with -ffp-contract=off: every product,
// sum and difference below is rounded on its own.
//
// With M2 >= max_i |x_i|^2 the index stores x~ = [x, sqrt(M2 - |x|^2)] (dim + 1 coordinates) and searches q~ = [q, 0]:
// |q~ - x~|^2 = |q|^2 + M2 - 2 q.x falls as q.x grows, so the squared-L2 kernels rank by inner product as they stand,
// and score = -(q.x) = 0.5 * (d - (|q|^2 + M2)) is recovered behind them.  The order of operations (fp32 throughout):
//     p_l  = +0;  for j = l, l + 64, l + 128, ... < dim:  p_l = p_l + (x[j] * x[j])          l = 0..63, the wave's lanes
//     s    = butterfly over the 64 p_l, xor distances 32, 16, 8, 4, 2, 1:  p_l = p_l + p_(l ^ d)   (the cosine metric's sum)
//     row:    out[0..dim) = x (the bits),  out[dim] = sqrt(M2 - s)                             sqrt correctly rounded
//     query:  out[0..dim) = q (the bits),  out[dim] = +0,  c = s + M2
//     score:  dist = 0.5 * (dist - c)  wherever id >= 0;  a padding entry (id < 0) keeps its bytes
// A vector is bad when !(s < inf) -- a NaN or Inf in it, a norm that overflows; a row is over the bound when s > M2.
// Such a row is written as dim + 1 times +0.0f and counted (bad rows and over-bound rows apart), and the lowest number
// of a row of either kind is kept (kIpNoRow when there is none).  A bad query is written as the zero vector with
// c = M2.  A zero vector is good.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

namespace cph {

constexpr uint64_t kIpNoRow = ~0ull;

// s above (NaN or inf for a bad vector).
inline float ip_sq_norm_host(const float* x, uint32_t dim) {
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
    return p[0];
}

// The largest s over the good rows of x [n][dim] (+0 when there is none); counters[0] += bad rows, counters[2] = the
// lowest bad row when it is lower.  counters = {bad, over, first}; may be null.
inline float ip_max_sq_norm_host(const float* x, uint64_t n, uint32_t dim, uint64_t* counters) {
    float m2 = 0.0f;
    for (uint64_t i = 0; i < n; ++i) {
        const float s = ip_sq_norm_host(x + i * dim, dim);
        if (s < std::numeric_limits<float>::infinity()) {
            if (s > m2) m2 = s;
        } else if (counters) {
            ++counters[0];
            if (i < counters[2]) counters[2] = i;
        }
    }
    return m2;
}

// x [n][dim] -> out [n][dim + 1] (not in place).  c == null: rows; otherwise queries, and c [n] is written.
// counters = {bad, over, first} are added to / lowered; may be null.
inline void ip_augment_host(const float* x, uint64_t n, uint32_t dim, float m2, float* out, float* c, uint64_t* counters) {
    for (uint64_t i = 0; i < n; ++i) {
        const float* r = x + i * dim;
        float* o = out + i * (uint64_t)(dim + 1);
        const float s = ip_sq_norm_host(r, dim);
        const bool bad = !(s < std::numeric_limits<float>::infinity());
        const bool over = !bad && !c && s > m2;
        if (bad || over) {
            for (uint32_t j = 0; j <= dim; ++j) o[j] = 0.0f;
            if (c) c[i] = m2;
            if (counters) {
                ++counters[bad ? 0 : 1];
                if (i < counters[2]) counters[2] = i;
            }
            continue;
        }
        std::memcpy(o, r, (size_t)dim * sizeof(float));
        if (c) {
            o[dim] = 0.0f;
            c[i] = s + m2;
        } else {
            o[dim] = std::sqrt(m2 - s);
        }
    }
}

// The scores of a [n][k] result table, in place.
inline void ip_epilogue_host(const int64_t* ids, float* dist, uint64_t n, uint64_t k, const float* c) {
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t j = 0; j < k; ++j)
            if (ids[i * k + j] >= 0) dist[i * k + j] = 0.5f * (dist[i * k + j] - c[i]);
}

}  // namespace cph
