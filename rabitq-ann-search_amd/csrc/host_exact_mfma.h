// host_exact_mfma.h — the slack of the matrix-core prefilter of the exact scan (device_exact_mfma.h), stated once for the
// host and the device.  cph_host_exact_matrix_slack exports it; tests/test_exact_matrix_host.py checks it against float64.
//
// exact_matrix_slack(qnorm, bn_max, D) >= |d^ - d| for every pair (query q, row b) with norm_sq[b] <= bn_max, where
//   d   the distance of the eight-chain path (device_exact.h): dot = eight fmaf chains of D / 8 terms from 0 and the 3-add
//       tree, d = max((qnorm + norm_sq) - 2 dot, 0);
//   d^  the prefilter's: s = one chain of D products that starts at -norm_sq / 2, each product rounded at most twice (fused
//       or not), d^ = max(fma(-2, s, qnorm), 0).
// The derivation is in the header comment of device_exact_mfma.h.
#pragma once
#include <cfloat>
#include <cstdint>

#if defined(__HIPCC__)
#define CPH_EXACT_MFMA_HD __host__ __device__
#else
#define CPH_EXACT_MFMA_HD
#endif

namespace cph {

// Roundings a product can pass through on both paths together, plus the roundings of the final expressions and the
// second-order terms: 2 (2 D + 2) + (D / 8 + 3) + 5 and a margin of 12 (see device_exact_mfma.h).
CPH_EXACT_MFMA_HD inline float exact_matrix_slack_terms(uint32_t D) { return __builtin_fmaf(4.125f, (float)D, 24.0f); }

// c (u N + FLT_MIN (1 + N)), rounded outward: the unit roundoff is taken a little large (0x1.0002p-24), which pays for the
// roundings of this expression itself and absorbs FLT_MIN N; the FLT_MIN term covers products and sums in or below the
// subnormal range, flushed or not (at most c FLT_MIN (1 + N) / 2 on both paths together: sum |x_i| <= (D + |x|^2) / 2).
// One dependent chain of operations on purpose: nothing here can be paired into a packed instruction.
CPH_EXACT_MFMA_HD inline float exact_matrix_slack(float qnorm, float bn_max, uint32_t D) {
    const float c = exact_matrix_slack_terms(D);
    const float N = qnorm + bn_max;
    return c * __builtin_fmaf(0x1.0002p-24f, N, FLT_MIN);
}

// The limit of the range search's prefilter (device_range_mfma.h) for a query of radius `radius` and slack `eps`: a pair
// is DISCARDED iff its approximate distance d^ is finite and d^ >= lim; everything else survives and is re-scored.
//   d^ >= lim >= radius + eps  =>  d >= d^ - eps >= radius: the pair is not a hit (a hit is d < radius, strict).
//   NaN radius or radius <= 0: -1.  No distance (>= +0, or NaN) is < radius, so nothing need survive.
//   eps not finite (and with it a qnorm that is not): NaN.  No comparison discards anything; the vector arithmetic answers.
//   Otherwise (radius + eps) * (1 + 2^-22): the sum rounds to nearest, within one ulp below the real sum, and the factor
//   gives two (the rounding-up of mx_limit).  +inf stays +inf, and a finite d^ is never >= it.
// cph_host_range_matrix_limit exports it; tests/test_range_matrix_host.py checks lim >= radius + eps in exact rationals.
CPH_EXACT_MFMA_HD inline float range_matrix_limit(float radius, float eps) {
    if (!(radius > 0.0f)) return -1.0f;
    if (!(__builtin_fabsf(eps) <= FLT_MAX)) return __builtin_nanf("");
    return (radius + eps) * 0x1.000004p+0f;
}

}  // namespace cph
