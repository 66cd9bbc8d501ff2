// host_maxsim_all.h — the bound of the exhaustive MaxSim pass (cph_search_maxsim_all; device_maxsim_all.h holds the kernels),
// stated once for the host and the device.  cph_host_maxsim_all_term exports the term; tests/test_maxsim_all_host.py checks
// it in exact rationals.
//
// For query i, live token t and a key with at least one allowed row (an id < cph_size with that key whose bit is set in the
// query's effective filter):
//     d^(t, row)  the prefilter distance of device_exact_mfma.h: one chain from -|b|^2 / 2, then max(fma(-2, s, qn), 0)
//     eps_t       exact_matrix_slack(qnorm_t, bn_max, D) >= |d^ - d| for every row, d having the bytes of exact_l2
//     m^_t        min over the key's allowed rows of d^(t, row)
//     l_t         maxsim_all_term(m^_t, eps_t) <= max(m^_t - eps_t, 0) <= min over the allowed rows of d(t, row):
//                 every d^ is within eps_t of its d, so m^_t - eps_t <= d^(r) - eps_t <= d(r) for every allowed row r, and
//                 d >= +0
//     lb          ((+0.0f + l_0) + l_1) + ... in float32, in token order
// lb <= score.  score(key) of the rescoring statement (host_maxsim_rescore.h) is the same left-to-right float32 sum over
// dmin_t = min d(t, row) >= l_t.  Round-to-nearest addition is monotone in both operands (a <= a', b <= b' gives
// fl(a + b) <= fl(a' + b'): rounding never reorders two reals), so by induction over t every partial sum of lb is <= the
// partial sum of score.  Hence a key outside the R smallest (lb, key) has score >= lb >= lb_{R-1}, over the WHOLE index.
//
// The term.  x = fl(m^ - eps) may round UP past the real difference y; x <= y (1 + u), u = 2^-24, when x is normal and
// x == y when x < 2^-125 (both operands are multiples of 2^-149).  l = fl(x (1 - 2^-22)):
//     x >= 2^-125:  l <= x (1 - 4 u) (1 + u) <= y (1 + u)^2 (1 - 4 u) < y;
//     x <  2^-125:  x == y, and rounding is monotone: l <= fl(x) = y.
// x <= 0 or NaN (eps not finite: the query is "unbounded" anyway) gives +0.0f, a bound of every distance.
//
// How tight.  m^_t >= dmin_t - eps_t, so l_t >= (dmin_t - 2 eps_t) (1 - u) (1 - 4 u) (1 - u) >= dmin_t - 2 eps_t - 6 u dmin_t
// (or l_t = 0 >= dmin_t - 2 eps_t).  Each of the at most T additions of either sum has relative error u, so with
// S = sum_t dmin_t <= score / (1 - T u):
//     score - lb <= sum_t 2 eps_t + (6 + 2 T) u S
// which tests/test_gpu_maxsim_all.py computes from cph_host_exact_matrix_slack and asserts.
//
// Queries that cannot be bounded (qnorm, eps or bn_max not finite, or some d^ of an allowed row not finite) get lb = +0.0f
// for every key with an allowed row: still a true bound; certified comes out 0 by the rule of the rescoring statement.
#pragma once
#include <algorithm>
#include <cstdint>

#include "host_exact_mfma.h"

namespace cph {

CPH_EXACT_MFMA_HD inline float maxsim_all_term(float m_hat, float eps) {
    const float x = m_hat - eps;
    if (!(x > 0.0f)) return 0.0f;
    return x * 0x1.fffff8p-1f;
}

// The word of the bound table for a (query, key) without an allowed row; every bound is the bits of a float >= +0.
constexpr uint32_t kMaxsimAllNone = 0xFFFFFFFFu;

// T rounded up to 1, 2, 4, ..., 64: the rows a query takes in a 128-row tile (128 / Tp whole queries per tile).
inline uint32_t maxsim_all_padded_tokens(uint32_t T) {
    uint32_t tp = 1;
    while (tp < T) tp <<= 1;
    return tp;
}

// How a call is cut: chunks of `chunk` queries whose bound table [chunk][n_keys] floats fits `budget` bytes (at least one
// query), each a grid of P parts x tiles of 128 / Tp queries.  Parts are `part` columns of the inverted key column (a multiple
// of 128), moved to key boundaries by the workgroups themselves (a bisection of offsets[]): two workgroups per CU are asked
// for, as in plan_range_matrix.
struct MaxsimAllPlan {
    uint32_t Tp, chunk, P;
    uint64_t part;
};

inline MaxsimAllPlan plan_maxsim_all(uint64_t size, uint64_t n_keys, uint64_t n, uint32_t T, int num_cus, uint64_t budget) {
    MaxsimAllPlan pl{};
    pl.Tp = maxsim_all_padded_tokens(T);
    pl.chunk = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, budget / (std::max<uint64_t>(n_keys, 1) * 4)));
    pl.chunk = (uint32_t)std::min<uint64_t>(pl.chunk, 65535ull * 128 / pl.Tp);          // (tiles of a chunk: the grid's y)
    const uint64_t wgs = (uint64_t)std::max(1, num_cus) * 2, blocks = std::max<uint64_t>(1, (size + 127) / 128);
    const uint64_t tiles = ((uint64_t)pl.chunk * pl.Tp + 127) / 128;
    const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>({(wgs + tiles - 1) / tiles, blocks, (uint64_t)65535}));
    pl.part = (blocks + want - 1) / want * 128;
    pl.P = (uint32_t)((size + pl.part - 1) / pl.part);
    if (pl.P == 0) pl.P = 1;
    return pl;
}

}  // namespace cph
