// host_knn.h — the host statement of the exact 32-nearest-neighbour kernels (device_knn.h: knn_mfma_kernel, the "two-pass"
// kernel; device_knn_sym.h: the symmetric self-join).  No HIP call, so the CPU tests build this file with plain g++ under
// sanitizers.  Build it with -ffp-contract=off: every fused multiply-add below is a std::fmaf and stands where the kernels
// have one.
//
// v_mfma_f32_32x32x2_f32 is bit for bit a k-ordered fmaf chain, so everything the kernels compute can be said in scalar
// float32 arithmetic and their outputs compared byte for byte, ids included.
//
//   rows      zero padded to D = max(32, next power of two >= dim) floats (cph_knn_bruteforce pads to the power of two, the
//             builder to the K chunk of 32)
//   norm      |x|^2 = one chain s = fmaf(x[j], x[j], s) over j = 0 .. dim - 1 in index order, from +0
//   k order   the dot products are NOT summed in index order.  A chunk of 32 floats is four steps j of eight; lane half h of a
//             wave reads k = 8j + 4h .. 8j + 4h + 3 and feeds the four values to four consecutive MFMAs (.x .y .z .w), each of
//             which adds the product of lane half 0 and then that of lane half 1.  Inside every group of eight coordinates the
//             order is therefore 0, 4, 1, 5, 2, 6, 3, 7 (knn_k_order)
//   two-pass  key s(q, b) = the chain over all D coordinates in k order, started at -0.5f * norm(b).  Row i's answer: the
//             columns b != self(i) whose key is greater than -inf (a NaN never is), ranked by (s descending, id ascending), the
//             first 32; d = norm(q) - 2 s rounded once, negative values replaced by +0.  self(i) = i for a self-join, q_ids[i]
//             for gathered rows, nothing otherwise.  Padding: id 0xFFFFFFFF, distance FLT_MAX
//   join      seed: the two-pass answer of every row against the rows 0, 16, 32, ... (nothing excluded); tau[r] = its 8th
//             distance, the 9th when r is itself a sample row.  Pair value: acc = the chain in k order from +0,
//             dd(r, c) = fmaf(-2, acc, norm[r] + norm[c]) -- symmetric in r and c.  Column c != r is a candidate of row r if
//             dd <= tau[r].  A row with 32 .. 256 candidates lists the first 32 by (max(dd, +0) ascending, id ascending); any
//             other row takes the two-pass answer against every row (self excluded) and is counted as a fallback row
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <vector>

#include "host_parallel.h"

namespace cph {

constexpr uint32_t kHostKnnK = 32;            // = kKnnK
constexpr uint32_t kHostKnnChunk = 32;        // = kKnnKC
constexpr uint32_t kHostKnnSymSample = 16;    // = kKnnSymSample
constexpr uint32_t kHostKnnSymRank = 8;       // = kKnnSymRank
constexpr uint32_t kHostKnnSymCap = 256;      // = kKnnSymCap
constexpr uint64_t kHostKnnJoinMaxRows = 4096;    // the join model keeps an n x n table of pair values

// The t-th fmaf of a chain takes this coordinate.
inline uint32_t knn_k_order(uint32_t t) {
    constexpr uint32_t in8[8] = {0, 4, 1, 5, 2, 6, 3, 7};
    return (t & ~7u) | in8[t & 7u];
}

inline uint64_t knn_padded_dim(uint64_t dim) {
    uint64_t D = kHostKnnChunk;
    while (D < dim) D *= 2;
    return D;
}

// The conditions under which the builder takes the join at all (builder.h: knn_sym_wanted without its size limit): a
// self-join whose sample holds at least 64 rows, more than one K chunk per tile.  The debug entry adds n >= 1024.
inline bool knn_join_possible(uint64_t n, uint64_t D) {
    return n / kHostKnnSymSample >= 64 && D >= 2 * kHostKnnChunk && n < (1ull << 31);
}

// src[rows][dim] -> x[rows][D] zero padded, nrm[rows] (what cph_knn_bruteforce hands to the kernels)
inline void knn_pad_rows(const float* src, uint64_t rows, uint64_t dim, uint64_t D, std::vector<float>& x, std::vector<float>& nrm) {
    x.assign(rows * D, 0.0f);
    nrm.resize(rows);
    for (uint64_t i = 0; i < rows; ++i) {
        std::memcpy(&x[i * D], src + i * dim, dim * 4);
        float s = 0.0f;
        for (uint64_t j = 0; j < dim; ++j) s = std::fmaf(x[i * D + j], x[i * D + j], s);
        nrm[i] = s;
    }
}

// x[rows][D] -> the same rows with their coordinates in the order the chains take them
inline std::vector<float> knn_in_k_order(const float* x, uint64_t rows, uint32_t D) {
    std::vector<float> p(rows * D);
    for (uint64_t i = 0; i < rows; ++i)
        for (uint32_t t = 0; t < D; ++t) p[i * D + t] = x[i * D + knn_k_order(t)];
    return p;
}

inline float knn_chain(const float* a, const float* b, uint32_t D, float acc) {
    for (uint32_t t = 0; t < D; ++t) acc = std::fmaf(a[t], b[t], acc);
    return acc;
}

// The two-pass kernel.  qk / bk: rows in k order (knn_in_k_order).  self: 0 = nothing excluded, 1 = row i excludes column
// q_ids[i], or column i where q_ids is null.
inline void knn_two_pass_host(const float* qk, const float* qnorm, uint64_t nq, const float* bk, const float* bnorm, uint64_t nb, uint32_t D,
                              bool exclude_self, const uint32_t* q_ids, uint32_t* out_ids, float* out_dist) {
    struct Entry { float s; uint32_t id; };
    const float neg_inf = -std::numeric_limits<float>::infinity();
    parallel_for(nq, 1, [&](size_t lo, size_t hi) {
        std::vector<Entry> pass;
        for (size_t i = lo; i < hi; ++i) {
            const uint32_t self = q_ids ? q_ids[i] : (uint32_t)i;
            pass.clear();
            for (uint64_t c = 0; c < nb; ++c) {
                if (exclude_self && c == self) continue;
                const float s = knn_chain(qk + i * D, bk + c * D, D, -0.5f * bnorm[c]);
                if (s > neg_inf) pass.push_back({s, (uint32_t)c});
            }
            const size_t keep = std::min<size_t>(pass.size(), kHostKnnK);
            std::partial_sort(pass.begin(), pass.begin() + keep, pass.end(),
                              [](const Entry& a, const Entry& b) { return a.s > b.s || (a.s == b.s && a.id < b.id); });
            for (size_t j = 0; j < kHostKnnK; ++j) {
                float d = FLT_MAX;
                if (j < keep) {
                    d = qnorm[i] - 2.0f * pass[j].s;
                    d = d > 0.0f ? d : 0.0f;
                }
                out_ids[i * kHostKnnK + j] = j < keep ? pass[j].id : 0xFFFFFFFFu;
                out_dist[i * kHostKnnK + j] = d;
            }
        }
    });
}

// The symmetric self-join.  xk: rows in k order.  Returns the number of fallback rows; cand_count (may be null) receives
// every row's number of candidates.
inline uint32_t knn_join_host(const float* xk, const float* norm, uint64_t n, uint32_t D, uint32_t* out_ids, float* out_dist,
                              uint32_t* cand_count = nullptr) {
    if (!knn_join_possible(n, D) || n > kHostKnnJoinMaxRows) throw std::invalid_argument("knn_join_host: not a shape of the join");
    // 1. thresholds from the sample
    const uint64_t ns = (n + kHostKnnSymSample - 1) / kHostKnnSymSample;
    std::vector<float> sx(ns * D), sn(ns), sd(n * kHostKnnK), tau(n);
    std::vector<uint32_t> si(n * kHostKnnK);
    for (uint64_t s = 0; s < ns; ++s) {
        std::memcpy(&sx[s * D], xk + s * kHostKnnSymSample * D, (size_t)D * 4);
        sn[s] = norm[s * kHostKnnSymSample];
    }
    knn_two_pass_host(xk, norm, n, sx.data(), sn.data(), ns, D, false, nullptr, si.data(), sd.data());
    for (uint64_t r = 0; r < n; ++r) tau[r] = sd[r * kHostKnnK + kHostKnnSymRank - 1 + (r % kHostKnnSymSample == 0 ? 1 : 0)];
    // 2. every pair once
    std::vector<float> dd(n * n);
    parallel_for(n, 1, [&](size_t lo, size_t hi) {
        for (size_t r = lo; r < hi; ++r)
            for (uint64_t c = r; c < n; ++c) {
                const float acc = knn_chain(xk + r * D, xk + c * D, D, 0.0f);
                const float v = std::fmaf(-2.0f, acc, norm[r] + norm[c]);
                dd[r * n + c] = v;
                dd[c * n + r] = v;
            }
    });
    // 3. selection
    struct Entry { float d; uint32_t id; };
    std::vector<uint32_t> redo;
    std::vector<Entry> cand;
    for (uint64_t r = 0; r < n; ++r) {
        cand.clear();
        for (uint64_t c = 0; c < n; ++c) {
            const float v = dd[r * n + c];
            if (v <= tau[r] && c != r) cand.push_back({v > 0.0f ? v : 0.0f, (uint32_t)c});
        }
        if (cand_count) cand_count[r] = (uint32_t)cand.size();
        if (cand.size() < kHostKnnK || cand.size() > kHostKnnSymCap) {
            redo.push_back((uint32_t)r);
            continue;
        }
        std::partial_sort(cand.begin(), cand.begin() + kHostKnnK, cand.end(),
                          [](const Entry& a, const Entry& b) { return a.d < b.d || (a.d == b.d && a.id < b.id); });
        for (uint32_t j = 0; j < kHostKnnK; ++j) {
            out_ids[r * kHostKnnK + j] = cand[j].id;
            out_dist[r * kHostKnnK + j] = cand[j].d;
        }
    }
    // 4. fallback rows
    if (!redo.empty()) {
        const size_t m = redo.size();
        std::vector<float> rx(m * D), rn(m), rd(m * kHostKnnK);
        std::vector<uint32_t> ri(m * kHostKnnK);
        for (size_t i = 0; i < m; ++i) {
            std::memcpy(&rx[i * D], xk + (size_t)redo[i] * D, (size_t)D * 4);
            rn[i] = norm[redo[i]];
        }
        knn_two_pass_host(rx.data(), rn.data(), m, xk, norm, n, D, true, redo.data(), ri.data(), rd.data());
        for (size_t i = 0; i < m; ++i) {
            std::memcpy(out_ids + (size_t)redo[i] * kHostKnnK, &ri[i * kHostKnnK], kHostKnnK * 4);
            std::memcpy(out_dist + (size_t)redo[i] * kHostKnnK, &rd[i * kHostKnnK], kHostKnnK * 4);
        }
    }
    return (uint32_t)redo.size();
}

// What both debug entries accept (cph_host_knn, cph_debug_knn): throws std::invalid_argument with the reason.
//   queries == null   the self-join of vectors[n][dim]; a row never lists itself; q_ids must be null
//   queries != null   queries[nq][dim] against vectors; exclude_self = 0: nothing excluded, q_ids must be null;
//                     exclude_self = 1: row i excludes column q_ids[i] (q_ids[nq], every entry < n)
//   path              0 = the two-pass kernel, 1 = the join (self-join only, n >= 1024, padded D >= 64)
inline void knn_debug_check(const float* vectors, uint64_t n, uint64_t dim, const float* queries, uint64_t nq, const uint32_t* q_ids,
                            int exclude_self, int path, const void* ids, const void* dist) {
    if (!vectors || !ids || !dist || n == 0 || dim == 0) throw std::invalid_argument("knn debug: bad arguments");
    if (n >= 0x7FFFFFFFull || nq >= 0x7FFFFFFFull || dim > 2048) throw std::invalid_argument("knn debug: sizes out of range");
    if (path != 0 && path != 1) throw std::invalid_argument("knn debug: path is 0 (two-pass) or 1 (join)");
    if (exclude_self != 0 && exclude_self != 1) throw std::invalid_argument("knn debug: exclude_self is 0 or 1");
    if (!queries) {
        if (q_ids || nq) throw std::invalid_argument("knn debug: q_ids and nq go with queries");
    } else {
        if (nq == 0) throw std::invalid_argument("knn debug: bad arguments");
        if ((exclude_self != 0) != (q_ids != nullptr)) throw std::invalid_argument("knn debug: exclude_self with queries needs q_ids, and q_ids needs exclude_self");
        for (uint64_t i = 0; q_ids && i < nq; ++i)
            if (q_ids[i] >= n) throw std::invalid_argument("knn debug: q_ids entry out of range");
    }
    if (path == 1 && (queries || n < 1024 || !knn_join_possible(n, knn_padded_dim(dim))))
        throw std::invalid_argument("knn debug: the join needs a self-join, n >= 1024 and padded D >= 64");
    if (path == 1 && n > kHostKnnJoinMaxRows) throw std::invalid_argument("knn debug: the join entry takes at most 4096 rows");
}

// The whole of cph_host_knn behind its argument checks (cand_count: the join's candidates per row, may be null).
inline uint32_t knn_host(const float* vectors, uint64_t n, uint64_t dim, const float* queries, uint64_t nq, const uint32_t* q_ids,
                         int path, uint32_t* ids, float* dist, uint32_t* cand_count = nullptr) {
    const uint32_t D = (uint32_t)knn_padded_dim(dim);
    std::vector<float> x, nrm, q, qn;
    knn_pad_rows(vectors, n, dim, D, x, nrm);
    const std::vector<float> xk = knn_in_k_order(x.data(), n, D);
    if (path == 1) return knn_join_host(xk.data(), nrm.data(), n, D, ids, dist, cand_count);
    if (!queries) {
        knn_two_pass_host(xk.data(), nrm.data(), n, xk.data(), nrm.data(), n, D, true, nullptr, ids, dist);
        return 0;
    }
    knn_pad_rows(queries, nq, dim, D, q, qn);
    const std::vector<float> qk = knn_in_k_order(q.data(), nq, D);
    knn_two_pass_host(qk.data(), qn.data(), nq, xk.data(), nrm.data(), n, D, q_ids != nullptr, q_ids, ids, dist);
    return 0;
}

}  // namespace cph
