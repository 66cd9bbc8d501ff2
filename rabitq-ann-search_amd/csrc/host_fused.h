// host_fused.h — the host statement of fused search (cph_search_fused; device_fused.h holds the kernels): several query vectors
// per query, one ranked list of rows by the exact weighted sum of their distances.  No HIP call, so the CPU tests build this
// file with plain g++ under sanitizers.  Build it with -ffp-contract=off: a score is separately rounded products and sums.
//
// Query i has T vectors of which the first L = n_vectors[i] are live (1 <= L <= T; null: T) and weights w[i][0 .. T), float32,
// finite, any sign.  Its input is the T candidate rows [C] an ordinary search at k = C returned for its vectors, in internal
// ids, padded with -1; the distances of that search are used for nothing.
//     candidates   the DISTINCT ids x, 0 <= x < n_ids, that occur in the rows of the live vectors
//     hits(x)      the number of live vectors whose row holds x (repeats inside one row count once)
//     d_t(x)       the bits cph_exact_l2 returns for query = vector t as the search saw it and id = x (host_diverse.h:
//                  diverse_dot8 / diverse_exact_from_dot over the zero-padded rows; qnorm the same chains over q_t * q_t, norm =
//                  norm_sq[x]), for EVERY live t, whether or not t's row held x
//     score(x)     s = +0.0f; for t = 0 .. L - 1 in this order: s = s + (w[i][t] * d_t(x)), the product and the sum each rounded
//                  once.  s is never -0.0 (+0 + -0 = +0, x + -x = +0).  A candidate whose s is a NaN is dropped: only
//                  +inf + -inf, that is overflow under weights of both signs, makes one.
// The answer: the min(k, candidates left) candidates with the smallest (s as a float, internal id), with their score and
// hits; ids through the row map where one is given.  Padding: id -1, score FLT_MAX, hits 0.  Every slot is written.
// The order of s is taken on its monotone key (fused_orderable: the usual sign flip of the bits), which is value order for
// everything but a NaN.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "host_diverse.h"
#include "host_maxsim.h"

namespace cph {

// The limits are MaxSim's: the union of a query is sorted in LDS by the sort of device_maxsim.h.
constexpr uint32_t kFusedMaxVectors = kMaxsimMaxTokens;            // T <= this
constexpr uint32_t kFusedMaxCandidates = kMaxsimMaxCandidates;     // C <= this
constexpr uint32_t kFusedMaxEntries = kMaxsimMaxEntries;           // T * C <= this
constexpr uint32_t kFusedMaxK = kMaxsimMaxK;                       // k <= min(this, T * C)

inline uint32_t fused_orderable_host(float s) {
    uint32_t u;
    std::memcpy(&u, &s, 4);
    return u ^ ((u & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
}

// cand_ids [n][T][C]; weights [n][T] or null: every weight is 1; qpad [n][T][D]: the vectors as the search saw them, zero-padded
// to D; raw [n_ids][D] zero-padded, norm_sq [n_ids]; rows (may be null): ids are written as rows[id].
inline void fused_rows_host(const int64_t* cand_ids, uint64_t n, uint32_t T, const int32_t* n_vectors, const float* weights, uint32_t C,
                            const float* qpad, const float* raw, const float* norm_sq, uint64_t n_ids, uint32_t D, const uint32_t* rows,
                            uint32_t k, int64_t* out_ids, float* out_score, int32_t* out_hits) {
    const float fmax = FLT_MAX;
    struct Cand { uint32_t key; uint32_t id; float score; int32_t hits; };
    std::map<uint32_t, uint64_t> seen;            // id -> the live vectors whose row holds it (T <= 64: one bit each)
    std::vector<Cand> order;
    std::vector<float> qn(T);
    for (uint64_t q = 0; q < n; ++q) {
        const uint32_t L = n_vectors ? (uint32_t)n_vectors[q] : T;
        const float* qv = qpad + q * T * D;
        seen.clear();
        for (uint32_t t = 0; t < L; ++t) {
            qn[t] = diverse_dot8(qv + (size_t)t * D, qv + (size_t)t * D, D);
            for (uint32_t j = 0; j < C; ++j) {
                const int64_t id = cand_ids[(q * T + t) * C + j];
                if (id >= 0 && (uint64_t)id < n_ids) seen[(uint32_t)id] |= 1ull << t;
            }
        }
        order.clear();
        for (const auto& e : seen) {
            const uint32_t id = e.first;
            float s = 0.0f;
            for (uint32_t t = 0; t < L; ++t) {
                const float d = diverse_exact_from_dot(qn[t], norm_sq[id], diverse_dot8(qv + (size_t)t * D, raw + (size_t)id * D, D));
                const float w = weights ? weights[q * T + t] : 1.0f;
                const float p = w * d;
                s = s + p;
            }
            if (s != s) continue;
            order.push_back(Cand{fused_orderable_host(s), id, s, (int32_t)__builtin_popcountll(e.second)});
        }
        std::sort(order.begin(), order.end(), [](const Cand& a, const Cand& b) { return a.key != b.key ? a.key < b.key : a.id < b.id; });
        for (uint32_t o = 0; o < k; ++o) {
            const size_t at = q * k + o;
            if (o < order.size()) {
                const Cand& c = order[o];
                out_ids[at] = rows ? (int64_t)rows[c.id] : (int64_t)c.id;
                std::memcpy(out_score + at, &c.score, 4);
                out_hits[at] = c.hits;
            } else {
                out_ids[at] = -1;
                std::memcpy(out_score + at, &fmax, 4);
                out_hits[at] = 0;
            }
        }
    }
}

}  // namespace cph
