// host_maxsim_rescore.h — the host statement of the exact rescoring stage of multi-vector search (cph_search_maxsim_rescored;
// device_maxsim_rescore.h holds the kernels): no HIP call, so the CPU tests build this file with plain g++ under sanitizers.
// Build it with -ffp-contract=off: a distance is separately rounded operations around eight FMA chains.
//
// Input: per query the f = cand_found <= R candidate keys of the lower-bound statement (host_maxsim.h at k = R) with their
// lower bounds lb_j, in (lb, key) order, and the query's T token rows of which the first L are live.
//     A_i(key)   the ids < n_ids with key_of[id] == key whose bit is set in query i's bitmap (no bitmap: every such id)
//     best_t     min over id in A_i(key) of (bits(d(q_t, id)) << 32 | id), unsigned; d has the bits cph_exact_l2 returns for the
//                pair (host_diverse.h: diverse_dot8 / diverse_exact_from_dot over the zero-padded rows; qnorm the same chains
//                over q_t * q_t, norm = norm_sq[id]); d >= +0, so bit order is value order and ties go to the lowest id
//     score      s = +0.0f; for t = 0 .. L - 1: s = s + d(best_t)         (float32, in that order)
// The answer: the min(k, f) candidates with the smallest (score bits, key as a signed int32), each with its score, hits = L
// and rows[t] = the id of best_t (through the row map where one is given), -1 for t >= L.  Padding: key 0, score FLT_MAX,
// hits 0, rows -1.  certified = the number of leading answer slots whose score is strictly below lb_{R-1} (as float
// values), or the number of answer slots when f < R: every key outside the candidates has a lower bound >= lb_{R-1}.
// A candidate without an allowed row (no search produces one) has best_t = all ones; its row is written as -1.
//
// key_rows_host is the inverted key column the kernels read: ids ordered by (key, id), the distinct keys ascending, and
// the offsets of every key's run.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstring>
#include <map>
#include <numeric>
#include <vector>

#include "host_diverse.h"

namespace cph {

constexpr uint32_t kMaxsimRescoreMax = 1024;        // R <= this

// keys [n] -> out_ids [n] (the ids by (key, id)), out_keys [<= n] (distinct, ascending), out_offsets [distinct + 1]
// (key u owns out_ids[out_offsets[u] .. out_offsets[u + 1])); returns the number of distinct keys.
inline uint64_t key_rows_host(const int32_t* keys, uint64_t n, uint32_t* out_ids, int32_t* out_keys, uint32_t* out_offsets) {
    std::iota(out_ids, out_ids + n, 0u);
    std::stable_sort(out_ids, out_ids + n, [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    uint64_t u = 0;
    for (uint64_t i = 0; i < n; ++i)
        if (i == 0 || keys[out_ids[i]] != keys[out_ids[i - 1]]) {
            out_keys[u] = keys[out_ids[i]];
            out_offsets[u++] = (uint32_t)i;
        }
    out_offsets[u] = (uint32_t)n;
    return u;
}

// tokens [n][T][dim] (what the search saw), raw [n_ids][D] zero-padded, allow [n][(n_ids + 31) / 32] or null.
inline void maxsim_rescore_host(const int32_t* cand_keys, const float* cand_lb, const int32_t* cand_found, uint64_t n, uint32_t R,
                                const float* tokens, uint32_t T, uint32_t dim, const int32_t* n_tokens, const float* raw,
                                const float* norm_sq, uint64_t n_ids, uint32_t D, const int32_t* key_of, const uint32_t* allow,
                                const uint32_t* rows, uint32_t k, int32_t* out_keys, float* out_score, int32_t* out_hits,
                                int64_t* out_rows, int32_t* out_found, int32_t* out_certified) {
    const float fmax = FLT_MAX;
    const uint64_t nw = (n_ids + 31) / 32;
    std::map<int32_t, std::vector<uint32_t>> rows_of;
    for (uint64_t id = 0; id < n_ids; ++id) rows_of[key_of[id]].push_back((uint32_t)id);
    std::vector<float> qp((size_t)T * D), qn(T);
    struct Cand { uint32_t score; int32_t key; uint32_t slot; };
    std::vector<Cand> order;
    std::vector<uint64_t> best;
    for (uint64_t q = 0; q < n; ++q) {
        const uint32_t L = n_tokens ? (uint32_t)n_tokens[q] : T;
        const uint32_t f = (uint32_t)std::min<int64_t>(std::max<int64_t>(cand_found[q], 0), R);
        const uint32_t* bm = allow ? allow + q * nw : nullptr;
        std::fill(qp.begin(), qp.end(), 0.0f);
        for (uint32_t t = 0; t < L; ++t) {
            std::memcpy(&qp[(size_t)t * D], tokens + ((size_t)q * T + t) * dim, dim * sizeof(float));
            qn[t] = diverse_dot8(&qp[(size_t)t * D], &qp[(size_t)t * D], D);
        }
        best.assign((size_t)f * L, ~0ull);
        order.clear();
        for (uint32_t j = 0; j < f; ++j) {
            const int32_t key = cand_keys[q * R + j];
            const auto it = rows_of.find(key);
            float s = 0.0f;
            for (uint32_t t = 0; t < L; ++t) {
                uint64_t b = ~0ull;
                if (it != rows_of.end())
                    for (uint32_t id : it->second) {
                        if (bm && !((bm[id >> 5] >> (id & 31)) & 1u)) continue;
                        const float d = diverse_exact_from_dot(qn[t], norm_sq[id], diverse_dot8(&qp[(size_t)t * D], raw + (size_t)id * D, D));
                        uint32_t bits;
                        std::memcpy(&bits, &d, 4);
                        b = std::min(b, ((uint64_t)bits << 32) | id);
                    }
                best[(size_t)j * L + t] = b;
                const uint32_t bits = (uint32_t)(b >> 32);
                float d;
                std::memcpy(&d, &bits, 4);
                s = s + d;
            }
            uint32_t sb;
            std::memcpy(&sb, &s, 4);
            order.push_back(Cand{sb, key, j});
        }
        std::sort(order.begin(), order.end(), [](const Cand& a, const Cand& b) {
            return a.score != b.score ? a.score < b.score : (a.key != b.key ? a.key < b.key : a.slot < b.slot);
        });
        const uint32_t found = std::min(k, f);
        out_found[q] = (int32_t)found;
        uint32_t cert = 0;
        for (uint32_t o = 0; o < k; ++o) {
            int64_t* orow = out_rows + (q * k + o) * T;
            for (uint32_t t = 0; t < T; ++t) orow[t] = -1;
            if (o >= found) {
                out_keys[q * k + o] = 0;
                out_hits[q * k + o] = 0;
                std::memcpy(out_score + q * k + o, &fmax, 4);
                continue;
            }
            const Cand& c = order[o];
            out_keys[q * k + o] = c.key;
            out_hits[q * k + o] = (int32_t)L;
            std::memcpy(out_score + q * k + o, &c.score, 4);
            for (uint32_t t = 0; t < L; ++t) {
                const uint32_t id = (uint32_t)best[(size_t)c.slot * L + t];
                if (id < n_ids) orow[t] = rows ? (int64_t)rows[id] : (int64_t)id;
            }
            float sc;
            std::memcpy(&sc, &c.score, 4);
            if (f == R && cert == o && sc < cand_lb[q * R + R - 1]) ++cert;
        }
        out_certified[q] = (int32_t)(f < R ? found : cert);
    }
}

}  // namespace cph
