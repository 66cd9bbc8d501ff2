// host_maxsim.h — the host statement of multi-vector (late-interaction, MaxSim) search (cph_search_maxsim;
// device_maxsim.h holds the kernel): no HIP call, so the CPU tests build this file with plain g++ under sanitizers.
//
// A query is T token vectors of which the first L (1 <= L <= T) are live.  Every live token t has a candidate row: what
// an ordinary search returns for it at k = C, C entries (id, dist) ascending by (distance, id), padded with -1 / FLT_MAX.
// key_of[id] is an int32 per internal id, every int32 value an ordinary key.  An entry is valid when 0 <= id < n_ids; the
// rows of the tokens t >= L are not read.  Everything but the sum and the final order is defined by POSITION:
//     floor_t     the distance of the last valid entry of row t, +0.0f when the row has none
//     pos_t(κ)    the lowest position of row t whose entry has key κ, if any (κ: any key of a valid entry of a live row)
//     term_t(κ)   the distance at pos_t(κ) if it exists, else floor_t
//     hits(κ)     the number of live t for which pos_t(κ) exists
//     score(κ)    s = +0.0f; for t = 0 .. L - 1: s = s + term_t(κ)      (float32, in that order, no reassociation)
// The answer: the min(k, distinct keys) keys with the smallest (score as a float value, key as a signed int32), in that
// order, each with its score, its hits and rows[t] = the id at pos_t(κ) (through the row map where one is given), -1 where
// token t has no row of κ or t >= L.  Padding: key 0, score FLT_MAX, hits 0, rows -1.
//
// What it means: floor_t is the C-th distance of token t, and a row of κ that the search did not return for t is no
// closer than that.  With an exact underlying search score(κ) is therefore a LOWER BOUND of the true
// sum_t min_{r in κ, allowed} dist(q_t, r) -- in float32 too, float addition being monotone -- and equal to it when
// hits(κ) == L.  With C at least the number of allowed rows the answer is the exact MaxSim top-k.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

namespace cph {

constexpr uint32_t kMaxsimMaxTokens = 64;           // T <= this
constexpr uint32_t kMaxsimMaxCandidates = 1024;     // C <= this (kExactMaxK: the longest row the exact route returns)
constexpr uint32_t kMaxsimMaxEntries = 8192;        // T * C <= this (the kernel sorts a query's entries in LDS)
constexpr uint32_t kMaxsimMaxK = 1024;              // k <= this

// n queries of T rows of C candidates (ids / dist [n][T][C]); n_tokens [n] or null (every query has T live tokens; a
// value outside [1, T] is the caller's to refuse) -> per query out_keys / out_score / out_hits [k], out_rows [k][T],
// out_found = the groups returned.  rows (may be null): ids are written as rows[id].
inline void maxsim_rows_host(const int64_t* ids, const float* dist, uint64_t n, uint32_t T, const int32_t* n_tokens, uint32_t C,
                             const int32_t* key_of, uint64_t n_ids, const uint32_t* rows, uint32_t k, int32_t* out_keys,
                             float* out_score, int32_t* out_hits, int64_t* out_rows, int32_t* out_found) {
    const float fmax = FLT_MAX;
    std::map<int32_t, std::vector<int32_t>> first;      // key -> pos_t of every live token, -1: none
    std::vector<float> floor_of(T);
    std::vector<std::pair<float, int32_t>> order;
    for (uint64_t q = 0; q < n; ++q) {
        const uint32_t L = n_tokens ? (uint32_t)n_tokens[q] : T;
        const int64_t* qi = ids + q * T * C;
        const float* qd = dist + q * T * C;
        first.clear();
        for (uint32_t t = 0; t < L; ++t) {
            floor_of[t] = 0.0f;
            for (uint32_t j = 0; j < C; ++j) {
                const int64_t id = qi[(size_t)t * C + j];
                if (id < 0 || (uint64_t)id >= n_ids) continue;
                floor_of[t] = qd[(size_t)t * C + j];
                auto it = first.find(key_of[id]);
                if (it == first.end()) it = first.emplace(key_of[id], std::vector<int32_t>(L, -1)).first;
                if (it->second[t] < 0) it->second[t] = (int32_t)j;
            }
        }
        order.clear();
        for (const auto& kv : first) {
            float s = 0.0f;
            for (uint32_t t = 0; t < L; ++t) s = s + (kv.second[t] >= 0 ? qd[(size_t)t * C + kv.second[t]] : floor_of[t]);
            order.emplace_back(s, kv.first);
        }
        std::sort(order.begin(), order.end(), [](const std::pair<float, int32_t>& a, const std::pair<float, int32_t>& b) {
            return a.first < b.first || (a.first == b.first && a.second < b.second);
        });
        const uint32_t found = (uint32_t)std::min<size_t>(k, order.size());
        out_found[q] = (int32_t)found;
        for (uint32_t o = 0; o < k; ++o) {
            int32_t* okey = out_keys + q * k + o;
            int32_t* ohit = out_hits + q * k + o;
            int64_t* orow = out_rows + (q * k + o) * T;
            for (uint32_t t = 0; t < T; ++t) orow[t] = -1;
            if (o >= found) {
                *okey = 0;
                *ohit = 0;
                std::memcpy(out_score + q * k + o, &fmax, 4);
                continue;
            }
            const std::vector<int32_t>& pos = first[order[o].second];
            int32_t hits = 0;
            for (uint32_t t = 0; t < L; ++t) {
                if (pos[t] < 0) continue;
                const int64_t id = qi[(size_t)t * C + pos[t]];
                orow[t] = rows ? (int64_t)rows[id] : id;
                ++hits;
            }
            *okey = order[o].second;
            *ohit = hits;
            std::memcpy(out_score + q * k + o, &order[o].first, 4);
        }
    }
}

}  // namespace cph
