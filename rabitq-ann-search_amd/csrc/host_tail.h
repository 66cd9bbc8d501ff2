// host_tail.h — the host statements of the tail (cph_add; device_tail.h holds the kernels): no HIP call, so the CPU tests
// build this file with plain g++ under sanitizers.
//
// A finalized handle holds n_b base rows (the rows of its graph) and, behind them, t tail rows: tail row j has id
// n_b + j, in internal ids and in input rows alike.  A graph-routed search returns, per query, the first k entries of
// the stable merge of the graph's row G and the exact top-k T of the allowed tail rows:
//     numpy: argsort(concatenate([G, T]), kind="stable")[:k]
// entries compared as float values, the graph entry first where two are equal, padding (-1 / FLT_MAX) last.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstring>
#include <vector>

namespace cph {

// Rows the resident arrays hold room for once `need` rows no longer fit into `cap`: half as much again, 1,024 rows at
// least, so that m single-row adds copy the arrays O(log m) times; never more than the id space (2^32 - 1 ids).
inline uint64_t tail_capacity(uint64_t cap, uint64_t need) {
    if (need <= cap) return cap;
    const uint64_t grown = cap + std::max<uint64_t>(cap / 2, 1024);
    return std::min<uint64_t>(std::max(need, grown), 0xFFFFFFFFull);
}

// The fold of one batch: row i of g_ids / g_dist [n][k] (ascending in distance, padding last: what every search returns)
// with the P sorted tail lists of query i -- pools[P][n][C] keys (distance bits << 32 | id, ascending), counts[P][n]
// keys in each, every count <= k -- into row i of out_ids / out_dist.  out may be g (in place).
inline void tail_fold_host(const int64_t* g_ids, const float* g_dist, uint64_t n, uint64_t k, const uint64_t* pools,
                           const uint32_t* counts, uint32_t P, uint32_t C, int64_t* out_ids, float* out_dist) {
    std::vector<uint64_t> keys;
    std::vector<int64_t> gi(k), ri(k);
    std::vector<float> gd(k), rd(k);
    for (uint64_t q = 0; q < n; ++q) {
        keys.clear();
        for (uint32_t p = 0; p < P; ++p) {
            const uint64_t* pool = pools + ((uint64_t)p * n + q) * C;
            keys.insert(keys.end(), pool, pool + counts[(uint64_t)p * n + q]);
        }
        std::sort(keys.begin(), keys.end());          // (distance bits, id): the parts hold disjoint ids
        if (keys.size() > k) keys.resize(k);
        std::copy(g_ids + q * k, g_ids + (q + 1) * k, gi.begin());
        std::copy(g_dist + q * k, g_dist + (q + 1) * k, gd.begin());
        uint64_t a = 0, b = 0;
        for (uint64_t o = 0; o < k; ++o) {
            float td = 0.0f;
            if (b < keys.size()) {
                const uint32_t bits = (uint32_t)(keys[b] >> 32);
                std::memcpy(&td, &bits, 4);
            }
            if (b < keys.size() && td < gd[a]) {      // (a + b == o < k: a < k)
                ri[o] = (int64_t)(uint32_t)keys[b];
                rd[o] = td;
                ++b;
            } else {
                ri[o] = gi[a];
                rd[o] = gd[a];
                ++a;
            }
        }
        std::copy(ri.begin(), ri.end(), out_ids + q * k);
        std::copy(rd.begin(), rd.end(), out_dist + q * k);
    }
}

}  // namespace cph
