// host_group.h — the host statement of grouped search (cph_search_grouped; device_group.h holds the kernel): no HIP
// call, so the CPU tests build this file with plain g++ under sanitizers.
//
// A candidate row is what an ordinary search returns at k = C: C entries ascending by (distance, id), padded with
// -1 / FLT_MAX.  key_of[id] is an int32 per internal id.  The row is walked front to back:
//     padding is skipped; an id that occurred earlier in the row is skipped;
//     an entry whose key has no group opens one at the next group index while fewer than k exist;
//     an entry whose key has a group with fewer than g members is appended to it; every other entry is dropped.
// So groups are ordered by their best member, members ascend, ties keep the order of the row.  Keys are compared as
// values over the whole int32 range: no value is reserved.
#pragma once
#include <cfloat>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <unordered_set>

namespace cph {

constexpr uint32_t kGroupMaxCandidates = 1024;      // C <= this (kExactMaxK: the longest row the exact route returns)

// n rows of C candidates -> per row out_ids / out_dist [k][g] (padded -1 / FLT_MAX; a distance keeps the bytes of the
// row), out_keys / out_counts [k] (0 where there is no group), out_complete: (k groups, each with g members) or (fewer
// than C entries of the row are valid, so a longer row would add nothing).  rows (may be null): ids are written as
// rows[id].  Every valid id is < the length of key_of (and of rows); the caller has checked that.
inline void group_rows_host(const int64_t* ids, const float* dist, uint64_t n, uint32_t C, const int32_t* key_of, const uint32_t* rows,
                            uint32_t k, uint32_t g, int64_t* out_ids, float* out_dist, int32_t* out_keys, int32_t* out_counts,
                            uint8_t* out_complete) {
    const float fmax = FLT_MAX;
    std::unordered_set<int64_t> seen;
    std::unordered_map<int32_t, uint32_t> group_of;
    for (uint64_t q = 0; q < n; ++q) {
        const int64_t* ri = ids + q * C;
        const float* rd = dist + q * C;
        int64_t* oi = out_ids + q * k * g;
        float* od = out_dist + q * k * g;
        int32_t* ok = out_keys + q * k;
        int32_t* oc = out_counts + q * k;
        for (uint64_t t = 0; t < (uint64_t)k * g; ++t) {
            oi[t] = -1;
            std::memcpy(od + t, &fmax, 4);
        }
        for (uint32_t t = 0; t < k; ++t) ok[t] = oc[t] = 0;
        seen.clear();
        group_of.clear();
        uint32_t valid = 0, groups = 0, full = 0;
        for (uint32_t j = 0; j < C; ++j) {
            const int64_t id = ri[j];
            if (id < 0) continue;
            ++valid;
            if (!seen.insert(id).second) continue;
            const int32_t key = key_of[id];
            auto it = group_of.find(key);
            if (it == group_of.end()) {
                if (groups == k) continue;
                it = group_of.emplace(key, groups).first;
                ok[groups++] = key;
            }
            const uint32_t G = it->second;
            if ((uint32_t)oc[G] == g) continue;
            const uint64_t o = (uint64_t)G * g + (uint32_t)oc[G];
            oi[o] = rows ? (int64_t)rows[id] : id;
            std::memcpy(od + o, rd + j, 4);
            if ((uint32_t)++oc[G] == g) ++full;
        }
        out_complete[q] = (full == k || valid < C) ? 1 : 0;
    }
}

}  // namespace cph
