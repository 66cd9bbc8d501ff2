// host_diverse.h — the host statement of diversified search (cph_search_diverse; device_diverse.h holds the kernel): no
// HIP call, so the CPU tests build this file with plain g++ under sanitizers.  Build it with -ffp-contract=off: the score
// below is three separately rounded operations.
//
// A candidate row is what an ordinary search returns at k = C: C entries ascending by (distance, id), padded with
// -1 / FLT_MAX.  Walked front to back, padding and ids that occurred earlier in the row are skipped; the survivors are the
// candidates, each with its position j in the row and its relevance r_j = dist[j].  With a = lam and b = 1 - a (fp32):
//     pick 0 is the first candidate;
//     for pick t >= 1 every unpicked candidate has m_j = min over picked s of d(s, j) and score_j = (a * r_j) - (b * m_j);
//     the smallest score is picked, equal scores go to the lower position; k picks, or until the candidates run out.
// d(s, j) has the bits cph_exact_l2 returns for query = the stored row s and id = j: eight FMA chains over the padded rows
// (chain c = elements c, c + 8, ...), reduced ((c0+c4)+(c1+c5))+((c2+c6)+(c3+c7)); qnorm = the same chains over s * s (NOT
// norm_sq[s], which the builder summed with one chain); norm = norm_sq[j].  It is not symmetric in its bits.
// Outputs in pick order: ids (-1 padded), dist = r of the pick, gap = m of the pick when it was taken (FLT_MAX for pick 0
// and for padding).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <unordered_set>
#include <vector>

namespace cph {

constexpr uint32_t kDiverseMaxCandidates = 1024;    // C <= this (kExactMaxK: the longest row the exact route returns)

inline float diverse_dot8(const float* x, const float* y, uint32_t D) {
    float c[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (uint32_t i = 0; i < D; ++i) c[i & 7] = std::fma(x[i], y[i], c[i & 7]);
    return ((c[0] + c[4]) + (c[1] + c[5])) + ((c[2] + c[6]) + (c[3] + c[7]));
}

inline float diverse_exact_from_dot(float qnorm, float norm, float dot) {
    const float v = (qnorm + norm) - 2.0f * dot;
    return (v < 0.0f) ? 0.0f : v;
}

// n rows of C candidates -> per row out_ids / out_dist / out_gap [k].  raw [n_ids][D] (zero-padded rows), norm_sq [n_ids];
// ids at or above n_ids count as padding.  rows (may be null): ids are written as rows[id].
inline void diverse_rows_host(const int64_t* ids, const float* dist, uint64_t n, uint32_t C, const float* raw, const float* norm_sq,
                              uint64_t n_ids, uint32_t D, const uint32_t* rows, uint32_t k, float a, int64_t* out_ids, float* out_dist,
                              float* out_gap) {
    const float fmax = FLT_MAX;
    const float b = 1.0f - a;
    std::unordered_set<int64_t> seen;
    std::vector<uint32_t> pos;                  // the candidates that are not picked yet, ascending by position
    std::vector<float> m(C);
    for (uint64_t q = 0; q < n; ++q) {
        const int64_t* ri = ids + q * C;
        const float* rd = dist + q * C;
        int64_t* oi = out_ids + q * k;
        float* od = out_dist + q * k;
        float* og = out_gap + q * k;
        seen.clear();
        pos.clear();
        for (uint32_t j = 0; j < C; ++j) {
            const int64_t id = ri[j];
            if (id < 0 || (uint64_t)id >= n_ids) continue;
            if (!seen.insert(id).second) continue;
            pos.push_back(j);
            m[j] = fmax;
        }
        uint32_t t = 0;
        size_t take = 0;                        // index into pos of the pick (pick 0: the first candidate)
        while (t < k && !pos.empty()) {
            const uint32_t pj = pos[take];
            const uint64_t s = (uint64_t)ri[pj];
            oi[t] = rows ? (int64_t)rows[s] : (int64_t)s;
            std::memcpy(od + t, rd + pj, 4);
            og[t] = m[pj];
            pos.erase(pos.begin() + (std::ptrdiff_t)take);
            if (++t == k || pos.empty()) break;
            const float* sv = raw + s * D;
            const float qnorm = diverse_dot8(sv, sv, D);
            float best = 0.0f;
            for (size_t i = 0; i < pos.size(); ++i) {
                const uint32_t j = pos[i];
                const uint64_t id = (uint64_t)ri[j];
                const float d = diverse_exact_from_dot(qnorm, norm_sq[id], diverse_dot8(sv, raw + id * D, D));
                if (d < m[j]) m[j] = d;
                const float ar = a * rd[j], bm = b * m[j];
                const float score = ar - bm;
                if (i == 0 || score < best) {   // (equal scores: the lower position stays)
                    best = score;
                    take = i;
                }
            }
        }
        for (; t < k; ++t) {
            oi[t] = -1;
            std::memcpy(od + t, &fmax, 4);
            std::memcpy(og + t, &fmax, 4);
        }
    }
}

}  // namespace cph
