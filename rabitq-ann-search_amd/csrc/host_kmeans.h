// host_kmeans.h — the host statements of k-means over the resident rows (cph_kmeans; device_kmeans.h holds the kernels): no
// HIP call.  Build it with -ffp-contract=off: the sum below is separately rounded additions.
//
// One Lloyd iteration is an ASSIGNMENT (every live row to the centroid with the smallest (exact_l2 bits, centroid id),
// exact_l2 taken with the centroid as the query and the row as the id: cph_exact_l2) and an UPDATE (every centroid to the
// mean of its members).  The assignment's arithmetic is that of device_exact.h; this file states the update's.
#pragma once
#include <algorithm>
#include <cstdint>

namespace cph {

constexpr uint32_t kKmeansMaxClusters = 16384;   // the cluster counters of a sorting workgroup live in LDS: 4 B each
constexpr uint32_t kKmeansWaves = 4;             // partial sums of a centroid coordinate

// The mean of one cluster, coordinate by coordinate: THE definition of the update's arithmetic.  members[m] are the
// cluster's row ids ASCENDING (m >= 1); partial w sums the members w, w + 4, w + 8, ... in that order from 0, the four
// partials combine as ((p0 + p1) + p2) + p3, and one division by m follows.  The shape depends on the membership alone,
// so two runs over the same assignment give the same bytes.  A cluster without members keeps its centroid (the caller
// does not call this).
inline void kmeans_mean_host(const float* raw, uint32_t D, const uint32_t* members, uint32_t m, float* out) {
    for (uint32_t d = 0; d < D; ++d) {
        float p[kKmeansWaves];
        for (uint32_t w = 0; w < kKmeansWaves; ++w) {
            p[w] = 0.0f;
            for (uint32_t j = w; j < m; j += kKmeansWaves) p[w] = p[w] + raw[(uint64_t)members[j] * D + d];
        }
        out[d] = (((p[0] + p[1]) + p[2]) + p[3]) / (float)m;
    }
}

// The segments of the counting sort: rows [s * seg, (s + 1) * seg) belong to segment s; one wave ranks a segment, so
// there are enough of them to fill the GPU and few enough that the [segments][k] counters stay small.
struct KmeansSegments {
    uint32_t count, rows;
};
inline KmeansSegments kmeans_segments(uint64_t n) {
    KmeansSegments s;
    s.count = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 511) / 512, 512));
    s.rows = (uint32_t)((n + s.count - 1) / s.count);
    return s;
}

}  // namespace cph
