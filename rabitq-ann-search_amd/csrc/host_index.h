// host_index.h — host side of the hot path: v2 index file reader/writer, the repacker that
// turns reference-layout neighbour blocks into the device layout, and the host mirror of the
// query encoder (used to make the synthetic query of the streaming benchmark; queries of a
// search are encoded on the device, device_encode.h).
//
// Reference counterparts (relative to /root/reference/include/cphnsw/):
//   api/hnsw_index.hpp:217-303 save, :305-443 load            -> HostIndex::save / load
//   graph/rabitq_graph.hpp:19-29, distance/fastscan_layout.hpp -> repack_* (layout only)
//   encoder/rotation.hpp:15-67, encoder/transform/fht.hpp:23-57 -> Rotation
//   encoder/rabitq_encoder.hpp:73-79,98-136,197-209            -> encode_query
// This file is compiled with -ffp-contract=off; each fused multiply-add is explicit and
// sits where the compiled reference has one.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "cph_core.h"

namespace cph {

struct UpperEdge {
    uint32_t node;
    std::vector<uint32_t> nbrs;
};

struct Rotation {
    size_t D = 0;
    std::vector<float> signs;  // [3][D]
    void init(size_t D_, uint64_t seed) {
        D = D_;
        signs.resize(3 * D);
        // one mt19937_64 stream, uniform_int_distribution<int>(0,1) drawn layer-major
        // (rotation.hpp:23-31); libstdc++ resolves that range to the top bit of each draw.
        std::mt19937_64 rng(seed);
        for (size_t i = 0; i < 3 * D; ++i) signs[i] = (rng() >> 63) ? 1.0f : -1.0f;
    }
    static void fht(float* v, size_t len) {
        // butterflies of fht.hpp:26-56: the in-register stages (h = 1,2,4) keep
        // (upper - lower) in the upper slot, the strided stages (h >= 8) (lower - upper)
        for (size_t h = 1; h < len; h *= 2)
            for (size_t i = 0; i < len; i += 2 * h)
                for (size_t j = i; j < i + h; ++j) {
                    float x = v[j], y = v[j + h];
                    v[j] = x + y;
                    v[j + h] = (h < 8) ? (y - x) : (x - y);
                }
    }
    void apply(float* x) const {
        for (int l = 0; l < 3; ++l) {
            const float* s = &signs[l * D];
            for (size_t i = 0; i < D; ++i) x[i] = x[i] * s[i];
            fht(x, D);
        }
    }
};

struct EncodedQuery {
    float A, B, C;
    std::vector<uint8_t> qu;  // 4-bit scalars per dimension [D]
};

// buf: padded raw query (D floats), overwritten with the rotated, scaled vector.
inline void encode_query(const Rotation& rot, float* buf, EncodedQuery& out) {
    const size_t D = rot.D;
    rot.apply(buf);
    const float d = static_cast<float>(D);
    const float norm_factor = 1.0f / (d * std::sqrt(d));
    const float inv_sqrt_d = 1.0f / std::sqrt(d);
    for (size_t i = 0; i < D; ++i) buf[i] = buf[i] * norm_factor;
    float vl = buf[0], vmax = buf[0];
    for (size_t i = 1; i < D; ++i) {
        if (buf[i] < vl) vl = buf[i];
        if (buf[i] > vmax) vmax = buf[i];
    }
    float delta = (vmax - vl) / 15.0f;
    if (delta < kEpsTiny) delta = kEpsTiny;
    const float inv_delta = 1.0f / delta;
    out.qu.resize(D);
    float sum_qu = 0.0f;
    for (size_t i = 0; i < D; ++i) {
        int u = static_cast<int>(std::fmaf(buf[i] - vl, inv_delta, 0.5f));
        u = u < 0 ? 0 : (u > 15 ? 15 : u);
        out.qu[i] = static_cast<uint8_t>(u);
        sum_qu += static_cast<float>(u);
    }
    out.A = (2.0f * delta) * inv_sqrt_d;
    out.B = (2.0f * vl) * inv_sqrt_d;
    out.C = -std::fmaf(d, vl, delta * sum_qu) * inv_sqrt_d;
}

// Bit-slice the 4-bit scalars into the device query masks: word w -> {Q0,Q1,Q2,Q3}, bit t of
// Q_j = bit j of qu[32w + t].
inline void qu_to_masks(const uint8_t* qu, size_t D, uint32_t* masks /*[PW][4]*/) {
    const size_t PW = D >= 32 ? D / 32 : 1;
    std::memset(masks, 0, PW * 16);
    for (size_t d = 0; d < D; ++d)
        for (int j = 0; j < 4; ++j)
            if ((qu[d] >> j) & 1) masks[(d / 32) * 4 + j] |= 1u << (d % 32);
}

// Reference LUT format (u8[D/4][16]) <-> 4-bit scalars.
inline void qu_to_lut(const uint8_t* qu, size_t D, uint8_t* lut) {
    for (size_t s = 0; s < D / 4; ++s)
        for (unsigned p = 0; p < 16; ++p) {
            uint8_t v = 0;
            for (unsigned b = 0; b < 4; ++b)
                if (p & (1u << b)) v = static_cast<uint8_t>(v + qu[4 * s + b]);
            lut[s * 16 + p] = v;
        }
}
inline void lut_to_qu(const uint8_t* lut, size_t D, uint8_t* qu) {
    for (size_t d = 0; d < D; ++d) qu[d] = lut[(d / 4) * 16 + (1u << (d % 4))];
}

// A file that appears under its final name only when it is complete: written as <path>.tmp.<pid>, flushed, synced to
// the device (fsync: a rename can reach the disk before the data it names, and a crash in between would leave a
// truncated file under the final name) and closed with the results checked, then renamed over the target and the
// directory entry synced.  A handle that serves an index out of a mapping of `path` keeps its (old) inode; a failed or
// interrupted save leaves the previous file untouched.
struct AtomicFile {
    std::string path, tmp;
    FILE* f = nullptr;
    explicit AtomicFile(const std::string& p) : path(p), tmp(p + ".tmp." + std::to_string((long)getpid())) {
        f = std::fopen(tmp.c_str(), "wb");
        if (!f) throw std::runtime_error("Cannot open file for writing: " + path);
    }
    AtomicFile(const AtomicFile&) = delete;
    AtomicFile& operator=(const AtomicFile&) = delete;
    void write(const void* p, size_t b) {
        if (b && std::fwrite(p, 1, b, f) != b) throw std::runtime_error("Write error: " + path);
    }
    void commit() {
        const bool ok = std::fflush(f) == 0 && ::fsync(fileno(f)) == 0;
        const bool closed = std::fclose(f) == 0;
        f = nullptr;
        if (!ok || !closed) throw std::runtime_error("Write error: " + path);
        if (std::rename(tmp.c_str(), path.c_str()) != 0) throw std::runtime_error("Cannot rename the finished file into place: " + path);
        tmp.clear();
        // the new directory entry (best effort: some file systems refuse to open a directory for this)
        const size_t slash = path.find_last_of('/');
        const std::string dir = slash == std::string::npos ? "." : (slash == 0 ? "/" : path.substr(0, slash));
        const int dfd = ::open(dir.c_str(), O_RDONLY | O_DIRECTORY);
        if (dfd >= 0) { (void)::fsync(dfd); ::close(dfd); }
    }
    ~AtomicFile() {
        if (f) std::fclose(f);
        if (!tmp.empty()) std::remove(tmp.c_str());
    }
};

// rows[0..n) holds every value of 0..n-1 once (what a row map must be: HostIndex::rows).
inline bool is_row_permutation(const uint32_t* rows, size_t n) {
    std::vector<uint8_t> seen(n, 0);
    for (size_t i = 0; i < n; ++i) {
        if (rows[i] >= n || seen[rows[i]]) return false;
        seen[rows[i]] = 1;
    }
    return true;
}

// The host statement of the row-space filter (cph_filter_create_rows; device_rows.h): bit i of `out` = bit rows[i] of
// `in`, for the n internal ids; bits of the last word behind n are clear.  Both bitmaps are (n + 31) / 32 words.
inline void rows_filter_host(const uint32_t* in, const uint32_t* rows, size_t n, uint32_t* out) {
    for (size_t w = 0; w < (n + 31) / 32; ++w) out[w] = 0u;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t r = rows[i];
        out[i >> 5] |= ((in[r >> 5] >> (r & 31)) & 1u) << (i & 31);
    }
}

// The host statement of the effective filter of a handle with removed rows (device_tombstone.h: live_filter_kernel;
// cph_host_live_filter): out = allow & ~removed (allow null: every id) over n ids, the bits of the last word behind n
// clear whatever the inputs hold there; returns the number of ids left.  All bitmaps are (n + 31) / 32 words.
inline uint64_t live_filter_host(const uint32_t* allow, const uint32_t* removed, size_t n, uint32_t* out) {
    uint64_t c = 0;
    for (size_t w = 0, nw = (n + 31) / 32; w < nw; ++w) {
        uint32_t x = (allow ? allow[w] : 0xFFFFFFFFu) & ~removed[w];
        if (w == nw - 1 && (n & 31)) x &= (1u << (n & 31)) - 1u;
        out[w] = x;
        c += (uint64_t)__builtin_popcount(x);
    }
    return c;
}

// The host statement of the label filters (cph_filters_from_labels; device_labels.h): bit i of filter j = lo[j] <=
// labels[i] <= hi[j] (signed, both ends inclusive; lo[j] > hi[j]: the empty filter).  out: m bitmaps of (n + 31) / 32
// words each, one behind the other, every word written and the bits of the last word behind n clear; counts[j] = ids
// allowed by filter j.
inline void label_filters_host(const int32_t* labels, size_t n, const int32_t* lo, const int32_t* hi, size_t m, uint32_t* out,
                               uint64_t* counts) {
    const size_t nw = (n + 31) / 32;
    for (size_t j = 0; j < m; ++j) {
        uint32_t* w = out + j * nw;
        uint64_t c = 0;
        for (size_t k = 0; k < nw; ++k) w[k] = 0u;
        for (size_t i = 0; i < n; ++i)
            if (labels[i] >= lo[j] && labels[i] <= hi[j]) {
                w[i >> 5] |= 1u << (i & 31);
                ++c;
            }
        counts[j] = c;
    }
}

// Labels given per input row -> the label column in internal-id order (cph_set_labels with CPH_IDS_INPUT): out[i] =
// by_row[rows[i]] for the n internal ids; rows is a row map (every entry < n).
inline void labels_to_internal_host(const int32_t* by_row, const uint32_t* rows, size_t n, int32_t* out) {
    for (size_t i = 0; i < n; ++i) out[i] = by_row[rows[i]];
}

// ---- tag columns (cph_set_tags; device_tags.h) ----
// A tag column gives every row a SET of int32 tags, as a CSR in internal-id order: lims[n + 1] (uint32, lims[0] = 0) and
// tags[lims[n]], ascending and distinct inside a row.  A tag test is a set V of at most kMaxTagTestValues values
// (ascending, distinct) and a mode; with c(row) = |tags(row) & V| it allows the row when c > 0 (any), c == |V| (all: exact,
// because both sides are distinct) or c == 0 (none).
constexpr uint32_t kMaxTagColumns = 4;        // CPH_MAX_TAG_COLUMNS
constexpr uint32_t kMaxTagsPerRow = 1024;     // CPH_MAX_TAGS_PER_ROW, after dedup
constexpr uint32_t kMaxTagTestValues = 64;    // CPH_MAX_TAG_TEST_VALUES, after dedup
enum TagMode : uint8_t { kTagsAny = 0, kTagsAll = 1, kTagsNone = 2 };

// The caller's CSR (lims[n + 1], 64-bit, any order and duplicates inside a row) -> the canonical column.  rows (may be
// null): canonical row i is the caller's row rows[i] for i < n_rows (cph_set_tags with CPH_IDS_INPUT; the rows behind
// n_rows stay where they are), else row i.  Refuses (std::invalid_argument) a lims that does not start at 0 or decreases,
// null tags with lims[n] != 0, a row of more than kMaxTagsPerRow distinct tags and 2^32 tags or more after dedup.
inline void tags_canonical_host(const uint64_t* lims, const int32_t* tags, size_t n, const uint32_t* rows, size_t n_rows,
                                std::vector<uint32_t>& out_lims, std::vector<int32_t>& out_tags) {
    if (!lims) throw std::invalid_argument("null tag limits");
    if (lims[0] != 0) throw std::invalid_argument("tag limits must start at 0");
    for (size_t i = 0; i < n; ++i)
        if (lims[i + 1] < lims[i]) throw std::invalid_argument("tag limits must not decrease (row " + std::to_string(i) + ")");
    if (lims[n] != 0 && !tags) throw std::invalid_argument("null tags");
    std::vector<uint32_t> ol(n + 1, 0u);
    std::vector<int32_t> ot, row;
    ot.reserve(lims[n]);
    for (size_t i = 0; i < n; ++i) {
        const size_t r = rows && i < n_rows ? rows[i] : i;
        row.clear();                                        // (an empty row touches no pointer: tags may be null)
        if (lims[r + 1] != lims[r]) row.assign(tags + lims[r], tags + lims[r + 1]);
        std::sort(row.begin(), row.end());
        row.erase(std::unique(row.begin(), row.end()), row.end());
        if (row.size() > kMaxTagsPerRow)
            throw std::invalid_argument("row " + std::to_string(r) + " has " + std::to_string(row.size()) + " distinct tags, at most " +
                                        std::to_string(kMaxTagsPerRow) + " (CPH_MAX_TAGS_PER_ROW)");
        ot.insert(ot.end(), row.begin(), row.end());
        if (ot.size() > 0xFFFFFFFFull) throw std::invalid_argument("a tag column holds fewer than 2^32 tags");
        ol[i + 1] = (uint32_t)ot.size();
    }
    out_lims.swap(ol);
    out_tags.swap(ot);
}

// The caller's m tests (test_lims[m + 1] from 0, non-decreasing; values in any order, duplicates allowed) -> canonical
// ones.  Refuses a mode above kTagsNone and a test of more than kMaxTagTestValues distinct values.
inline void tag_tests_canonical_host(const uint32_t* test_lims, const int32_t* test_vals, const uint8_t* modes, size_t m,
                                     std::vector<uint32_t>& out_lims, std::vector<int32_t>& out_vals) {
    if (!test_lims || !modes) throw std::invalid_argument("null tag tests");
    if (test_lims[0] != 0) throw std::invalid_argument("tag test limits must start at 0");
    std::vector<uint32_t> ol(m + 1, 0u);
    std::vector<int32_t> ov, v;
    for (size_t j = 0; j < m; ++j) {
        if (test_lims[j + 1] < test_lims[j]) throw std::invalid_argument("tag test limits must not decrease (test " + std::to_string(j) + ")");
        if (modes[j] > kTagsNone) throw std::invalid_argument("tag test mode must be CPH_TAGS_ANY, CPH_TAGS_ALL or CPH_TAGS_NONE");
        if (test_lims[j + 1] != test_lims[j] && !test_vals) throw std::invalid_argument("null tag test values");
        v.clear();
        if (test_lims[j + 1] != test_lims[j]) v.assign(test_vals + test_lims[j], test_vals + test_lims[j + 1]);
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
        if (v.size() > kMaxTagTestValues)
            throw std::invalid_argument("tag test " + std::to_string(j) + " has " + std::to_string(v.size()) + " distinct values, at most " +
                                        std::to_string(kMaxTagTestValues) + " (CPH_MAX_TAG_TEST_VALUES)");
        ov.insert(ov.end(), v.begin(), v.end());
        ol[j + 1] = (uint32_t)ov.size();
    }
    out_lims.swap(ol);
    out_vals.swap(ov);
}

inline bool tag_mode_allows(uint8_t mode, uint32_t c, uint32_t nv) {
    return mode == kTagsAny ? c > 0 : mode == kTagsAll ? c == nv : c == 0;
}

// The host statement of the tag filters (cph_filters_from_tags; device_tags.h) on a canonical column and canonical tests:
// bit i of filter j = tag_mode_allows(modes[j], |tags(i) & V_j|, |V_j|).  out: m bitmaps of (n + 31) / 32 words each, one
// behind the other, every word written and the bits of the last word behind n clear; counts[j] = ids allowed by filter j.
inline void tag_filters_host(const uint32_t* lims, const int32_t* tags, size_t n, const uint32_t* test_lims, const int32_t* test_vals,
                             const uint8_t* modes, size_t m, uint32_t* out, uint64_t* counts) {
    const size_t nw = (n + 31) / 32;
    for (size_t j = 0; j < m; ++j) {
        uint32_t* w = out + j * nw;
        const uint32_t nv = test_lims[j + 1] - test_lims[j];
        const int32_t* v0 = nv ? test_vals + test_lims[j] : nullptr;
        uint64_t total = 0;
        for (size_t k = 0; k < nw; ++k) w[k] = 0u;
        for (size_t i = 0; i < n; ++i) {
            uint32_t c = 0;
            for (uint32_t t = lims[i]; t < lims[i + 1]; ++t) c += std::binary_search(v0, v0 + nv, tags[t]) ? 1u : 0u;
            if (tag_mode_allows(modes[j], c, nv)) {
                w[i >> 5] |= 1u << (i & 31);
                ++total;
            }
        }
        counts[j] = total;
    }
}

// Canonical rows [first, first + count) of a canonical column as a CSR of their own, the limits rebased to 0 (what
// cph_get_tags returns; the cut of a partitioned index).
inline void tags_slice_host(const uint32_t* lims, const int32_t* tags, size_t first, size_t count, uint64_t* lims_out, int32_t* tags_out) {
    for (size_t i = 0; i <= count; ++i) lims_out[i] = (uint64_t)(lims[first + i] - lims[first]);
    if (tags_out && lims[first + count] != lims[first]) std::copy(tags + lims[first], tags + lims[first + count], tags_out);
}

// The tests as the kernel reads them, one uint32 table: offs[m + 1] | info[m] | (pad to 4) | values.  Every test's values
// are padded to a multiple of kTagTestPad with copies of its last value (the kernel ORs the compares of a group, so a
// repeated value changes nothing) and start on a 16 B boundary; offs counts in values from the start of the value area;
// info[j] = mode | |V_j| << 8 (the real size: what `all` compares with).  An empty test has no values at all.
constexpr uint32_t kTagTestPad = 4;
inline void tag_tests_pack_host(const uint32_t* test_lims, const int32_t* test_vals, const uint8_t* modes, size_t m,
                                std::vector<uint32_t>& table, size_t& vals_at) {
    vals_at = (2 * m + 1 + 3) / 4 * 4;
    table.assign(vals_at, 0u);
    for (size_t j = 0; j < m; ++j) {
        const uint32_t nv = test_lims[j + 1] - test_lims[j];
        table[m + 1 + j] = (uint32_t)modes[j] | nv << 8;
        for (uint32_t i = 0; i < (nv + kTagTestPad - 1) / kTagTestPad * kTagTestPad; ++i)
            table.push_back((uint32_t)test_vals[test_lims[j] + std::min(i, nv - 1)]);
        table[j + 1] = (uint32_t)(table.size() - vals_at);
    }
}

// ---- facet counts (cph_facet_counts, cph_facet_top; device_facets.h) ----
// The dictionary of a column: `values` = its distinct values ascending (as int32: INT32_MIN and INT32_MAX are ordinary),
// codes[i] = the position of vals[i] in `values`, so codes ascend with values.  vals: one per row, or one per CSR entry of
// a tag column.  Fewer than 2^32 entries (a code is 32-bit).
constexpr uint32_t kFacetTopMaxHost = 1024;   // (= device_facets.h: kFacetTopMax) K of facet_top_host, at most
inline void facet_dictionary_host(const int32_t* vals, size_t n_entries, std::vector<int32_t>& values, std::vector<uint32_t>& codes) {
    if (n_entries > 0xFFFFFFFFull) throw std::invalid_argument("a facet column holds fewer than 2^32 entries");
    if (n_entries != 0 && !vals) throw std::invalid_argument("null facet column");
    std::vector<int32_t> v(vals, vals + n_entries);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    std::vector<uint32_t> c(n_entries);
    for (size_t i = 0; i < n_entries; ++i) c[i] = (uint32_t)(std::lower_bound(v.begin(), v.end(), vals[i]) - v.begin());
    values.swap(v);
    codes.swap(c);
}

// The host statement of the counting pass: counts[j][u] = rows i < n whose bit is set in filters[j] (a null entry, or
// filters == null: every row), clear in `removed` (null: nothing removed), and whose code is u -- for a tag column (lims
// != null: [n + 1], codes parallel to the tags) whose entries codes[lims[i] .. lims[i + 1]) hold u.  Bits at ids >= n and
// words behind (n + 31) / 32 are not read.  counts: [m][U], every one written.  Refuses (std::invalid_argument, before the
// first write) n >= 2^32 - 1, limits that do not start at 0 or decrease, and a code >= U.
inline void facet_counts_host(const uint32_t* codes, const uint32_t* lims, size_t n, size_t U, const uint32_t* const* filters,
                              const uint32_t* removed, size_t m, uint64_t* counts) {
    if (n >= 0xFFFFFFFFull) throw std::invalid_argument("facet counts cover fewer than 2^32 - 1 rows");
    const size_t entries = lims ? lims[n] : n;
    if (lims && lims[0] != 0) throw std::invalid_argument("facet limits must start at 0");
    for (size_t i = 0; lims && i < n; ++i)
        if (lims[i + 1] < lims[i]) throw std::invalid_argument("facet limits must not decrease (row " + std::to_string(i) + ")");
    for (size_t e = 0; e < entries; ++e)
        if (codes[e] >= U) throw std::invalid_argument("facet code out of range (entry " + std::to_string(e) + ")");
    for (size_t j = 0; j < m; ++j) {
        uint64_t* c = counts + j * U;
        const uint32_t* f = filters ? filters[j] : nullptr;
        for (size_t u = 0; u < U; ++u) c[u] = 0;
        for (size_t i = 0; i < n; ++i) {
            if (f && !((f[i >> 5] >> (i & 31)) & 1u)) continue;
            if (removed && ((removed[i >> 5] >> (i & 31)) & 1u)) continue;
            if (!lims) ++c[codes[i]];
            else
                for (uint32_t e = lims[i]; e < lims[i + 1]; ++e) ++c[codes[e]];
        }
    }
}

// The host statement of the selection: of one filter's counts[U], the K values with the largest non-zero counts, count
// descending and ties by value ascending (values ascend with codes); *found = min(K, non-zero counts); the slots at and
// behind *found hold value 0 and count 0.  Refuses K outside [1, kFacetTopMaxHost].
inline void facet_top_host(const uint64_t* counts, const int32_t* values, size_t U, size_t K, int32_t* values_out, uint64_t* counts_out,
                           uint32_t* found) {
    if (K < 1 || K > kFacetTopMaxHost) throw std::invalid_argument("facet top must lie in [1, " + std::to_string(kFacetTopMaxHost) + "]");
    std::vector<uint32_t> order;
    for (size_t u = 0; u < U; ++u)
        if (counts[u]) order.push_back((uint32_t)u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return counts[a] > counts[b]; });
    const size_t got = std::min(K, order.size());
    for (size_t i = 0; i < K; ++i) {
        values_out[i] = i < got ? values[order[i]] : 0;
        counts_out[i] = i < got ? counts[order[i]] : 0;
    }
    *found = (uint32_t)got;
}

// The host statement of the filter algebra (cph_filters_combine; device_filter_ops.h): out[j] = a[j] OP b[j] word by
// word for m bitmaps of (n_bits + 31) / 32 words each, one behind the other; b holds m bitmaps, or ONE that every j
// reads (b_broadcast), and is not read for kFilterNot.  Every word of `out` is written; the bits of the last word at
// or above n_bits are clear whatever the inputs hold there (NOT would set them); counts[j] = popcount(out[j]).
enum FilterOp : int { kFilterAnd = 0, kFilterOr = 1, kFilterAndNot = 2, kFilterXor = 3, kFilterNot = 4 };
constexpr int kFilterOps = 5;

inline uint32_t filter_op_word(int op, uint32_t a, uint32_t b) {
    switch (op) {
        case kFilterAnd: return a & b;
        case kFilterOr: return a | b;
        case kFilterAndNot: return a & ~b;
        case kFilterXor: return a ^ b;
        default: return ~a;
    }
}

inline void filter_combine_host(int op, const uint32_t* a, const uint32_t* b, bool b_broadcast, size_t n_bits, size_t m,
                                uint32_t* out, uint64_t* counts) {
    const size_t nw = (n_bits + 31) / 32;
    const uint32_t last = (n_bits & 31) ? (1u << (n_bits & 31)) - 1u : 0xFFFFFFFFu;
    for (size_t j = 0; j < m; ++j) {
        const uint32_t* aj = a + j * nw;
        const uint32_t* bj = op == kFilterNot ? nullptr : b + (b_broadcast ? 0 : j * nw);
        uint64_t c = 0;
        for (size_t w = 0; w < nw; ++w) {
            uint32_t x = filter_op_word(op, aj[w], bj ? bj[w] : 0u);
            if (w == nw - 1) x &= last;
            out[j * nw + w] = x;
            c += (uint64_t)__builtin_popcount(x);
        }
        counts[j] = c;
    }
}

constexpr uint32_t kMaxColumns = 8;   // extra attribute columns of a handle (cph_set_column), next to the label column
// The row attributes of a handle, each under one id: 0 the label column, 1..kMaxColumns the int32 columns, then the tag columns.
constexpr uint32_t kFacetColumns = 1 + kMaxColumns + kMaxTagColumns;

// The host copy of one row attribute in internal-id order.  A dense column (the label column, an int32 column) is vals[n]
// and no lims; a tag column is the canonical CSR lims[n + 1] into vals.  Both empty = the index holds no such column.
struct HostColumn {
    std::vector<int32_t> vals;
    std::vector<uint32_t> lims;
    bool empty() const { return vals.empty() && lims.empty(); }
    bool dense() const { return lims.empty(); }
    // complete over n rows (what a replica without host arrays never is)
    bool covers(size_t n) const { return dense() ? !vals.empty() && vals.size() == n : lims.size() == n + 1; }
    // the values of row i: vals[row_begin(i)] .. vals[row_end(i) - 1]
    size_t row_begin(size_t i) const { return dense() ? i : lims[i]; }
    size_t row_end(size_t i) const { return dense() ? i + 1 : lims[i + 1]; }
};

struct HostIndex {
    size_t D = 0, bw = 0, dim = 0, n = 0;
    int32_t max_level = 0;
    uint32_t entry = kInvalidNode;
    float upper_tau = 0.0f, upper_alpha = 1.2f;
    double mL = 0.0;
    uint64_t seed = 42;
    uint8_t calib[248];
    uint8_t profile[72];
    std::vector<float> centroid;
    std::vector<int32_t> levels;
    std::vector<float> norm_sq;
    std::vector<float> raw;           // [n][D]  (empty when the vectors are served from a mapped native file)
    const float* raw_view = nullptr;  // [n][D] inside a mapped native file (csrc/native_file.h), else null
    std::vector<uint8_t> search_data; // n * vertex_bytes, reference layout (kept for save; a native load rebuilds it on demand)
    std::vector<std::vector<UpperEdge>> upper;
    // The row map: rows[i] = row of the array given to build() that internal id i holds (a permutation of 0..n-1).
    // Empty = no map: the index came from a v2 file, which cannot carry one (save() drops it).
    std::vector<uint32_t> rows;
    // The removed rows (cph_remove): bit i & 31 of word i >> 5 = internal id i is a tombstone; (n + 31) / 32 words, or
    // empty = none (n_removed = 0).  Only a native file carries them; save() refuses an index that has some.
    std::vector<uint32_t> removed;
    uint64_t n_removed = 0;
    // The row attributes (cph_set_labels, cph_set_column, cph_set_tags), by column id; an empty one = none.  No file
    // carries them: a load or a build leaves none, compact carries them over.
    HostColumn cols[kFacetColumns];
    RefLayout RL;
    Rotation rot;
    bool has_dup_neighbors = false;

    template <class T>
    static T rd(const uint8_t* p) {
        T v;
        std::memcpy(&v, p, sizeof(T));
        return v;
    }

    SearchConsts consts() const {
        SearchConsts s{};
        s.affine_a = rd<float>(calib + 0);
        s.affine_b = rd<float>(calib + 4);
        s.ip_qo_floor = rd<float>(calib + 8);
        s.gamma_max = rd<float>(calib + 84);
        s.gamma_beta = rd<float>(calib + 88);
        s.gamma_warmup = rd<uint64_t>(calib + 96);
        std::memcpy(s.slack, calib + 108, 128);
        s.num_slack = rd<int32_t>(calib + 236);
        if (s.num_slack > kMaxSlack) s.num_slack = kMaxSlack;
        s.gamma = rd<float>(calib + 240);
        return s;
    }

    // api/hnsw_index.hpp:305-443.  expect_* come from the handle (the reference's template
    // parameters / constructor argument) and produce the same error texts.
    void load(const std::string& path, size_t expect_D, size_t expect_bw, size_t expect_dim) {
        FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) throw std::runtime_error("Cannot open file for reading: " + path);
        struct Closer { FILE* f; ~Closer() { std::fclose(f); } } closer{f};
        auto rdn = [&](void* p, size_t b) {
            if (b && std::fread(p, 1, b, f) != b)
                throw std::runtime_error("Read error or truncated file: " + path);
        };
        uint8_t hdr[68];
        rdn(hdr, 12);
        if (rd<uint64_t>(hdr) != 0x57534E48504300ULL)
            throw std::runtime_error("Invalid magic bytes (not a CP-HNSW index file).");
        if (rd<uint32_t>(hdr + 8) != 2)
            throw std::runtime_error("Unsupported index file version: " +
                                     std::to_string(rd<uint32_t>(hdr + 8)));
        rdn(hdr + 12, 56);
        const uint32_t fD = rd<uint32_t>(hdr + 12), fR = rd<uint32_t>(hdr + 16),
                       fBW = rd<uint32_t>(hdr + 20), fdim = rd<uint32_t>(hdr + 24);
        if (fD != expect_D || fR != 32 || fBW != expect_bw)
            throw std::runtime_error(
                "Index file template parameters mismatch: file D=" + std::to_string(fD) +
                " R=" + std::to_string(fR) + " BW=" + std::to_string(fBW) + ", expected D=" +
                std::to_string(expect_D) + " R=32 BW=" + std::to_string(expect_bw));
        if (fdim != expect_dim)
            throw std::runtime_error("Index file dim=" + std::to_string(fdim) +
                                     " mismatches Index dim=" + std::to_string(expect_dim));
        if (rd<uint64_t>(hdr + 60) != 42) throw std::runtime_error("Index file rotation seed mismatch.");

        HostIndex t;
        t.D = fD; t.bw = fBW; t.dim = fdim;
        t.n = rd<uint64_t>(hdr + 28);
        t.max_level = rd<int32_t>(hdr + 36);
        t.entry = rd<uint32_t>(hdr + 40);
        t.upper_tau = rd<float>(hdr + 44);
        t.upper_alpha = rd<float>(hdr + 48);
        t.mL = rd<double>(hdr + 52);
        t.seed = rd<uint64_t>(hdr + 60);
        t.RL = make_ref_layout(t.D, t.bw);
        rdn(t.calib, 248);
        rdn(t.profile, 72);
        const size_t n = t.n;
        {   // the counts come from the file: check them against its size before anything is allocated from them
            const long here = std::ftell(f);
            std::fseek(f, 0, SEEK_END);
            const long total = std::ftell(f);
            std::fseek(f, here, SEEK_SET);
            const unsigned __int128 need = (unsigned __int128)n * (8 + t.D * 4 + t.RL.vertex_bytes) + t.dim * 4 + 4;
            if (here < 0 || total < here || need > (unsigned __int128)(total - here))
                throw std::runtime_error("Read error or truncated file: " + path);
        }
        t.centroid.resize(t.dim);  rdn(t.centroid.data(), t.dim * 4);
        t.levels.resize(n);        rdn(t.levels.data(), n * 4);
        t.norm_sq.resize(n);       rdn(t.norm_sq.data(), n * 4);
        t.raw.resize(n * t.D);     rdn(t.raw.data(), n * t.D * 4);
        t.search_data.resize(n * t.RL.vertex_bytes);
        rdn(t.search_data.data(), t.search_data.size());
        uint32_t nl = 0;
        rdn(&nl, 4);
        if (nl > 64) throw std::runtime_error("Corrupt index: too many upper layers");
        t.upper.resize(nl);
        for (uint32_t l = 0; l < nl; ++l) {
            uint32_t sz = 0;
            rdn(&sz, 4);
            if (sz > n) throw std::runtime_error("Corrupt index: upper layer larger than the index");
            t.upper[l].resize(sz);
            for (uint32_t e = 0; e < sz; ++e) {
                uint32_t cnt = 0;
                rdn(&t.upper[l][e].node, 4);
                rdn(&cnt, 4);
                if (cnt > n) throw std::runtime_error("Corrupt index: upper-layer degree out of range");
                t.upper[l][e].nbrs.resize(cnt);
                rdn(t.upper[l][e].nbrs.data(), (size_t)cnt * 4);
            }
        }
        t.validate();
        t.rot.init(t.D, t.seed);
        *this = std::move(t);
    }

    // The reference trusts the file; the GPU path must not chase an out-of-range id.
    void validate() {
        has_dup_neighbors = false;
        if (n != 0 && entry != kInvalidNode && entry >= n) throw std::runtime_error("Corrupt index: entry point out of range");
        for (size_t v = 0; v < n; ++v) {
            const uint8_t* nb = &search_data[v * RL.vertex_bytes + RL.nb_off];
            uint32_t cnt = rd<uint32_t>(nb + RL.count);
            if (cnt > 32) throw std::runtime_error("Corrupt index: neighbour count > 32");
            const uint32_t* ids = reinterpret_cast<const uint32_t*>(nb + RL.ids);
            for (uint32_t i = 0; i < cnt; ++i) {
                if (ids[i] >= n) throw std::runtime_error("Corrupt index: neighbour id out of range");
                for (uint32_t j = 0; j < i; ++j)
                    if (ids[j] == ids[i]) has_dup_neighbors = true;
            }
        }
        for (auto& layer : upper)
            for (auto& e : layer) {
                if (e.node >= n) throw std::runtime_error("Corrupt index: upper-layer node out of range");
                for (uint32_t x : e.nbrs)
                    if (x >= n) throw std::runtime_error("Corrupt index: upper-layer neighbour out of range");
            }
    }

    // api/hnsw_index.hpp:217-303
    void save(const std::string& path) const {
        AtomicFile out(path);
        auto wr = [&](const void* p, size_t b) { out.write(p, b); };
        const uint64_t magic = 0x57534E48504300ULL;
        const uint32_t version = 2, hD = (uint32_t)D, hR = 32, hBW = (uint32_t)bw, hdim = (uint32_t)dim;
        const uint64_t hn = n;
        wr(&magic, 8); wr(&version, 4); wr(&hD, 4); wr(&hR, 4); wr(&hBW, 4); wr(&hdim, 4);
        wr(&hn, 8); wr(&max_level, 4); wr(&entry, 4); wr(&upper_tau, 4); wr(&upper_alpha, 4);
        wr(&mL, 8); wr(&seed, 8);
        wr(calib, 248); wr(profile, 72);
        wr(centroid.data(), dim * 4);
        wr(levels.data(), n * 4);
        wr(norm_sq.data(), n * 4);
        wr(vec(0), n * D * 4);
        wr(search_data.data(), search_data.size());
        const uint32_t nl = (uint32_t)upper.size();
        wr(&nl, 4);
        for (const auto& layer : upper) {
            const uint32_t sz = (uint32_t)layer.size();
            wr(&sz, 4);
            for (const auto& e : layer) {
                const uint32_t cnt = (uint32_t)e.nbrs.size();
                wr(&e.node, 4); wr(&cnt, 4);
                wr(e.nbrs.data(), (size_t)cnt * 4);
            }
        }
        out.commit();
    }

    const uint8_t* nb(size_t v) const { return &search_data[v * RL.vertex_bytes + RL.nb_off]; }
    const float* vec(size_t v) const { return (raw_view ? raw_view : raw.data()) + v * D; }
};

// ---- reference neighbour block <-> device block -----------------------------------------
inline size_t dev_dword_offset(const DevLayout& L, uint32_t plane, uint32_t w, uint32_t i) {
    return plane_dword_offset(L, plane, w, i);
}

// Host restatement of the device re-layout of one block's codes (cph_core.h: `nib`; device_relayout.h).  The
// repackers below read and write the plane-major storage layout; these convert its codes region to the resident
// nibble layout and back.  Aux, ids and count are copied unchanged.  src and dst may be the same block.
inline void block_plane_to_nib(const uint8_t* src, const DevLayout& L, uint8_t* dst) {
    std::vector<uint8_t> out(src, src + L.stride);
    if (L.nib) {
        const uint32_t NW = L.D / 8;  // nibble words per neighbour
        for (uint32_t i = 0; i < 32; ++i)
            for (uint32_t w = 0; w < NW; ++w) {
                uint32_t p[4];
                for (uint32_t b = 0; b < 4; ++b) std::memcpy(&p[b], src + plane_dword_offset(L, b, w / 4, i), 4);
                const uint32_t v = nib_word_from_planes(p[0], p[1], p[2], p[3], w);
                std::memcpy(&out[((size_t)i * NW + w) * 4], &v, 4);
            }
    }
    std::memcpy(dst, out.data(), L.stride);
}
inline void block_nib_to_plane(const uint8_t* src, const DevLayout& L, uint8_t* dst) {
    std::vector<uint8_t> out(src, src + L.stride);
    if (L.nib) {
        const uint32_t NW = L.D / 8;
        for (uint32_t i = 0; i < 32; ++i)
            for (uint32_t pw = 0; pw < L.PW; ++pw) {
                uint32_t n[4];
                std::memcpy(n, src + ((size_t)i * NW + 4 * pw) * 4, 16);
                for (uint32_t b = 0; b < 4; ++b) {
                    const uint32_t v = plane_dword_from_nibs(n[0], n[1], n[2], n[3], b);
                    std::memcpy(&out[plane_dword_offset(L, b, pw, i)], &v, 4);
                }
            }
    }
    std::memcpy(dst, out.data(), L.stride);
}

inline void repack_ref_to_dev(const uint8_t* ref_nb, const RefLayout& RL, const DevLayout& L,
                              uint8_t* dev) {
    std::memset(dev, 0, L.stride);
    const size_t bytes_per_plane_nb = (L.D + 7) / 8;  // code bytes per neighbour per plane
    const size_t plane_stride = round_up(RL.plane_bytes, 64);
    for (uint32_t b = 0; b < L.BW; ++b) {
        const uint8_t* plane = ref_nb + RL.codes + b * plane_stride;
        for (uint32_t w = 0; w < L.PW; ++w)
            for (uint32_t i = 0; i < 32; ++i) {
                uint32_t v = 0;
                for (uint32_t s = 0; s < 4; ++s) {
                    size_t sp = (size_t)4 * w + s;  // byte [sp][i] = dims 8sp..8sp+7
                    if (sp < bytes_per_plane_nb) v |= (uint32_t)plane[sp * 32 + i] << (8 * s);
                }
                std::memcpy(dev + dev_dword_offset(L, b, w, i), &v, 4);
            }
    }
    const float* nop = reinterpret_cast<const float*>(ref_nb + RL.nop);
    const float* ipqo = reinterpret_cast<const float*>(ref_nb + RL.ip_qo);
    const float* ipcp = reinterpret_cast<const float*>(ref_nb + RL.ip_cp);
    const uint16_t* pop = reinterpret_cast<const uint16_t*>(ref_nb + RL.pop);
    const uint16_t* wpop = L.BW > 1 ? reinterpret_cast<const uint16_t*>(ref_nb + RL.wpop) : nullptr;
    for (uint32_t i = 0; i < 32; ++i) {
        uint32_t a[4];
        std::memcpy(&a[0], &nop[i], 4);
        std::memcpy(&a[1], &ipqo[i], 4);
        std::memcpy(&a[2], &ipcp[i], 4);
        a[3] = (uint32_t)pop[i] | ((uint32_t)(wpop ? wpop[i] : 0) << 16);
        std::memcpy(dev + L.aux_off + i * 16, a, 16);
    }
    // slots >= count may hold stale ids in the file (graph_refinement.hpp:46-47); the device
    // copy marks them invalid so that the kernels never need `count` on their critical path
    uint32_t cnt;
    std::memcpy(&cnt, ref_nb + RL.count, 4);
    if (cnt > 32) cnt = 32;
    uint32_t ids[32];
    std::memcpy(ids, ref_nb + RL.ids, 128);
    for (uint32_t i = cnt; i < 32; ++i) ids[i] = kInvalidNode;
    std::memcpy(dev + L.ids_off, ids, 128);
    std::memcpy(dev + L.count_off, &cnt, 4);
}

inline void repack_dev_to_ref(const uint8_t* dev, const DevLayout& L, const RefLayout& RL,
                              uint8_t* ref_nb) {
    std::memset(ref_nb, 0, RL.nb_bytes);
    const size_t bytes_per_plane_nb = (L.D + 7) / 8;
    const size_t plane_stride = round_up(RL.plane_bytes, 64);
    for (uint32_t b = 0; b < L.BW; ++b) {
        uint8_t* plane = ref_nb + RL.codes + b * plane_stride;
        for (uint32_t w = 0; w < L.PW; ++w)
            for (uint32_t i = 0; i < 32; ++i) {
                uint32_t v;
                std::memcpy(&v, dev + dev_dword_offset(L, b, w, i), 4);
                for (uint32_t s = 0; s < 4; ++s) {
                    size_t sp = (size_t)4 * w + s;
                    if (sp < bytes_per_plane_nb) plane[sp * 32 + i] = (uint8_t)(v >> (8 * s));
                }
            }
    }
    for (uint32_t i = 0; i < 32; ++i) {
        uint32_t a[4];
        std::memcpy(a, dev + L.aux_off + i * 16, 16);
        std::memcpy(ref_nb + RL.nop + 4 * i, &a[0], 4);
        std::memcpy(ref_nb + RL.ip_qo + 4 * i, &a[1], 4);
        std::memcpy(ref_nb + RL.ip_cp + 4 * i, &a[2], 4);
        uint16_t p = (uint16_t)(a[3] & 0xFFFF), wp = (uint16_t)(a[3] >> 16);
        std::memcpy(ref_nb + RL.pop + 2 * i, &p, 2);
        if (L.BW > 1) std::memcpy(ref_nb + RL.wpop + 2 * i, &wp, 2);
    }
    std::memcpy(ref_nb + RL.ids, dev + L.ids_off, 128);
    std::memcpy(ref_nb + RL.count, dev + L.count_off, 4);
}

}  // namespace cph
