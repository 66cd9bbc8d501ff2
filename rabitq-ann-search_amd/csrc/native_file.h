// native_file.h — the GPU-native index file (second half).
//
// The reference's v2 file (api/hnsw_index.hpp:217-443) stores every vertex in the AVX2 FastScan layout, so
// loading it means reading 3.4 GB (1M x 128, 4-bit) and re-laying-out every neighbour block on the host
// (0.99 s).  The native file keeps what the GPU reads in the form the GPU reads it:
//
//   header | calibration, profile, centroid, levels, norms, upper layers      (the v2 file's small fields)
//          [ NativeRemovedExt ]  format 3 only: behind the upper layers, in front of the row-map record
//          [ NativeRowsExt ]  format 2 (and a format 3 made from it): the last bytes of the small section
//   rows   [n] u32           4096-aligned, format 2 only: the row map (HostIndex::rows), input row of every internal id
//   removed [(n + 31) / 32] u32  4096-aligned, format 3 only: the removed rows (HostIndex::removed), one bit per internal id
//   own    [n][own_stride]   the vertices' own codes + {nop, ip_qo} (only needed to write a v2 file again)
//   raw    [n][D] f32        4096-aligned
//   blocks [n][stride]       4096-aligned, device block layout (cph_core.h)
//
// Format 1 has no row map; format 2 = format 1 plus the `rows` section and a NativeRowsExt record that names the
// format and the section's offset.  An index without a map is written as format 1, byte for byte what earlier
// releases wrote.  Format 2 is an EXTENSION a format-1 reader can still load: index caches are shared between builds
// of the project (bench.py compares builds on one cached file), so a file written by this library must stay readable
// by the previous one.  A format-1 reader refuses any NativeHeader::version but 1, reads the small section field by
// field and ignores what follows the upper layers, and lets sections start later than the previous one ends.  So
// NativeHeader::version stays 1 -- "what a reader must understand to search the file" -- the record sits at the END
// of the small section (inside small_bytes), and the `rows` section sits in front of `own`, inside file_bytes.  This
// reader returns the file's format (1, 2 or 3) in the `version` field of the header it hands back.
//
// Format 3 = format 1 or 2 plus the `removed` section (cph_remove) and a NativeRemovedExt record; an index without
// removed rows is written as format 1 or 2, byte for byte as before.  Format 3 is NOT an extension an older reader may
// load: it would search the file with the removed rows back in every result.  So the record is laid out to be refused:
// the format-2 reader accepts behind the upper layers nothing, or exactly sizeof(NativeRowsExt) = 24 bytes that start
// with the rows magic, and calls anything else damage ("unknown data behind the upper layers").  NativeRemovedExt is 32
// bytes, starts with its own magic and comes FIRST, so what such a reader finds there is 32 or 56 bytes, never 24 --
// it refuses the file whether or not a row map follows.  (NativeHeader::version stays 1: the sections it names are
// unchanged, and one way of refusing is enough.)  The section sits behind `rows`, in front of `own`.
//
// Format 4 = any of the above plus a NativeMetricExt record: the rows were stored for a metric other than squared L2
// (cosine: every row scaled to squared norm 1/2).  An L2 index is written without the record, byte for byte as before,
// and a file without it is L2.  Like format 3 it must be refused by older readers, which would search cosine rows as L2
// data: the record is 16 bytes, starts with its own magic and comes FIRST behind the upper layers, so an older reader
// finds there 16, 40, 48 or 72 bytes that do not start with a magic it knows -- never nothing, and never 24 bytes that
// start with the rows magic or 32 / 56 that start with the removed-rows magic.  It names no section.
//
// Format 5 = format 4's record with version = 5, metric = 2 (inner product) and two more words: the float M2 the rows
// were augmented against and a zero reserved word -- 24 bytes in the place of 16 (NativeMetricIpExt).  A format-4
// reader refuses it: it finds the metric magic, reads the 16 bytes it knows and rejects version 5 ("Unsupported native
// index file version: 5") before it looks at anything behind them (read_metric_record with newest = 4 is that reader's
// check, and tests/ip_host/ip_host.cpp pins it).  Older readers refuse it like format 4: the 24 bytes do not start
// with the rows magic.  Cosine files stay format 4 and L2 files carry no record: both keep their bytes.
//
// load = mmap + two host-to-device copies straight out of the mapping; the vectors stay mapped for
// cph_get_vectors / save.  A v2 file can always be regenerated from a native one (cph_save after
// cph_load_native): the reference-layout blocks are re-derived from the device blocks.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include <atomic>

#include "host_index.h"
#include "host_parallel.h"

namespace cph {

constexpr uint64_t kNativeMagic = 0x3535334948504300ULL;   // "\0CPHI355"
constexpr uint32_t kNativeVersion = 1;        // NativeHeader::version of every file; the format of one without a row map
constexpr uint32_t kNativeVersionRows = 2;    // NativeRowsExt::version: the format of a file with one
constexpr uint64_t kNativeRowsMagic = 0x53574F5249485043ULL;   // "CPHIROWS"
constexpr uint32_t kNativeVersionRemoved = 3; // NativeRemovedExt::version: the format of a file with removed rows
constexpr uint64_t kNativeRemovedMagic = 0x44564D5249485043ULL;   // "CPHIRMVD"
constexpr uint32_t kNativeVersionMetric = 4;  // NativeMetricExt::version: the format of a file whose rows are not squared-L2 rows
constexpr uint64_t kNativeMetricMagic = 0x5254454D49485043ULL;    // "CPHIMETR"
constexpr uint32_t kNativeMetricL2 = 0, kNativeMetricCosine = 1;  // (CPH_METRIC_L2, CPH_METRIC_COSINE)
constexpr uint32_t kNativeVersionIp = 5;      // NativeMetricIpExt::version: the format of a file of inner-product rows
constexpr uint32_t kNativeMetricIp = 2;       // (CPH_METRIC_IP)

struct NativeHeader {
    uint64_t magic;
    uint32_t version, D, bw, dim;
    uint64_t n;
    uint32_t stride, own_stride;
    int32_t max_level;
    uint32_t entry;
    float upper_tau, upper_alpha;
    double mL;
    uint64_t seed;
    uint32_t has_dup, n_layers;
    uint64_t small_bytes;     // bytes of the small section that follows the header
    uint64_t own_off, raw_off, blocks_off, file_bytes;
};

struct NativeRowsExt {        // format 2: the last sizeof(NativeRowsExt) bytes of the small section
    uint64_t magic;           // kNativeRowsMagic
    uint32_t version;         // kNativeVersionRows
    uint32_t reserved;        // 0
    uint64_t rows_off;        // n x u32, between the small section and `own`
};

struct NativeRemovedExt {     // format 3: behind the upper layers, in front of NativeRowsExt (if any)
    uint64_t magic;           // kNativeRemovedMagic
    uint32_t version;         // kNativeVersionRemoved
    uint32_t reserved;        // 0
    uint64_t removed_off;     // (n + 31) / 32 x u32, between the small section (and `rows`) and `own`
    uint64_t removed_count;   // set bits of the section: 1..n, no bit at or behind n
};
static_assert(sizeof(NativeRemovedExt) != sizeof(NativeRowsExt) && sizeof(NativeRemovedExt) == 32, "a format-2 reader must refuse the record");

struct NativeMetricExt {      // format 4: behind the upper layers, in front of every other record
    uint64_t magic;           // kNativeMetricMagic
    uint32_t version;         // kNativeVersionMetric
    uint32_t metric;          // kNativeMetricCosine (0, squared L2, is never written: such a file has no record)
};
static_assert(sizeof(NativeMetricExt) == 16, "older readers must refuse the record by its size");

struct NativeMetricIpExt {    // format 5: in the place of NativeMetricExt
    uint64_t magic;           // kNativeMetricMagic
    uint32_t version;         // kNativeVersionIp
    uint32_t metric;          // kNativeMetricIp
    float m2;                 // the bound the rows were augmented against: finite, >= 0
    uint32_t reserved;        // 0
};
static_assert(sizeof(NativeMetricIpExt) == 24 && offsetof(NativeMetricIpExt, version) == offsetof(NativeMetricExt, version),
              "a format-4 reader must find the version where it looks for it");

// The metric record at p (avail bytes are readable), as a reader that knows formats up to `newest` (4 or 5) takes it:
// returns the bytes the record occupies, 0 when p does not start with the metric magic.  A version above `newest` is
// refused before any byte behind the first 16 is read.
inline size_t read_metric_record(const uint8_t* p, size_t avail, uint32_t newest, uint32_t* metric, float* m2) {
    NativeMetricExt e{};
    if (avail < sizeof(e)) return 0;
    std::memcpy(&e, p, sizeof(e));
    if (e.magic != kNativeMetricMagic) return 0;
    if (e.version != kNativeVersionMetric && !(e.version == kNativeVersionIp && newest >= kNativeVersionIp))
        throw std::runtime_error("Unsupported native index file version: " + std::to_string(e.version));
    if (e.version == kNativeVersionMetric) {
        if (e.metric != kNativeMetricCosine) throw std::runtime_error("Corrupt index: unknown metric " + std::to_string(e.metric));
        *metric = e.metric;
        *m2 = 0.0f;
        return sizeof(e);
    }
    NativeMetricIpExt x{};
    if (e.metric != kNativeMetricIp || avail < sizeof(x))
        throw std::runtime_error("Corrupt index: a version-5 metric record holds the inner-product metric and its bound, not metric " +
                                 std::to_string(e.metric));
    std::memcpy(&x, p, sizeof(x));
    if (!(x.m2 >= 0.0f && x.m2 < std::numeric_limits<float>::infinity()) || x.reserved != 0)
        throw std::runtime_error("Corrupt index: bad inner-product bound");
    *metric = x.metric;
    *m2 = x.m2;
    return sizeof(x);
}

struct NativeMapping {
    void* base = nullptr;
    size_t bytes = 0;
    NativeMapping() = default;
    NativeMapping(const NativeMapping&) = delete;
    NativeMapping& operator=(const NativeMapping&) = delete;
    NativeMapping(NativeMapping&& o) noexcept : base(o.base), bytes(o.bytes) { o.base = nullptr; o.bytes = 0; }
    NativeMapping& operator=(NativeMapping&& o) noexcept {
        if (this != &o) { reset(); base = o.base; bytes = o.bytes; o.base = nullptr; o.bytes = 0; }
        return *this;
    }
    void reset() {
        if (base) munmap(base, bytes);
        base = nullptr;
        bytes = 0;
    }
    ~NativeMapping() { reset(); }
};

inline uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// `own` = [n][own_stride] vertex headers, `blocks` = [n][stride] device blocks (both host pointers).
inline void write_native(const std::string& path, const HostIndex& hi, uint32_t stride, const uint8_t* own,
                         uint32_t own_stride, const uint8_t* blocks, uint32_t metric = kNativeMetricL2, const float* ip_m2 = nullptr) {
    std::vector<uint8_t> small;
    auto put = [&](const void* p, size_t b) { const uint8_t* q = static_cast<const uint8_t*>(p); small.insert(small.end(), q, q + b); };
    put(hi.calib, 248);
    put(hi.profile, 72);
    put(hi.centroid.data(), hi.dim * 4);
    put(hi.levels.data(), hi.n * 4);
    put(hi.norm_sq.data(), hi.n * 4);
    for (const auto& layer : hi.upper) {
        const uint32_t sz = (uint32_t)layer.size();
        put(&sz, 4);
        for (const auto& e : layer) {
            const uint32_t cnt = (uint32_t)e.nbrs.size();
            put(&e.node, 4);
            put(&cnt, 4);
            put(e.nbrs.data(), (size_t)cnt * 4);
        }
    }
    const bool with_rows = !hi.rows.empty();
    if (with_rows && hi.rows.size() != hi.n) throw std::runtime_error("row map does not match the index size");
    const bool with_removed = hi.n_removed != 0;
    const uint64_t rm_words = (hi.n + 31) / 32;
    if (with_removed) {
        uint64_t pc = 0;
        if (hi.removed.size() != rm_words) throw std::runtime_error("removed-row bitmap does not match the index size");
        for (uint32_t x : hi.removed) pc += (uint64_t)__builtin_popcount(x);
        if (pc != hi.n_removed || ((hi.n & 31) && (hi.removed.back() >> (hi.n & 31))))
            throw std::runtime_error("removed-row bitmap does not match its count");
    }
    if (metric != kNativeMetricL2 && metric != kNativeMetricCosine && metric != kNativeMetricIp) throw std::runtime_error("unknown metric");
    // (inner-product rows mean nothing without the bound they were augmented against)
    if (metric == kNativeMetricIp && !(ip_m2 && *ip_m2 >= 0.0f && *ip_m2 < std::numeric_limits<float>::infinity()))
        throw std::runtime_error("the inner-product metric is written with its bound");
    const bool with_metric = metric != kNativeMetricL2;
    uint64_t rows_off = 0, removed_off = 0;
    const uint64_t records = (with_rows ? sizeof(NativeRowsExt) : 0) + (with_removed ? sizeof(NativeRemovedExt) : 0) +
                             (!with_metric ? 0 : metric == kNativeMetricIp ? sizeof(NativeMetricIpExt) : sizeof(NativeMetricExt));
    uint64_t sections_end = sizeof(NativeHeader) + small.size() + records;
    if (metric == kNativeMetricIp) {
        const NativeMetricIpExt ext{kNativeMetricMagic, kNativeVersionIp, metric, *ip_m2, 0u};
        put(&ext, sizeof(ext));
    } else if (with_metric) {
        const NativeMetricExt ext{kNativeMetricMagic, kNativeVersionMetric, metric};
        put(&ext, sizeof(ext));
    }
    if (with_rows) {
        rows_off = align_up(sections_end, 4096);
        sections_end = rows_off + hi.n * 4;
    }
    if (with_removed) {
        removed_off = align_up(sections_end, 4096);
        sections_end = removed_off + rm_words * 4;
        const NativeRemovedExt ext{kNativeRemovedMagic, kNativeVersionRemoved, 0u, removed_off, hi.n_removed};
        put(&ext, sizeof(ext));
    }
    if (with_rows) {
        const NativeRowsExt ext{kNativeRowsMagic, kNativeVersionRows, 0u, rows_off};
        put(&ext, sizeof(ext));
    }
    NativeHeader h{};
    h.magic = kNativeMagic; h.version = kNativeVersion; h.D = (uint32_t)hi.D; h.bw = (uint32_t)hi.bw; h.dim = (uint32_t)hi.dim;
    h.n = hi.n; h.stride = stride; h.own_stride = own_stride; h.max_level = hi.max_level; h.entry = hi.entry;
    h.upper_tau = hi.upper_tau; h.upper_alpha = hi.upper_alpha; h.mL = hi.mL; h.seed = hi.seed;
    h.has_dup = hi.has_dup_neighbors ? 1u : 0u; h.n_layers = (uint32_t)hi.upper.size();
    h.small_bytes = small.size();
    h.own_off = align_up(sections_end, 4096);
    h.raw_off = align_up(h.own_off + hi.n * own_stride, 4096);
    h.blocks_off = align_up(h.raw_off + hi.n * hi.D * 4, 4096);
    h.file_bytes = h.blocks_off + hi.n * (uint64_t)stride;
    AtomicFile out(path);       // saving over the file this handle is mapped from keeps the old inode mapped
    uint64_t pos = 0;
    auto wr = [&](const void* p, size_t b) { out.write(p, b); pos += b; };
    auto pad_to = [&](uint64_t off) {
        std::vector<uint8_t> z((size_t)(off - pos), 0);
        wr(z.data(), z.size());
    };
    wr(&h, sizeof(h));
    wr(small.data(), small.size());
    if (with_rows) {
        pad_to(rows_off);
        wr(hi.rows.data(), hi.n * 4);
    }
    if (with_removed) {
        pad_to(removed_off);
        wr(hi.removed.data(), rm_words * 4);
    }
    pad_to(h.own_off);
    wr(own, hi.n * own_stride);
    pad_to(h.raw_off);
    wr(hi.vec(0), hi.n * hi.D * 4);
    pad_to(h.blocks_off);
    wr(blocks, hi.n * (uint64_t)stride);
    out.commit();
}

// Maps the file and fills everything of `hi` except raw / search_data (raw_view points into the mapping); hi.rows is
// the file's row map (format 2) or empty (format 1), hi.removed / hi.n_removed the file's removed rows (format 3) or
// none; the returned header's `version` is that format.  *metric: the file's metric (formats 4 and 5; L2 without the
// record) -- a caller that does not ask cannot hold anything but L2 rows, and is refused a file of another metric.
// *ip_m2: the bound of an inner-product file (format 5); a caller that does not ask is refused such a file.
inline NativeHeader read_native(const std::string& path, size_t expect_D, size_t expect_bw, size_t expect_dim, HostIndex& hi,
                                NativeMapping& map, uint32_t* metric = nullptr, float* ip_m2 = nullptr) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0) throw std::runtime_error("Cannot open file for reading: " + path);
    struct stat st{};
    if (fstat(fd, &st) != 0 || (size_t)st.st_size < sizeof(NativeHeader)) { ::close(fd); throw std::runtime_error("Read error or truncated file: " + path); }
    void* base = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (base == MAP_FAILED) throw std::runtime_error("Cannot map file: " + path);
    NativeMapping m;
    m.base = base;
    m.bytes = (size_t)st.st_size;
    NativeHeader h;
    std::memcpy(&h, base, sizeof(h));
    if (h.magic != kNativeMagic) throw std::runtime_error("Invalid magic bytes (not a CP-HNSW MI355X native index file).");
    if (h.version != kNativeVersion) throw std::runtime_error("Unsupported native index file version: " + std::to_string(h.version));
    if (h.D != expect_D || h.bw != expect_bw)
        throw std::runtime_error("Index file template parameters mismatch: file D=" + std::to_string(h.D) + " R=32 BW=" +
                                 std::to_string(h.bw) + ", expected D=" + std::to_string(expect_D) + " R=32 BW=" + std::to_string(expect_bw));
    if (h.dim != expect_dim)
        throw std::runtime_error("Index file dim=" + std::to_string(h.dim) + " mismatches Index dim=" + std::to_string(expect_dim));
    // Nothing below trusts the header: every section must lie inside the mapping, in order and without overlap,
    // with the strides this library computes itself (a wrong offset would otherwise be a SIGBUS in a memcpy, which
    // no exception handler catches).
    {
        typedef unsigned __int128 u128;
        const DevLayout DL = make_dev_layout(h.D, h.bw);
        const RefLayout RLc = make_ref_layout(h.D, h.bw);
        const bool ok = h.n >= 1 && h.n < 0xFFFFFFFFull && h.stride == DL.stride && h.own_stride == RLc.nb_off &&
                        h.n_layers <= 64 &&
                        (u128)sizeof(NativeHeader) + h.small_bytes <= h.own_off &&
                        (u128)h.own_off + (u128)h.n * h.own_stride <= h.raw_off &&
                        (u128)h.raw_off + (u128)h.n * h.D * 4 <= h.blocks_off &&
                        (u128)h.blocks_off + (u128)h.n * h.stride == h.file_bytes && h.file_bytes <= m.bytes &&
                        h.raw_off % 4 == 0 && h.blocks_off % 4 == 0 &&
                        (u128)h.small_bytes >= (u128)320 + (u128)h.dim * 4 + (u128)h.n * 8;
        if (!ok) throw std::runtime_error("Read error or truncated file: " + path);
        if (h.entry != kInvalidNode && h.entry >= h.n) throw std::runtime_error("Corrupt index: entry point out of range");
    }
    HostIndex t;
    t.D = h.D; t.bw = h.bw; t.dim = h.dim; t.n = h.n; t.max_level = h.max_level; t.entry = h.entry;
    t.upper_tau = h.upper_tau; t.upper_alpha = h.upper_alpha; t.mL = h.mL; t.seed = h.seed;
    t.has_dup_neighbors = h.has_dup != 0;
    t.RL = make_ref_layout(t.D, t.bw);
    const uint8_t* p = static_cast<const uint8_t*>(base) + sizeof(NativeHeader);
    const uint8_t* end = p + h.small_bytes;
    auto get = [&](void* dst, size_t b) {
        if (p + b > end) throw std::runtime_error("Read error or truncated file: " + path);
        std::memcpy(dst, p, b);
        p += b;
    };
    get(t.calib, 248);
    get(t.profile, 72);
    t.centroid.resize(t.dim);  get(t.centroid.data(), t.dim * 4);
    t.levels.resize(t.n);      get(t.levels.data(), t.n * 4);
    t.norm_sq.resize(t.n);     get(t.norm_sq.data(), t.n * 4);
    t.upper.resize(h.n_layers);
    for (auto& layer : t.upper) {
        uint32_t sz = 0;
        get(&sz, 4);
        if (sz > t.n) throw std::runtime_error("Corrupt index: upper layer larger than the index");
        layer.resize(sz);
        for (auto& e : layer) {
            uint32_t cnt = 0;
            get(&e.node, 4);
            get(&cnt, 4);
            if ((size_t)cnt * 4 > (size_t)(end - p)) throw std::runtime_error("Read error or truncated file: " + path);
            e.nbrs.resize(cnt);
            get(e.nbrs.data(), (size_t)cnt * 4);
            if (e.node >= t.n) throw std::runtime_error("Corrupt index: upper-layer node out of range");
            for (uint32_t x : e.nbrs)
                if (x >= t.n) throw std::runtime_error("Corrupt index: upper-layer neighbour out of range");
        }
    }
    // What follows the upper layers: nothing (format 1), the row-map record (format 2), or the removed-rows record with
    // or without the row-map record behind it (format 3); anything else is damage.
    // In front of them the metric record (formats 4 and 5), told by its magic.
    bool with_rows = false, with_removed = false, with_metric = false;
    NativeRowsExt ext{};
    NativeRemovedExt rext{};
    uint32_t file_metric = kNativeMetricL2;
    float file_m2 = 0.0f;
    const uint64_t rm_words = (h.n + 31) / 32;
    if (const size_t b = read_metric_record(p, (size_t)(end - p), kNativeVersionIp, &file_metric, &file_m2)) {
        p += b;
        with_metric = true;
    }
    if (with_metric && !metric)
        throw std::runtime_error(file_metric == kNativeMetricIp
                                     ? "The file holds inner-product rows: it loads into an index created with the inner-product metric only."
                                     : "The file holds cosine rows: it loads into an index created with the cosine metric only.");
    if (file_metric == kNativeMetricIp && !ip_m2)
        throw std::runtime_error("The file holds inner-product rows: it loads into an index created with the inner-product metric only.");
    if (metric) *metric = file_metric;
    if (ip_m2) *ip_m2 = file_m2;
    if ((size_t)(end - p) == sizeof(rext) || (size_t)(end - p) == sizeof(rext) + sizeof(ext)) {
        typedef unsigned __int128 u128;
        get(&rext, sizeof(rext));
        if (rext.magic != kNativeRemovedMagic) throw std::runtime_error("Corrupt index: unknown data behind the upper layers");
        if (rext.version != kNativeVersionRemoved)
            throw std::runtime_error("Unsupported native index file version: " + std::to_string(rext.version));
        if (rext.reserved != 0 || rext.removed_off % 4 != 0 || (u128)rext.removed_off < (u128)sizeof(NativeHeader) + h.small_bytes ||
            (u128)rext.removed_off + (u128)rm_words * 4 > h.own_off)
            throw std::runtime_error("Corrupt index: removed-rows section out of bounds");
        if (rext.removed_count == 0 || rext.removed_count > h.n) throw std::runtime_error("Corrupt index: removed-rows count out of range");
        with_removed = true;
    }
    if (p != end) {
        typedef unsigned __int128 u128;
        if ((size_t)(end - p) != sizeof(ext)) throw std::runtime_error("Corrupt index: unknown data behind the upper layers");
        get(&ext, sizeof(ext));
        if (ext.magic != kNativeRowsMagic) throw std::runtime_error("Corrupt index: unknown data behind the upper layers");
        if (ext.version != kNativeVersionRows)
            throw std::runtime_error("Unsupported native index file version: " + std::to_string(ext.version));
        if (ext.rows_off % 4 != 0 || (u128)ext.rows_off < (u128)sizeof(NativeHeader) + h.small_bytes ||
            (u128)ext.rows_off + (u128)h.n * 4 > h.own_off)
            throw std::runtime_error("Corrupt index: row map section out of bounds");
        // (sections in order, no overlap: the row map lies in front of the removed rows)
        if (with_removed && (u128)ext.rows_off + (u128)h.n * 4 > rext.removed_off)
            throw std::runtime_error("Corrupt index: row map section out of bounds");
        with_rows = true;
        h.version = kNativeVersionRows;      // the format, for the caller (the file's field stays 1, see the top)
    }
    if (with_removed) h.version = kNativeVersionRemoved;
    if (with_metric) h.version = file_metric == kNativeMetricIp ? kNativeVersionIp : kNativeVersionMetric;
    // The device blocks are handed to the GPU as they are: a neighbour id the search kernel would chase must be a
    // vertex (the v2 loader's validate() makes the same promise), unused slots must carry the invalid marker the
    // kernels rely on instead of `count`, and the repeated-id flag is recomputed rather than believed.
    {
        const DevLayout DL = make_dev_layout(h.D, h.bw);
        const uint8_t* blocks = static_cast<const uint8_t*>(base) + h.blocks_off;
        std::atomic<int> bad{0}, dup{0};
        parallel_for(t.n, 4096, [&](size_t lo, size_t hi_) {
            int b = 0, d = 0;
            for (size_t v = lo; v < hi_ && !b; ++v) {
                const uint8_t* blk = blocks + v * (size_t)DL.stride;
                uint32_t cnt, ids[32];
                std::memcpy(&cnt, blk + DL.count_off, 4);
                std::memcpy(ids, blk + DL.ids_off, 128);
                if (cnt > 32) { b = 1; break; }
                for (uint32_t i = 0; i < 32; ++i) {
                    if (i < cnt) {
                        if (ids[i] >= t.n) b = 2;
                        for (uint32_t j = 0; j < i; ++j) d |= ids[j] == ids[i];
                    } else if (ids[i] != kInvalidNode) b = 3;
                }
            }
            if (b) bad.store(b);
            if (d) dup.store(1);
        });
        if (bad.load() == 1) throw std::runtime_error("Corrupt index: neighbour count > 32");
        if (bad.load()) throw std::runtime_error("Corrupt index: neighbour id out of range");
        t.has_dup_neighbors = dup.load() != 0;
    }
    if (with_rows) {
        t.rows.resize(t.n);
        std::memcpy(t.rows.data(), static_cast<const uint8_t*>(base) + ext.rows_off, t.n * 4);
        if (!is_row_permutation(t.rows.data(), t.n)) throw std::runtime_error("Corrupt index: the row map is not a permutation");
    }
    if (with_removed) {
        t.removed.resize(rm_words);
        std::memcpy(t.removed.data(), static_cast<const uint8_t*>(base) + rext.removed_off, rm_words * 4);
        uint64_t pc = 0;
        for (uint32_t x : t.removed) pc += (uint64_t)__builtin_popcount(x);
        if ((h.n & 31) && (t.removed.back() >> (h.n & 31))) throw std::runtime_error("Corrupt index: removed row behind the last id");
        if (pc != rext.removed_count) throw std::runtime_error("Corrupt index: removed-rows count does not match the bitmap");
        t.n_removed = pc;
    }
    t.raw_view = reinterpret_cast<const float*>(static_cast<const uint8_t*>(base) + h.raw_off);
    t.rot.init(t.D, t.seed);
    hi = std::move(t);
    map = std::move(m);
    return h;
}

}  // namespace cph
