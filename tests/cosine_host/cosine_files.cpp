// cosine_files.cpp -- the native file's metric record (format 4) under sanitizers (tests/test_cosine_host.py builds this
// file with g++ -fsanitize=address,undefined; no HIP, no GPU).
//
//   cosine_files <fixture.idx> <parent_native_f2.cphn> <tmpdir>
//
// On the index of a reference-format fixture, with and without a row map and removed rows: an L2 index is written byte
// for byte as without the metric argument (and, with the row map (7 i + 3) mod n, as the file an older library wrote);
// a cosine index adds one 16-byte record, first behind the upper layers, that the readers of formats 1 to 3 (restated
// from their source) refuse; it reads back with its metric, is refused by a caller that does not ask for the metric, and
// is written again as the same bytes; damaged records end in a C++ exception, never in a sanitizer report.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../rabitq-ann-search_amd/csrc/host_index.h"
#include "../../rabitq-ann-search_amd/csrc/host_parallel.h"
#include "../../rabitq-ann-search_amd/csrc/native_file.h"

using namespace cph;

static std::vector<uint8_t> slurp(const std::string& p) {
    std::ifstream f(p, std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", p.c_str()); std::exit(2); }
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
static void spit(const std::string& p, const std::vector<uint8_t>& d) {
    std::ofstream f(p, std::ios::binary | std::ios::trunc);
    f.write(reinterpret_cast<const char*>(d.data()), (std::streamsize)d.size());
}
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

template <class F>
static std::string attempt(F&& f) {
    try { f(); return ""; } catch (const std::exception& e) { return std::string("!") + e.what(); }
}

// What the readers of formats 1, 2 and 3 (the library before the metric) accept behind the upper layers, restated from
// their source: nothing; 24 bytes that start with the rows magic; 32 bytes that start with the removed-rows magic; 56
// bytes: those 32, then those 24.  "Anything else is damage."
static bool old_reader_accepts_tail(const uint8_t* tail, size_t bytes) {
    auto magic_at = [&](size_t off) { uint64_t m; std::memcpy(&m, tail + off, 8); return m; };
    if (bytes == 0) return true;
    if (bytes == 24) return magic_at(0) == kNativeRowsMagic;
    if (bytes == 32) return magic_at(0) == kNativeRemovedMagic;
    if (bytes == 56) return magic_at(0) == kNativeRemovedMagic && magic_at(32) == kNativeRowsMagic;
    return false;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: cosine_files <fixture.idx> <parent_native_f2.cphn> <tmpdir>\n");
        return 2;
    }
    const std::string fixture = argv[1], parent = argv[2], tmp = argv[3];
    const std::vector<uint8_t> v2 = slurp(fixture);
    uint32_t D, bw, dim;
    std::memcpy(&D, &v2[12], 4); std::memcpy(&bw, &v2[20], 4); std::memcpy(&dim, &v2[24], 4);
    HostIndex hi;
    hi.load(fixture, D, bw, dim);
    const size_t n = hi.n, nw = (n + 31) / 32;
    const DevLayout DL = make_dev_layout(D, bw);
    const size_t own_stride = hi.RL.nb_off;
    std::vector<uint8_t> blocks(n * DL.stride), own(n * own_stride);
    for (size_t v = 0; v < n; ++v) {
        repack_ref_to_dev(hi.nb(v), hi.RL, DL, &blocks[v * DL.stride]);
        std::memcpy(&own[v * own_stride], &hi.search_data[v * hi.RL.vertex_bytes], own_stride);
    }
    auto wr_old = [&](const std::string& p, const HostIndex& t) { write_native(p, t, DL.stride, own.data(), (uint32_t)own_stride, blocks.data()); };
    auto wr = [&](const std::string& p, const HostIndex& t, uint32_t metric) {
        write_native(p, t, DL.stride, own.data(), (uint32_t)own_stride, blocks.data(), metric);
    };
    std::mt19937_64 rng(n * 131 + D + bw);

    {   // an L2 index with the fixture's row map: the bytes an older library wrote
        HostIndex t = hi;
        t.rows.resize(n);
        for (size_t i = 0; i < n; ++i) t.rows[i] = (uint32_t)((7 * i + 3) % n);
        wr(tmp + "/l2_rows.cphn", t, kNativeMetricL2);
        REQUIRE(slurp(tmp + "/l2_rows.cphn") == slurp(parent));
    }

    for (int variant = 0; variant < 4; ++variant) {
        const bool with_rows = variant & 1, with_removed = variant & 2;
        HostIndex base = hi;
        if (with_rows) {
            base.rows.resize(n);
            std::iota(base.rows.begin(), base.rows.end(), 0u);
            std::shuffle(base.rows.begin(), base.rows.end(), rng);
        }
        if (with_removed) {
            base.removed.assign(nw, 0u);
            for (size_t i = 0; i < n; ++i)
                if (i == 0 || i == n - 1 || rng() % 4 == 0) { base.removed[i >> 5] |= 1u << (i & 31); ++base.n_removed; }
        }
        const size_t old_tail = (with_removed ? sizeof(NativeRemovedExt) : 0) + (with_rows ? sizeof(NativeRowsExt) : 0);
        // ---- L2: the file of the writer without a metric, and it reads as L2 ---------------------------------------------
        const std::string p0 = tmp + "/l2.cphn", p1 = tmp + "/cos.cphn";
        wr_old(p0, base);
        const std::vector<uint8_t> f0 = slurp(p0);
        wr(p0, base, kNativeMetricL2);
        REQUIRE(slurp(p0) == f0);
        NativeHeader h0;
        std::memcpy(&h0, f0.data(), sizeof(h0));
        REQUIRE(old_reader_accepts_tail(f0.data() + sizeof(NativeHeader) + h0.small_bytes - old_tail, old_tail));
        {
            HostIndex t;
            NativeMapping map;
            uint32_t metric = 99;
            const NativeHeader nh = read_native(p0, D, bw, dim, t, map, &metric);
            REQUIRE(metric == kNativeMetricL2 && nh.version == (with_removed ? 3u : with_rows ? 2u : 1u));
        }
        // ---- cosine: one more record, first in the trailer ----------------------------------------------------------------
        wr(p1, base, kNativeMetricCosine);
        const std::vector<uint8_t> f1 = slurp(p1);
        NativeHeader h1;
        std::memcpy(&h1, f1.data(), sizeof(h1));
        REQUIRE(h1.version == 1 && h1.small_bytes == h0.small_bytes + sizeof(NativeMetricExt) && h1.file_bytes == f1.size());
        const size_t xo = sizeof(NativeHeader) + (size_t)h1.small_bytes - old_tail - sizeof(NativeMetricExt);
        NativeMetricExt x;
        std::memcpy(&x, f1.data() + xo, sizeof(x));
        REQUIRE(x.magic == kNativeMetricMagic && x.version == 4 && x.metric == kNativeMetricCosine);
        // the readers of formats 1 to 3 must REFUSE the file (they would search cosine rows as squared-L2 data)
        REQUIRE(!old_reader_accepts_tail(f1.data() + xo, old_tail + sizeof(NativeMetricExt)));
        // everything in front of the record is the L2 file's, and so is every section
        REQUIRE(std::memcmp(&f1[sizeof(h1)], &f0[sizeof(h0)], xo - sizeof(h1)) == 0);
        REQUIRE(std::memcmp(&f1[h1.own_off], &f0[h0.own_off], n * own_stride) == 0 && std::memcmp(&f1[h1.raw_off], &f0[h0.raw_off], n * hi.D * 4) == 0);
        REQUIRE(std::memcmp(&f1[h1.blocks_off], &f0[h0.blocks_off], n * DL.stride) == 0);
        {
            HostIndex t;
            NativeMapping map;
            uint32_t metric = 99;
            const NativeHeader nh = read_native(p1, D, bw, dim, t, map, &metric);
            REQUIRE(metric == kNativeMetricCosine && nh.version == 4);
            REQUIRE(t.rows == base.rows && t.removed == base.removed && t.n_removed == base.n_removed);
            REQUIRE(t.n == n && t.entry == hi.entry && t.levels == hi.levels && std::memcmp(t.vec(0), hi.vec(0), n * hi.D * 4) == 0);
            // written again from what was read: the same bytes; as L2: the L2 file
            write_native(tmp + "/again.cphn", t, DL.stride, static_cast<const uint8_t*>(map.base) + nh.own_off, (uint32_t)own_stride,
                         static_cast<const uint8_t*>(map.base) + nh.blocks_off, metric);
            REQUIRE(slurp(tmp + "/again.cphn") == f1);
            write_native(tmp + "/again.cphn", t, DL.stride, static_cast<const uint8_t*>(map.base) + nh.own_off, (uint32_t)own_stride,
                         static_cast<const uint8_t*>(map.base) + nh.blocks_off);
            REQUIRE(slurp(tmp + "/again.cphn") == f0);
        }
        {   // a caller that does not ask for the metric holds L2 rows: refused, and told why
            HostIndex t;
            NativeMapping map;
            const std::string e = attempt([&] { read_native(p1, D, bw, dim, t, map); });
            REQUIRE(e.find("cosine") != std::string::npos && t.n == 0);
        }
        // ---- damaged records --------------------------------------------------------------------------------------------
        auto damaged = [&](size_t off, uint32_t value) {
            std::vector<uint8_t> g = f1;
            std::memcpy(&g[xo + off], &value, 4);
            spit(tmp + "/bad.cphn", g);
            HostIndex t;
            NativeMapping map;
            uint32_t metric = 99;
            return attempt([&] { read_native(tmp + "/bad.cphn", D, bw, dim, t, map, &metric); });
        };
        REQUIRE(damaged(8, 5).find("version") != std::string::npos);           // a later format
        REQUIRE(damaged(12, 7).find("metric") != std::string::npos);           // a metric nobody knows
        REQUIRE(damaged(12, 0).find("metric") != std::string::npos);           // L2 is never written as a record
        REQUIRE(!damaged(0, 0x12345678u).empty());                             // a broken magic: unknown data behind the upper layers
        REQUIRE(!attempt([&] { wr(tmp + "/bad.cphn", base, 2); }).empty());    // the writer refuses a metric it does not know
    }
    std::printf("cosine files: ok\n");
    return 0;
}
