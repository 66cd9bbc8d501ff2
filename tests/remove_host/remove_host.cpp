// remove_host.cpp -- the host code of removed rows under sanitizers (tests/test_remove_host.py builds this file with
// g++ -fsanitize=address,undefined; no HIP, no GPU).
//
//   remove_host files  <fixture.idx> <tmpdir>   native file with a `removed` section (format 3), with and without a row
//                                               map: round trip, the bytes of an index without removed rows, what a
//                                               reader of formats 1 and 2 makes of the record, malformed sections
//   remove_host golden <fixture.idx> <dir> <tmpdir>  this writer against files written by, and shown to, the library of the
//                                               commit before removed rows (run_golden)
//   remove_host filter                          live_filter_host (the statement of the F & ~R kernel) on exact-size
//                                               buffers against a bit-by-bit loop
//
// Every malformed input must end in a C++ exception, never in a sanitizer report.  Exit code 0 = all good.
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
static void spit(const std::string& p, const std::vector<uint8_t>& d, size_t len = (size_t)-1) {
    std::ofstream f(p, std::ios::binary | std::ios::trunc);
    f.write(reinterpret_cast<const char*>(d.data()), (std::streamsize)std::min(len, d.size()));
}
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

// "" = loaded, else the exception's text
template <class F>
static std::string attempt(F&& f) {
    try { f(); return ""; } catch (const std::exception& e) { return std::string("!") + e.what(); }
}
static bool starts(const std::string& s, const char* p) { return s.rfind(p, 0) == 0; }

// What the reader of formats 1 and 2 (the library before removed rows) does with the bytes behind the upper layers,
// restated from its source: nothing, or exactly one 24-byte record with the rows magic; "anything else is damage".
static bool old_reader_accepts_tail(const uint8_t* tail, size_t bytes) {
    if (bytes == 0) return true;
    if (bytes != 24) return false;
    uint64_t magic;
    std::memcpy(&magic, tail, 8);
    return magic == kNativeRowsMagic;
}

static int run_files(const std::string& fixture, const std::string& tmp) {
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
    auto wr = [&](const std::string& p, const HostIndex& t) { write_native(p, t, DL.stride, own.data(), (uint32_t)own_stride, blocks.data()); };
    auto rd = [&](const std::string& p, HostIndex& t, NativeMapping& map) { return read_native(p, D, bw, dim, t, map); };
    std::mt19937_64 rng(n * 131 + D + bw);
    int rejected = 0;

    for (int with_rows = 0; with_rows < 2; ++with_rows) {
        HostIndex base = hi;
        if (with_rows) {
            base.rows.resize(n);
            std::iota(base.rows.begin(), base.rows.end(), 0u);
            std::shuffle(base.rows.begin(), base.rows.end(), rng);
        }
        // ---- R empty: the bytes of the format the index had before (1 without a map, 2 with one) ----------------------
        const std::string p0 = tmp + "/clean.cphn";
        wr(p0, base);
        const std::vector<uint8_t> f0 = slurp(p0);
        NativeHeader h0;
        std::memcpy(&h0, f0.data(), sizeof(h0));
        {
            // independent of the writer: the record-free small section ends where format 1 / 2 end it
            HostIndex t;
            NativeMapping map;
            REQUIRE(rd(p0, t, map).version == (with_rows ? 2u : 1u) && t.n_removed == 0 && t.removed.empty());
            const size_t tail = with_rows ? sizeof(NativeRowsExt) : 0;
            REQUIRE(old_reader_accepts_tail(f0.data() + sizeof(NativeHeader) + h0.small_bytes - tail, tail));
            HostIndex z = base;                 // a bitmap without a set bit is "no removed rows": the same bytes
            z.removed.assign(nw, 0u);
            z.n_removed = 0;
            wr(tmp + "/zero.cphn", z);
            REQUIRE(slurp(tmp + "/zero.cphn") == f0);
        }
        // ---- with R: format 3, the same R back --------------------------------------------------------------------------
        HostIndex hr = base;
        hr.removed.assign(nw, 0u);
        for (size_t i = 0; i < n; ++i)
            if (i == 0 || i == n - 1 || rng() % 4 == 0) { hr.removed[i >> 5] |= 1u << (i & 31); ++hr.n_removed; }
        const std::string p3 = tmp + "/removed.cphn";
        wr(p3, hr);
        const std::vector<uint8_t> f3 = slurp(p3);
        NativeHeader h3;
        std::memcpy(&h3, f3.data(), sizeof(h3));
        const size_t tail3 = sizeof(NativeRemovedExt) + (with_rows ? sizeof(NativeRowsExt) : 0);
        const size_t xo = sizeof(NativeHeader) + (size_t)h3.small_bytes - tail3;
        NativeRemovedExt x3;
        std::memcpy(&x3, f3.data() + xo, sizeof(x3));
        REQUIRE(x3.magic == kNativeRemovedMagic && x3.version == 3 && x3.reserved == 0 && x3.removed_count == hr.n_removed);
        REQUIRE(x3.removed_off % 4096 == 0 && x3.removed_off >= sizeof(NativeHeader) + h3.small_bytes && x3.removed_off + nw * 4 <= h3.own_off);
        REQUIRE(std::memcmp(&f3[x3.removed_off], hr.removed.data(), nw * 4) == 0);
        REQUIRE(h3.version == 1 && h3.small_bytes == h0.small_bytes + sizeof(NativeRemovedExt));
        // a reader of formats 1 and 2 must REFUSE the file (it would bring the removed rows back)
        REQUIRE(!old_reader_accepts_tail(f3.data() + xo, tail3));
        // everything else is the clean file's
        REQUIRE(std::memcmp(&f3[sizeof(h3)], &f0[sizeof(h0)], xo - sizeof(h3)) == 0);
        REQUIRE(std::memcmp(&f3[h3.own_off], &f0[h0.own_off], n * own_stride) == 0 && std::memcmp(&f3[h3.raw_off], &f0[h0.raw_off], n * hi.D * 4) == 0);
        REQUIRE(std::memcmp(&f3[h3.blocks_off], &f0[h0.blocks_off], n * DL.stride) == 0 && h3.file_bytes == f3.size());
        {
            HostIndex t;
            NativeMapping map;
            const NativeHeader nh = rd(p3, t, map);
            REQUIRE(nh.version == 3 && t.removed == hr.removed && t.n_removed == hr.n_removed && t.rows == base.rows);
            REQUIRE(t.n == n && t.entry == hi.entry && t.levels == hi.levels && std::memcmp(t.vec(0), hi.vec(0), n * hi.D * 4) == 0);
            // written again from what was read: the same bytes; without R: the clean file
            write_native(p3, t, DL.stride, static_cast<const uint8_t*>(map.base) + nh.own_off, (uint32_t)own_stride,
                         static_cast<const uint8_t*>(map.base) + nh.blocks_off);
            REQUIRE(slurp(p3) == f3);
            t.removed.clear();
            t.n_removed = 0;
            write_native(tmp + "/back.cphn", t, DL.stride, static_cast<const uint8_t*>(map.base) + nh.own_off, (uint32_t)own_stride,
                         static_cast<const uint8_t*>(map.base) + nh.blocks_off);
            REQUIRE(slurp(tmp + "/back.cphn") == f0);
        }
        {   // the writer refuses a bitmap that does not match its count, its size, or the index
            HostIndex bad = hr;
            bad.n_removed += 1;
            REQUIRE(!attempt([&] { wr(tmp + "/bad.cphn", bad); }).empty());
            bad = hr;
            bad.removed.pop_back();
            REQUIRE(!attempt([&] { wr(tmp + "/bad.cphn", bad); }).empty());
            if (n % 32) {
                bad = hr;
                bad.removed.back() |= 1u << (n % 32);
                REQUIRE(!attempt([&] { wr(tmp + "/bad.cphn", bad); }).empty());
            }
        }
        // ---- malformed sections: the reader's usual errors, never a fault ------------------------------------------------
        auto try_bytes = [&](const std::vector<uint8_t>& d, size_t len = (size_t)-1) {
            spit(tmp + "/t.cphn", d, len);
            HostIndex t;
            NativeMapping map;
            return attempt([&] { rd(tmp + "/t.cphn", t, map); });
        };
        REQUIRE(try_bytes(f3).empty());
        const size_t ro = (size_t)x3.removed_off, xoff = xo + offsetof(NativeRemovedExt, removed_off);
        for (size_t len : {f3.size() - 1, (size_t)h3.own_off, ro + nw * 4, ro + nw * 4 - 1, ro + 2, ro, ro - 1, xo + sizeof(NativeRemovedExt), xo + 9, xo}) {
            REQUIRE(starts(try_bytes(f3, len), "!Read error or truncated file"));     // truncated behind, inside or in front of the section
            ++rejected;
        }
        auto patched = [&](size_t off, uint64_t val, size_t bytes) {
            std::vector<uint8_t> d = f3;
            std::memcpy(&d[off], &val, bytes);
            return try_bytes(d);
        };
        const size_t co = xo + offsetof(NativeRemovedExt, removed_count);
        REQUIRE(starts(patched(co, hr.n_removed + 1, 8), "!Corrupt index:"));                   // a wrong stored count
        REQUIRE(starts(patched(co, hr.n_removed - 1, 8), "!Corrupt index:"));
        REQUIRE(starts(patched(co, 0, 8), "!Corrupt index:"));
        REQUIRE(starts(patched(co, n + 1, 8), "!Corrupt index:"));
        {   // a bit flipped inside the bitmap: the count no longer matches
            std::vector<uint8_t> d = f3;
            d[ro] ^= 2u;
            REQUIRE(starts(try_bytes(d), "!Corrupt index:"));
        }
        if (n % 32) {                                                                          // a bit at id >= n
            std::vector<uint8_t> d = f3;
            uint32_t w;
            std::memcpy(&w, &d[ro + (nw - 1) * 4], 4);
            w |= 1u << (n % 32);
            std::memcpy(&d[ro + (nw - 1) * 4], &w, 4);
            REQUIRE(starts(try_bytes(d), "!Corrupt index:"));
            uint64_t c = hr.n_removed + 1;                                                     // ... also with a count that agrees
            std::memcpy(&d[co], &c, 8);
            REQUIRE(starts(try_bytes(d), "!Corrupt index:"));
        }
        REQUIRE(starts(patched(xoff, h3.own_off, 8), "!Corrupt index:"));                       // section over `own`
        REQUIRE(starts(patched(xoff, ro + 2, 8), "!Corrupt index:"));                           // ... unaligned
        REQUIRE(starts(patched(xoff, h3.blocks_off, 8), "!Corrupt index:"));                    // ... over the blocks
        REQUIRE(starts(patched(xoff, f3.size(), 8), "!Corrupt index:"));                        // ... behind the file
        REQUIRE(starts(patched(xoff, sizeof(NativeHeader), 8), "!Corrupt index:"));             // ... over the small section
        REQUIRE(starts(patched(xoff, 0, 8), "!Corrupt index:"));
        REQUIRE(starts(patched(xoff, 0xFFFFFFFFFFFFFFFCull, 8), "!Corrupt index:"));            // ... offset + size wraps
        REQUIRE(starts(patched(xo, kNativeRemovedMagic ^ 0x100, 8), "!Corrupt index:"));        // not the record
        REQUIRE(starts(patched(xo + offsetof(NativeRemovedExt, version), 4, 4), "!Unsupported native index file version"));
        REQUIRE(starts(patched(xo + offsetof(NativeRemovedExt, reserved), 1, 4), "!Corrupt index:"));
        REQUIRE(!patched(offsetof(NativeHeader, small_bytes), h3.small_bytes - 8, 8).empty());   // the record cut short
        REQUIRE(!patched(offsetof(NativeHeader, small_bytes), h3.small_bytes + 8, 8).empty());
        REQUIRE(!patched(offsetof(NativeHeader, own_off), ro, 8).empty());                       // `own` over the section
        if (with_rows) {                                                                         // the two sections must not overlap
            NativeRowsExt xr;
            std::memcpy(&xr, f3.data() + xo + sizeof(NativeRemovedExt), sizeof(xr));
            REQUIRE(xr.rows_off + n * 4 <= x3.removed_off);
            REQUIRE(starts(patched(xoff, xr.rows_off, 8), "!Corrupt index:"));
            REQUIRE(starts(patched(xo + sizeof(NativeRemovedExt) + offsetof(NativeRowsExt, rows_off), ro, 8), "!Corrupt index:"));
        }
        rejected += 20;
        // seeded bit flips in the header, the record and the section: load or throw, nothing else; whatever loads holds a
        // bitmap that matches its count and has no bit behind n
        for (int it = 0; it < 200; ++it) {
            std::vector<uint8_t> d = f3;
            const int flips = 1 + (int)(rng() % 3);
            for (int k = 0; k < flips; ++k) {
                const uint64_t r = rng() % 3;
                const size_t pos = r == 0 ? (size_t)(rng() % sizeof(NativeHeader)) : r == 1 ? xo + (size_t)(rng() % tail3) : ro + (size_t)(rng() % (nw * 4));
                d[pos] ^= (uint8_t)(1u << (rng() % 8));
            }
            spit(tmp + "/t.cphn", d);
            HostIndex t;
            NativeMapping map;
            if (attempt([&] { rd(tmp + "/t.cphn", t, map); }).empty()) {
                uint64_t pc = 0;
                for (uint32_t x : t.removed) pc += (uint64_t)__builtin_popcount(x);
                REQUIRE(pc == t.n_removed && (t.removed.empty() || t.removed.size() == (t.n + 31) / 32));
                REQUIRE(t.removed.empty() || !(t.n % 32) || (t.removed.back() >> (t.n % 32)) == 0);
            } else {
                ++rejected;
            }
        }
    }
    std::printf("files: ok (%d malformed inputs rejected)\n", rejected);
    return 0;
}

// Files written OUTSIDE this tree's writer (tests/golden/remove_g16_b1_*.cphn.gz, from the g16 1-bit fixture; rows[i] =
// (7 i + 3) mod n; R = every fifth id and the last one):
//   parent_native_f2   written by write_native of the commit before removed rows existed, with the row map
//   native_f3_plain / native_f3_rows   format-3 files that the READER of that commit was run on: it refused both with
//                      "Corrupt index: unknown data behind the upper layers"
// This writer must reproduce all three byte for byte: an index without removed rows is written exactly as the older
// library wrote it, and what this writer makes of an index with removed rows is what the older reader was seen to refuse.
static int run_golden(const std::string& fixture, const std::string& gold, const std::string& tmp) {
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
    auto wr = [&](const std::string& p, const HostIndex& t) { write_native(p, t, DL.stride, own.data(), (uint32_t)own_stride, blocks.data()); return slurp(p); };
    HostIndex with_rows = hi;
    with_rows.rows.resize(n);
    for (size_t i = 0; i < n; ++i) with_rows.rows[i] = (uint32_t)((i * 7 + 3) % n);
    REQUIRE(is_row_permutation(with_rows.rows.data(), n));
    with_rows.removed.assign(nw, 0u);             // a bitmap without a set bit: no removed rows
    REQUIRE(wr(tmp + "/f2.cphn", with_rows) == slurp(gold + "/parent_native_f2.cphn"));
    for (int rows = 0; rows < 2; ++rows) {
        HostIndex h = rows ? with_rows : hi;
        h.removed.assign(nw, 0u);
        for (size_t i = 0; i < n; ++i)
            if (i % 5 == 0 || i == n - 1) { h.removed[i >> 5] |= 1u << (i & 31); ++h.n_removed; }
        const std::string g = gold + (rows ? "/native_f3_rows.cphn" : "/native_f3_plain.cphn");
        REQUIRE(wr(tmp + "/f3.cphn", h) == slurp(g));
        HostIndex t;                                // ... and this reader takes the fixture, with its R
        NativeMapping map;
        REQUIRE(read_native(g, D, bw, dim, t, map).version == 3 && t.removed == h.removed && t.n_removed == h.n_removed && t.rows == h.rows);
    }
    {   // the older library's file loads here as format 2, nothing removed
        HostIndex t;
        NativeMapping map;
        REQUIRE(read_native(gold + "/parent_native_f2.cphn", D, bw, dim, t, map).version == 2 && t.n_removed == 0 && t.rows == with_rows.rows);
    }
    std::printf("golden: ok\n");
    return 0;
}

static int run_filter() {
    std::mt19937_64 rng(77);
    int cases = 0;
    for (size_t n : {(size_t)1, (size_t)31, (size_t)32, (size_t)33, (size_t)300, (size_t)8193}) {
        const size_t nw = (n + 31) / 32;
        for (int with_f = 0; with_f < 2; ++with_f)
            for (int kind = 0; kind < 4; ++kind) {
                // exact-size heap buffers: a read or write one word too far is an ASAN report
                std::vector<uint32_t> f(nw), r(nw), out(nw, 0xDEADBEEFu);
                for (size_t w = 0; w < nw; ++w) {
                    f[w] = kind == 0 ? 0xFFFFFFFFu : (uint32_t)rng();
                    r[w] = kind == 0 ? 0u : kind == 1 ? 0xFFFFFFFFu : kind == 2 ? (uint32_t)rng() : (uint32_t)(rng() & rng() & rng());
                }
                if (n % 32) {                                    // garbage behind n in both inputs: ignored, and clear in the output
                    f[nw - 1] |= ~((1u << (n % 32)) - 1u);
                    if (kind & 1) r[nw - 1] |= ~((1u << (n % 32)) - 1u);
                    else r[nw - 1] &= (1u << (n % 32)) - 1u;
                }
                const uint64_t got = live_filter_host(with_f ? f.data() : nullptr, r.data(), n, out.data());
                uint64_t want = 0;
                for (size_t i = 0; i < n; ++i) {
                    const uint32_t a = with_f ? (f[i / 32] >> (i % 32)) & 1u : 1u, b = (r[i / 32] >> (i % 32)) & 1u;
                    REQUIRE(((out[i / 32] >> (i % 32)) & 1u) == (a & ~b & 1u));
                    want += a & ~b & 1u;
                }
                REQUIRE(got == want);
                if (n % 32) REQUIRE((out[nw - 1] >> (n % 32)) == 0u);
                ++cases;
            }
    }
    std::printf("filter: ok (%d cases)\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "files" && argc == 4) return run_files(argv[2], argv[3]);
    if (mode == "golden" && argc == 5) return run_golden(argv[2], argv[3], argv[4]);
    if (mode == "filter") return run_filter();
    std::fprintf(stderr, "usage: remove_host files <fixture.idx> <tmpdir> | golden <fixture.idx> <golden dir> <tmpdir> | filter\n");
    return 2;
}
