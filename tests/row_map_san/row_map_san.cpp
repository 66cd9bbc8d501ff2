// row_map_san.cpp -- the host code of the row map under sanitizers (tests/test_row_map_host.py builds this file with
// g++ -fsanitize=address,undefined; no HIP, no GPU).
//
//   row_map_san files  <fixture.idx> <tmpdir>   native file with and without a `rows` section: round trip, the format-1
//                                               bytes of an index without a map, a format-2 file as a format-1 reader
//                                               sees it, malformed `rows` sections
//   row_map_san filter                          rows_filter_host (the statement of cph_filter_create_rows) on exact-size
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

// The format-1 file of `hi`, stated independently of write_native from the layout native_file.h documents: header,
// small fields, then own / raw / blocks, each 4096-aligned, zero padding between them, nothing behind the blocks.
static std::vector<uint8_t> v1_image(const HostIndex& hi, uint32_t stride, const std::vector<uint8_t>& own, uint32_t own_stride,
                                     const std::vector<uint8_t>& blocks) {
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
    auto up = [](uint64_t x) { return (x + 4095) / 4096 * 4096; };
    NativeHeader h{};
    h.magic = kNativeMagic; h.version = 1; h.D = (uint32_t)hi.D; h.bw = (uint32_t)hi.bw; h.dim = (uint32_t)hi.dim;
    h.n = hi.n; h.stride = stride; h.own_stride = own_stride; h.max_level = hi.max_level; h.entry = hi.entry;
    h.upper_tau = hi.upper_tau; h.upper_alpha = hi.upper_alpha; h.mL = hi.mL; h.seed = hi.seed;
    h.has_dup = hi.has_dup_neighbors ? 1u : 0u; h.n_layers = (uint32_t)hi.upper.size();
    h.small_bytes = small.size();
    h.own_off = up(sizeof(NativeHeader) + small.size());
    h.raw_off = up(h.own_off + hi.n * own_stride);
    h.blocks_off = up(h.raw_off + hi.n * hi.D * 4);
    h.file_bytes = h.blocks_off + hi.n * (uint64_t)stride;
    std::vector<uint8_t> img((size_t)h.file_bytes, 0);
    std::memcpy(&img[0], &h, sizeof(h));
    std::memcpy(&img[sizeof(h)], small.data(), small.size());
    std::memcpy(&img[h.own_off], own.data(), hi.n * own_stride);
    std::memcpy(&img[h.raw_off], hi.vec(0), hi.n * hi.D * 4);
    std::memcpy(&img[h.blocks_off], blocks.data(), hi.n * (size_t)stride);
    return img;
}

static int run_files(const std::string& fixture, const std::string& tmp) {
    const std::vector<uint8_t> v2 = slurp(fixture);
    uint32_t D, bw, dim;
    std::memcpy(&D, &v2[12], 4); std::memcpy(&bw, &v2[20], 4); std::memcpy(&dim, &v2[24], 4);
    HostIndex hi;
    hi.load(fixture, D, bw, dim);
    REQUIRE(hi.rows.empty());                                   // a v2 file carries no map
    const size_t n = hi.n;
    const DevLayout DL = make_dev_layout(D, bw);
    const size_t own_stride = hi.RL.nb_off;
    std::vector<uint8_t> blocks(n * DL.stride), own(n * own_stride);
    for (size_t v = 0; v < n; ++v) {
        repack_ref_to_dev(hi.nb(v), hi.RL, DL, &blocks[v * DL.stride]);
        std::memcpy(&own[v * own_stride], &hi.search_data[v * hi.RL.vertex_bytes], own_stride);
    }
    auto rd_native = [&](const std::string& p, HostIndex& t, NativeMapping& map) { return read_native(p, D, bw, dim, t, map); };

    // ---- no map: format 1, byte for byte the documented format-1 layout ----------------------------------------------
    const std::string p1 = tmp + "/plain.cphn";
    write_native(p1, hi, DL.stride, own.data(), (uint32_t)own_stride, blocks.data());
    const std::vector<uint8_t> f1 = slurp(p1);
    REQUIRE(f1 == v1_image(hi, DL.stride, own, (uint32_t)own_stride, blocks));
    {
        HostIndex t;
        NativeMapping map;
        const NativeHeader nh = rd_native(p1, t, map);
        REQUIRE(nh.version == 1 && t.rows.empty() && t.n == n);
    }

    // ---- with a map: format 2, the same map back; and still a file a format-1 reader loads --------------------------
    std::mt19937_64 rng(n * 31 + D);
    HostIndex hm = hi;
    hm.rows.resize(n);
    std::iota(hm.rows.begin(), hm.rows.end(), 0u);
    std::shuffle(hm.rows.begin(), hm.rows.end(), rng);
    const std::string p2 = tmp + "/rows.cphn";
    write_native(p2, hm, DL.stride, own.data(), (uint32_t)own_stride, blocks.data());
    const std::vector<uint8_t> f2 = slurp(p2);
    NativeHeader h1, h2;
    NativeRowsExt x2;
    std::memcpy(&h1, f1.data(), sizeof(h1));
    std::memcpy(&h2, f2.data(), sizeof(h2));
    const size_t xo = sizeof(NativeHeader) + (size_t)h2.small_bytes - sizeof(NativeRowsExt);   // the record ends the small section
    std::memcpy(&x2, f2.data() + xo, sizeof(x2));
    REQUIRE(x2.magic == kNativeRowsMagic && x2.version == 2 && x2.reserved == 0 && x2.rows_off % 4096 == 0);
    REQUIRE(x2.rows_off >= sizeof(NativeHeader) + h2.small_bytes && x2.rows_off + n * 4 <= h2.own_off);
    REQUIRE(std::memcmp(&f2[x2.rows_off], hm.rows.data(), n * 4) == 0);
    // What the format-1 reader of earlier releases demands (index caches are shared between builds): its version, its
    // small fields where it looks for them, the three sections in order, the blocks ending the file.
    REQUIRE(h2.version == 1 && h2.small_bytes == h1.small_bytes + sizeof(NativeRowsExt));
    REQUIRE(std::memcmp(&f2[sizeof(h2)], &f1[sizeof(h1)], (size_t)h1.small_bytes) == 0);
    REQUIRE(sizeof(NativeHeader) + h2.small_bytes <= h2.own_off && h2.own_off + n * own_stride <= h2.raw_off);
    REQUIRE(h2.raw_off + n * hi.D * 4 <= h2.blocks_off && h2.blocks_off + n * DL.stride == h2.file_bytes && h2.file_bytes == f2.size());
    REQUIRE(std::memcmp(&f2[h2.own_off], &f1[h1.own_off], n * own_stride) == 0 && std::memcmp(&f2[h2.raw_off], &f1[h1.raw_off], n * hi.D * 4) == 0);
    REQUIRE(std::memcmp(&f2[h2.blocks_off], &f1[h1.blocks_off], n * DL.stride) == 0);
    {
        NativeHeader a = h1, b = h2;       // apart from the offsets the headers are the same
        a.small_bytes = b.small_bytes = a.own_off = b.own_off = a.raw_off = b.raw_off = a.blocks_off = b.blocks_off = a.file_bytes = b.file_bytes = 0;
        REQUIRE(std::memcmp(&a, &b, sizeof(a)) == 0);
    }
    {
        HostIndex t;
        NativeMapping map;
        const NativeHeader nh = rd_native(p2, t, map);
        REQUIRE(nh.version == 2 && t.rows == hm.rows);
        REQUIRE(t.n == n && t.entry == hi.entry && t.levels == hi.levels && t.norm_sq == hi.norm_sq && t.upper.size() == hi.upper.size());
        REQUIRE(std::memcmp(t.calib, hi.calib, 248) == 0 && std::memcmp(t.vec(0), hi.vec(0), n * hi.D * 4) == 0);
        REQUIRE(std::memcmp(static_cast<const uint8_t*>(map.base) + nh.blocks_off, blocks.data(), blocks.size()) == 0);
        REQUIRE(std::memcmp(static_cast<const uint8_t*>(map.base) + nh.own_off, own.data(), own.size()) == 0);
        // written again from what was read (over the mapped file): the same bytes; and without its map: the format-1 file
        write_native(p2, t, DL.stride, static_cast<const uint8_t*>(map.base) + nh.own_off, (uint32_t)own_stride,
                     static_cast<const uint8_t*>(map.base) + nh.blocks_off);
        REQUIRE(slurp(p2) == f2);
        t.rows.clear();
        write_native(tmp + "/dropped.cphn", t, DL.stride, static_cast<const uint8_t*>(map.base) + nh.own_off, (uint32_t)own_stride,
                     static_cast<const uint8_t*>(map.base) + nh.blocks_off);
        REQUIRE(slurp(tmp + "/dropped.cphn") == f1);
    }
    {   // a map of the wrong length is refused by the writer
        HostIndex bad = hi;
        bad.rows.assign(n - 1, 0u);
        REQUIRE(!attempt([&] { write_native(tmp + "/bad.cphn", bad, DL.stride, own.data(), (uint32_t)own_stride, blocks.data()); }).empty());
    }

    // ---- malformed `rows` sections: an exception, never a fault ------------------------------------------------------
    int rejected = 0, loaded = 0;
    auto try_bytes = [&](const std::vector<uint8_t>& d, size_t len = (size_t)-1) {
        spit(tmp + "/t.cphn", d, len);
        HostIndex t;
        NativeMapping map;
        return attempt([&] { rd_native(tmp + "/t.cphn", t, map); });
    };
    REQUIRE(try_bytes(f2).empty());
    const size_t ro = (size_t)x2.rows_off, xro = xo + offsetof(NativeRowsExt, rows_off);
    for (size_t len : {f2.size() - 1, (size_t)h2.own_off, ro + n * 4, ro + n * 4 - 1, ro + 4, ro, ro - 1, xo + sizeof(NativeRowsExt), xo + 5, xo,
                       sizeof(NativeHeader)}) {
        REQUIRE(!try_bytes(f2, len).empty());                  // truncated behind, inside or in front of the section
        ++rejected;
    }
    auto patched = [&](size_t off, uint64_t val, size_t bytes) {
        std::vector<uint8_t> d = f2;
        std::memcpy(&d[off], &val, bytes);
        return try_bytes(d);
    };
    REQUIRE(patched(ro + 4 * (n / 2), n, 4).rfind("!Corrupt index:", 0) == 0);                   // entry >= n
    REQUIRE(patched(ro + 4 * (n / 2), 0xFFFFFFFFu, 4).rfind("!Corrupt index:", 0) == 0);
    REQUIRE(patched(ro, hm.rows[n - 1], 4).rfind("!Corrupt index:", 0) == 0);                    // entry 0 repeats the last one
    REQUIRE(patched(ro + 4 * (n - 1), hm.rows[3], 4).rfind("!Corrupt index:", 0) == 0);
    REQUIRE(patched(xro, h2.own_off, 8).rfind("!Corrupt index:", 0) == 0);                       // section over `own`
    REQUIRE(patched(xro, h2.own_off - 4, 8).rfind("!Corrupt index:", 0) == 0);                   // ... its last entry
    REQUIRE(patched(xro, ro + 2, 8).rfind("!Corrupt index:", 0) == 0);                           // ... unaligned
    REQUIRE(patched(xro, h2.blocks_off, 8).rfind("!Corrupt index:", 0) == 0);                    // ... over the blocks
    REQUIRE(patched(xro, f2.size(), 8).rfind("!Corrupt index:", 0) == 0);                        // ... behind the file
    REQUIRE(patched(xro, sizeof(NativeHeader), 8).rfind("!Corrupt index:", 0) == 0);             // ... over the small section
    REQUIRE(patched(xro, 0, 8).rfind("!Corrupt index:", 0) == 0);
    REQUIRE(patched(xro, 0xFFFFFFFFFFFFFFFCull, 8).rfind("!Corrupt index:", 0) == 0);            // ... offset + size wraps
    REQUIRE(patched(xo, kNativeRowsMagic ^ 0x100, 8).rfind("!Corrupt index:", 0) == 0);          // not the record
    REQUIRE(!patched(xo + offsetof(NativeRowsExt, version), 3, 4).empty());                       // a format this reader does not know
    REQUIRE(!patched(offsetof(NativeHeader, small_bytes), h2.small_bytes - 8, 8).empty());        // the record cut short
    REQUIRE(!patched(offsetof(NativeHeader, small_bytes), h2.small_bytes + 8, 8).empty());
    REQUIRE(!patched(offsetof(NativeHeader, own_off), ro, 8).empty());                            // `own` over the section
    REQUIRE(!patched(offsetof(NativeHeader, version), 2, 4).empty());                             // the header's field is 1 in every file
    rejected += 18;
    // seeded bit flips in the header, the record and the section: load or throw, nothing else; whatever loads with a
    // map holds a permutation
    for (int it = 0; it < 300; ++it) {
        std::vector<uint8_t> d = f2;
        const int flips = 1 + (int)(rng() % 3);
        for (int k = 0; k < flips; ++k) {
            const uint64_t r = rng() % 3;
            const size_t pos = r == 0 ? (size_t)(rng() % sizeof(NativeHeader)) : r == 1 ? xo + (size_t)(rng() % sizeof(NativeRowsExt))
                                                                                       : ro + (size_t)(rng() % (n * 4));
            d[pos] ^= (uint8_t)(1u << (rng() % 8));
        }
        spit(tmp + "/t.cphn", d);
        HostIndex t;
        NativeMapping map;
        if (attempt([&] { rd_native(tmp + "/t.cphn", t, map); }).empty()) {
            REQUIRE(t.rows.empty() || (t.rows.size() == t.n && is_row_permutation(t.rows.data(), t.n)));
            ++loaded;
        } else {
            ++rejected;
        }
    }
    std::printf("files: ok (%d malformed inputs rejected, %d bit-flipped inputs still loadable)\n", rejected, loaded);
    return 0;
}

static int run_filter() {
    std::mt19937_64 rng(99);
    int cases = 0;
    for (size_t n : {(size_t)1, (size_t)2, (size_t)31, (size_t)32, (size_t)33, (size_t)63, (size_t)64, (size_t)65, (size_t)95,
                     (size_t)96, (size_t)128, (size_t)1000, (size_t)4096, (size_t)50001}) {
        const size_t nw = (n + 31) / 32;
        std::vector<uint32_t> rows(n);
        std::iota(rows.begin(), rows.end(), 0u);
        std::shuffle(rows.begin(), rows.end(), rng);
        REQUIRE(is_row_permutation(rows.data(), n));
        for (int kind = 0; kind < 4; ++kind) {
            // exact-size heap buffers: a read or write one word too far is an ASAN report
            std::vector<uint32_t> in(nw), out(nw, 0xDEADBEEFu);
            for (size_t r = 0; r < n; ++r) {
                const bool b = kind == 0 ? false : kind == 1 ? true : kind == 2 ? (rng() & 1) : (rng() % 100 == 0);
                if (r % 32 == 0) in[r / 32] = 0;
                in[r / 32] |= (uint32_t)b << (r % 32);
            }
            if (n % 32) in[nw - 1] |= ~((1u << (n % 32)) - 1u);      // garbage behind n in the input must not leak out
            rows_filter_host(in.data(), rows.data(), n, out.data());
            size_t pc_in = 0, pc_out = 0;
            for (size_t i = 0; i < n; ++i) {
                const uint32_t want = (in[rows[i] / 32] >> (rows[i] % 32)) & 1u;
                REQUIRE(((out[i / 32] >> (i % 32)) & 1u) == want);
                pc_out += want;
                pc_in += (in[i / 32] >> (i % 32)) & 1u;
            }
            REQUIRE(pc_in == pc_out);                              // the popcount the filter records
            if (n % 32) REQUIRE((out[nw - 1] >> (n % 32)) == 0u);
            ++cases;
        }
    }
    const uint32_t not_perm[4] = {0, 1, 1, 3}, out_of_range[3] = {0, 3, 1};
    REQUIRE(!is_row_permutation(not_perm, 4) && !is_row_permutation(out_of_range, 3) && is_row_permutation(not_perm, 2));
    REQUIRE(is_row_permutation(nullptr, 0));
    std::printf("filter: ok (%d cases)\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "files" && argc == 4) return run_files(argv[2], argv[3]);
    if (mode == "filter") return run_filter();
    std::fprintf(stderr, "usage: row_map_san files <fixture.idx> <tmpdir> | filter\n");
    return 2;
}
