// tags_host.cpp -- the host statements of the tag columns under sanitizers (tests/test_tags_host.py builds this file
// with g++ -fsanitize=address,undefined; no HIP, no GPU).
//
//   tags_host eval <in> <out>   runs tags_canonical_host (with the gather to internal order through `rows`),
//                               tag_tests_canonical_host and tag_filters_host on the caller's data, on exact-size heap
//                               buffers (a read or write one element too far is an ASAN report):
//                               <in>  = u64 n, m, nnz, nvals, has_tags; u64 lims[n + 1]; i32 tags[nnz]; u32 rows[n];
//                                       u32 test_lims[m + 1]; i32 test_vals[nvals]; u8 modes[m]
//                                       (has_tags = 0: the column is given with a NULL tags pointer)
//                               <out> = u64 cnnz; u32 clims[n + 1]; i32 ctags[cnnz]; u32 words[m][(n + 31) / 32];
//                                       u64 counts[m]
//                               The test compares <out> with numpy (tests/tags_model.py).
//   tags_host refuse <in>       the same input; exit code 0 only if the canonicalisation refuses it (std::invalid_argument)
//   tags_host self              the statements against a bit-by-bit loop on random columns, every output buffer
//                               pre-filled with garbage, and the packed test table (tag_tests_pack_host) walked the way
//                               the kernel walks it: four padded values at a time, the compares ORed
//
// Exit code 0 = all good.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <numeric>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../rabitq-ann-search_amd/csrc/host_index.h"

using namespace cph;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

template <class T>
static std::vector<T> read_vec(std::ifstream& f, size_t count) {
    std::vector<T> v(count);
    if (count) f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)));
    REQUIRE(f.good());
    return v;
}
template <class T>
static void write_vec(std::ofstream& f, const std::vector<T>& v) {
    if (!v.empty()) f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

struct Input {
    size_t n = 0, m = 0;
    bool has_tags = true;
    std::vector<uint64_t> lims;
    std::vector<int32_t> tags, test_vals;
    std::vector<uint32_t> rows, test_lims;
    std::vector<uint8_t> modes;
    const int32_t* tags_ptr() const { return has_tags ? tags.data() : nullptr; }
};

static Input read_input(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    REQUIRE(f.good());
    const std::vector<uint64_t> hdr = read_vec<uint64_t>(f, 5);
    Input in;
    in.n = hdr[0];
    in.m = hdr[1];
    in.has_tags = hdr[4] != 0;
    in.lims = read_vec<uint64_t>(f, in.n + 1);
    in.tags = read_vec<int32_t>(f, hdr[2]);
    in.rows = read_vec<uint32_t>(f, in.n);
    in.test_lims = read_vec<uint32_t>(f, in.m + 1);
    in.test_vals = read_vec<int32_t>(f, hdr[3]);
    in.modes = read_vec<uint8_t>(f, in.m);
    return in;
}

static int run_eval(const std::string& path, const std::string& out) {
    const Input in = read_input(path);
    const size_t nw = (in.n + 31) / 32;
    REQUIRE(is_row_permutation(in.rows.data(), in.n));
    std::vector<uint32_t> clims, tl;
    std::vector<int32_t> ctags, tv;
    tags_canonical_host(in.lims.data(), in.tags_ptr(), in.n, in.rows.data(), in.n, clims, ctags);
    REQUIRE(clims.size() == in.n + 1 && clims[in.n] == ctags.size());
    tag_tests_canonical_host(in.test_lims.data(), in.test_vals.data(), in.modes.data(), in.m, tl, tv);
    std::vector<uint32_t> words(in.m * nw, 0xDEADBEEFu);
    std::vector<uint64_t> counts(in.m, 0xDEADBEEFull);
    std::vector<int32_t> exact_tags(ctags), exact_vals(tv);      // exact-size copies (a vector may have spare capacity)
    exact_tags.shrink_to_fit();
    exact_vals.shrink_to_fit();
    tag_filters_host(clims.data(), exact_tags.empty() ? nullptr : exact_tags.data(), in.n, tl.data(),
                     exact_vals.empty() ? nullptr : exact_vals.data(), in.modes.data(), in.m, words.data(), counts.data());
    // cph_get_tags' slice of the whole column is the column
    std::vector<uint64_t> sl(in.n + 1, 0xDEADBEEFull);
    std::vector<int32_t> st(ctags.size(), 0x5EADBEEF);
    tags_slice_host(clims.data(), ctags.data(), 0, in.n, sl.data(), st.empty() ? nullptr : st.data());
    for (size_t i = 0; i <= in.n; ++i) REQUIRE(sl[i] == clims[i]);
    REQUIRE(st == ctags);
    std::ofstream o(out, std::ios::binary | std::ios::trunc);
    write_vec(o, std::vector<uint64_t>{(uint64_t)ctags.size()});
    write_vec(o, clims);
    write_vec(o, ctags);
    write_vec(o, words);
    write_vec(o, counts);
    REQUIRE(o.good());
    std::printf("eval: ok\n");
    return 0;
}

static int run_refuse(const std::string& path) {
    const Input in = read_input(path);
    try {
        std::vector<uint32_t> clims, tl;
        std::vector<int32_t> ctags, tv;
        tags_canonical_host(in.lims.data(), in.tags_ptr(), in.n, in.rows.data(), in.n, clims, ctags);
        tag_tests_canonical_host(in.test_lims.data(), in.test_vals.data(), in.modes.data(), in.m, tl, tv);
    } catch (const std::invalid_argument& e) {
        std::printf("refused: %s\n", e.what());
        return 0;
    }
    std::fprintf(stderr, "accepted\n");
    return 1;
}

// The kernel's walk of one row against the packed table (device_tags.h: tag_walk).
static uint32_t packed_count(const std::vector<uint32_t>& table, size_t vals_at, size_t j, const int32_t* row, uint32_t len) {
    uint32_t c = 0;
    for (uint32_t v = table[j]; v < table[j + 1]; v += kTagTestPad)
        for (uint32_t t = 0; t < len; ++t) {
            bool hit = false;
            for (uint32_t k = 0; k < kTagTestPad; ++k) hit |= row[t] == (int32_t)table[vals_at + v + k];
            c += hit ? 1u : 0u;
        }
    return c;
}

static int run_self() {
    std::mt19937_64 rng(116);
    const int32_t special[] = {INT32_MIN, -1, 0, 1, 5, INT32_MAX};
    int cases = 0;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)31, (size_t)32, (size_t)33, (size_t)63, (size_t)64, (size_t)65, (size_t)2047,
                     (size_t)2048, (size_t)2049, (size_t)4100}) {
        const size_t nw = (n + 31) / 32;
        std::vector<uint64_t> lims(n + 1, 0);
        std::vector<int32_t> tags;
        for (size_t i = 0; i < n; ++i) {                  // unsorted rows with duplicates, a third of them empty
            const size_t len = rng() % 3 == 0 ? 0 : rng() % 12;
            for (size_t t = 0; t < len; ++t) tags.push_back(rng() % 2 ? special[rng() % 6] : (int32_t)(rng() % 20));
            lims[i + 1] = tags.size();
        }
        std::vector<uint32_t> rows(n);
        std::iota(rows.begin(), rows.end(), 0u);
        std::shuffle(rows.begin(), rows.end(), rng);
        std::vector<uint32_t> clims;
        std::vector<int32_t> ctags;
        tags_canonical_host(lims.data(), tags.empty() ? nullptr : tags.data(), n, rows.data(), n, clims, ctags);
        for (size_t i = 0; i < n; ++i) {                  // canonical row i = the set of the given row rows[i]
            const std::set<int32_t> want(tags.begin() + lims[rows[i]], tags.begin() + lims[rows[i] + 1]);
            REQUIRE(std::vector<int32_t>(want.begin(), want.end()) ==
                    std::vector<int32_t>(ctags.begin() + clims[i], ctags.begin() + clims[i + 1]));
        }
        for (size_t m : {(size_t)1, (size_t)3, (size_t)70}) {
            std::vector<uint32_t> test_lims(m + 1, 0);
            std::vector<int32_t> test_vals;
            std::vector<uint8_t> modes(m);
            for (size_t j = 0; j < m; ++j) {
                modes[j] = (uint8_t)((j / 6) % 3);
                switch (j % 6) {
                    case 0: test_vals.push_back(special[(j / 18) % 6]); break;                                 // one value
                    case 1: test_vals.push_back(3); test_vals.push_back(-1); break;                             // two, unsorted
                    case 2: for (int v = 0; v < 64; ++v) test_vals.push_back(v % 2 ? v : -v); break;           // exactly 64
                    case 3: break;                                                                              // the empty set
                    case 4: test_vals.push_back(123456789); break;                                              // nobody's
                    default: for (int v : {7, INT32_MAX, 7, INT32_MIN, 0, 7}) test_vals.push_back(v); break;   // duplicates
                }
                test_lims[j + 1] = (uint32_t)test_vals.size();
            }
            std::vector<uint32_t> tl;
            std::vector<int32_t> tv;
            tag_tests_canonical_host(test_lims.data(), test_vals.data(), modes.data(), m, tl, tv);
            std::vector<uint32_t> words(m * nw, 0xDEADBEEFu), table;
            std::vector<uint64_t> counts(m, 0xDEADBEEFull);
            size_t vals_at = 0;
            tag_filters_host(clims.data(), ctags.data(), n, tl.data(), tv.data(), modes.data(), m, words.data(), counts.data());
            tag_tests_pack_host(tl.data(), tv.data(), modes.data(), m, table, vals_at);
            REQUIRE(vals_at % 4 == 0 && vals_at >= 2 * m + 1);
            for (size_t j = 0; j < m; ++j) {
                const std::set<int32_t> V(test_vals.begin() + test_lims[j], test_vals.begin() + test_lims[j + 1]);
                REQUIRE(tl[j + 1] - tl[j] == V.size());
                REQUIRE(table[j] % kTagTestPad == 0 && table[j + 1] - table[j] == (V.size() + kTagTestPad - 1) / kTagTestPad * kTagTestPad);
                REQUIRE((table[m + 1 + j] & 0xFFu) == modes[j] && (table[m + 1 + j] >> 8) == V.size());
                uint64_t want = 0;
                for (size_t i = 0; i < n; ++i) {
                    uint32_t c = 0;
                    for (uint32_t t = clims[i]; t < clims[i + 1]; ++t) c += (uint32_t)V.count(ctags[t]);
                    REQUIRE(packed_count(table, vals_at, j, ctags.data() + clims[i], clims[i + 1] - clims[i]) == c);
                    const uint32_t bit = modes[j] == kTagsAny ? c > 0 : modes[j] == kTagsAll ? c == V.size() : c == 0;
                    REQUIRE(((words[j * nw + i / 32] >> (i % 32)) & 1u) == bit);
                    want += bit;
                }
                REQUIRE(counts[j] == want);
                if (n % 32) REQUIRE((words[j * nw + nw - 1] >> (n % 32)) == 0u);
                if (j % 6 == 3) REQUIRE(want == (modes[j] == kTagsAny ? 0 : n));
                ++cases;
            }
        }
    }
    std::printf("self: ok (%d filters)\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "eval" && argc == 4) return run_eval(argv[2], argv[3]);
    if (mode == "refuse" && argc == 3) return run_refuse(argv[2]);
    if (mode == "self") return run_self();
    std::fprintf(stderr, "usage: tags_host eval <in> <out> | refuse <in> | self\n");
    return 2;
}
