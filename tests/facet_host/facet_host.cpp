// facet_host.cpp -- the host statements of the facet counts under sanitizers (tests/test_facet_host.py builds this file
// with g++ -fsanitize=address,undefined; no HIP, no GPU).
//
//   facet_host eval <in> <out>  runs facet_dictionary_host, facet_counts_host and facet_top_host on the caller's data, every
//                               bitmap in an exact-size heap buffer of its own (a read one word too far is an ASAN report):
//                               <in>  = u64 n, m, n_entries, is_tags, has_removed, K; u64 lims[n + 1] (is_tags only);
//                                       i32 column[n_entries]; u8 present[m]; u32 words[m][(n + 31) / 32];
//                                       u32 removed[(n + 31) / 32] (has_removed only)
//                                       (present[j] = 0: filter j is "every row", its words are skipped)
//                               <out> = u64 U, entries; i32 values[U]; u32 codes[entries]; u64 counts[m][U];
//                                       i32 top_values[m][K]; u64 top_counts[m][K]; u32 found[m]
//                               A tag column is canonicalised first (tags_canonical_host), as cph_set_tags does.
//                               The test compares <out> with numpy (tests/facet_model.py).
//   facet_host refuse           every refusal of the statements must throw std::invalid_argument
//   facet_host self             the statements against a bit-by-bit loop on random columns, every output pre-filled with
//                               garbage
//
// Exit code 0 = all good.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
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

static int run_eval(const std::string& path, const std::string& out) {
    std::ifstream f(path, std::ios::binary);
    REQUIRE(f.good());
    const std::vector<uint64_t> hdr = read_vec<uint64_t>(f, 6);
    const size_t n = hdr[0], m = hdr[1], n_entries = hdr[2], K = hdr[5], nw = (n + 31) / 32;
    const bool is_tags = hdr[3] != 0, has_removed = hdr[4] != 0;
    std::vector<uint64_t> lims;
    if (is_tags) lims = read_vec<uint64_t>(f, n + 1);
    std::vector<int32_t> column = read_vec<int32_t>(f, n_entries);
    const std::vector<uint8_t> present = read_vec<uint8_t>(f, m);
    std::vector<std::vector<uint32_t>> words(m);
    for (size_t j = 0; j < m; ++j) words[j] = read_vec<uint32_t>(f, nw);
    std::vector<uint32_t> removed;
    if (has_removed) removed = read_vec<uint32_t>(f, nw);

    std::vector<uint32_t> clims;
    if (is_tags) {
        std::vector<int32_t> ctags;
        tags_canonical_host(lims.data(), n_entries ? column.data() : nullptr, n, nullptr, 0, clims, ctags);
        column.swap(ctags);
    }
    std::vector<int32_t> values;
    std::vector<uint32_t> codes;
    facet_dictionary_host(column.empty() ? nullptr : column.data(), column.size(), values, codes);
    const size_t U = values.size();
    std::vector<const uint32_t*> fs(m);
    for (size_t j = 0; j < m; ++j) fs[j] = present[j] ? words[j].data() : nullptr;
    std::vector<uint64_t> counts(m * U, 0xDEADBEEFDEADBEEFull);
    facet_counts_host(codes.data(), is_tags ? clims.data() : nullptr, n, U, fs.data(), has_removed ? removed.data() : nullptr, m, counts.data());
    std::vector<int32_t> tv(m * K, 0x5A5A5A5A);
    std::vector<uint64_t> tc(m * K, 0xDEADBEEFDEADBEEFull);
    std::vector<uint32_t> found(m, 0xDEADBEEFu);
    for (size_t j = 0; j < m; ++j)
        facet_top_host(counts.data() + j * U, values.data(), U, K, tv.data() + j * K, tc.data() + j * K, found.data() + j);

    std::ofstream o(out, std::ios::binary);
    write_vec(o, std::vector<uint64_t>{U, codes.size()});
    write_vec(o, values);
    write_vec(o, codes);
    write_vec(o, counts);
    write_vec(o, tv);
    write_vec(o, tc);
    write_vec(o, found);
    REQUIRE(o.good());
    std::printf("eval: ok\n");
    return 0;
}

template <class Call>
static int refused(Call call) {
    try {
        call();
    } catch (const std::invalid_argument& e) {
        std::printf("refused: %s\n", e.what());
        return 1;
    }
    return 0;
}

static int run_refuse() {
    const std::vector<uint32_t> codes = {0, 1, 2}, lims_ok = {0, 1, 3}, lims_from_1 = {1, 1, 3}, lims_down = {0, 2, 1};
    const std::vector<int32_t> values = {5, 6, 7};
    std::vector<uint64_t> counts(3, 0), one = {1, 1, 1}, tc(2000, 0);
    std::vector<int32_t> tv(2000, 0);
    uint32_t found = 0;
    int n = 0;
    n += refused([&] { facet_counts_host(codes.data(), nullptr, 3, 2, nullptr, nullptr, 1, counts.data()); });              // a code >= U
    n += refused([&] { facet_counts_host(codes.data(), lims_from_1.data(), 2, 3, nullptr, nullptr, 1, counts.data()); });
    n += refused([&] { facet_counts_host(codes.data(), lims_down.data(), 2, 3, nullptr, nullptr, 1, counts.data()); });
    n += refused([&] { facet_top_host(one.data(), values.data(), 3, 0, tv.data(), tc.data(), &found); });
    n += refused([&] { facet_top_host(one.data(), values.data(), 3, 1025, tv.data(), tc.data(), &found); });
    REQUIRE(n == 5);
    REQUIRE(counts[0] == 0 && counts[1] == 0 && counts[2] == 0 && found == 0 && tv[0] == 0 && tc[0] == 0);                   // nothing written
    // the limits themselves pass
    facet_counts_host(codes.data(), lims_ok.data(), 2, 3, nullptr, nullptr, 1, counts.data());
    REQUIRE(counts[0] == 1 && counts[1] == 1 && counts[2] == 1);
    facet_top_host(one.data(), values.data(), 3, 1024, tv.data(), tc.data(), &found);
    REQUIRE(found == 3 && tv[0] == 5 && tv[2] == 7 && tv[3] == 0 && tc[3] == 0);
    std::printf("refuse: ok\n");
    return 0;
}

static int run_self() {
    std::mt19937_64 rng(4242);
    const int32_t special[4] = {INT_MIN, -1, 0, INT_MAX};
    for (size_t n : {0, 1, 31, 32, 33, 64, 65, 257, 1000}) {
        for (int tags = 0; tags < 2; ++tags) {
            const size_t nw = (n + 31) / 32, m = 3;
            std::vector<uint32_t> lims(n + 1, 0);
            std::vector<int32_t> col;
            for (size_t i = 0; i < n; ++i) {
                std::set<int32_t> row;                                           // (a tag row: ascending and distinct, maybe empty)
                const size_t len = tags ? rng() % 4 : 1;
                for (size_t t = 0; t < len; ++t) row.insert(rng() % 7 == 0 ? special[rng() % 4] : (int32_t)(rng() % 12) - 3);
                col.insert(col.end(), row.begin(), row.end());
                lims[i + 1] = (uint32_t)col.size();
            }
            std::vector<int32_t> values;
            std::vector<uint32_t> codes;
            facet_dictionary_host(col.empty() ? nullptr : col.data(), col.size(), values, codes);
            const size_t U = values.size();
            for (size_t u = 1; u < U; ++u) REQUIRE(values[u - 1] < values[u]);
            for (size_t e = 0; e < col.size(); ++e) REQUIRE(codes[e] < U && values[codes[e]] == col[e]);
            std::vector<std::vector<uint32_t>> words(m, std::vector<uint32_t>(nw));
            std::vector<uint32_t> removed(nw);
            for (auto& w : words)
                for (auto& x : w) x = (uint32_t)rng();                           // (dirty bits behind n included)
            for (auto& x : removed) x = (uint32_t)rng() & (uint32_t)rng();
            std::vector<const uint32_t*> fs = {words[0].data(), nullptr, words[2].data()};
            std::vector<uint64_t> counts(m * U, 0xDEADBEEFDEADBEEFull);
            facet_counts_host(codes.data(), tags ? lims.data() : nullptr, n, U, fs.data(), removed.data(), m, counts.data());
            for (size_t j = 0; j < m; ++j) {
                std::map<int32_t, uint64_t> want;
                for (size_t i = 0; i < n; ++i) {
                    const bool allowed = !fs[j] || ((fs[j][i / 32] >> (i % 32)) & 1u);
                    const bool gone = (removed[i / 32] >> (i % 32)) & 1u;
                    if (!allowed || gone) continue;
                    for (uint32_t e = tags ? lims[i] : (uint32_t)i; e < (tags ? lims[i + 1] : (uint32_t)i + 1); ++e) ++want[col[e]];
                }
                uint64_t nonzero = 0;
                for (size_t u = 0; u < U; ++u) {
                    const auto it = want.find(values[u]);
                    REQUIRE(counts[j * U + u] == (it == want.end() ? 0 : it->second));
                    nonzero += counts[j * U + u] != 0;
                }
                for (size_t K : {1, 3, 1024}) {
                    std::vector<int32_t> tv(K, 0x5A5A5A5A);
                    std::vector<uint64_t> tc(K, 0xDEADBEEFDEADBEEFull);
                    uint32_t found = 0xDEADBEEFu;
                    facet_top_host(counts.data() + j * U, values.data(), U, K, tv.data(), tc.data(), &found);
                    REQUIRE(found == std::min<uint64_t>(K, nonzero));
                    for (size_t i = 0; i < K; ++i) {
                        if (i >= found) { REQUIRE(tv[i] == 0 && tc[i] == 0); continue; }
                        REQUIRE(tc[i] != 0 && want[tv[i]] == tc[i]);
                        if (i) REQUIRE(tc[i - 1] > tc[i] || (tc[i - 1] == tc[i] && tv[i - 1] < tv[i]));
                    }
                }
            }
        }
    }
    std::printf("self: ok\n");
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "eval" && argc == 4) return run_eval(argv[2], argv[3]);
    if (mode == "refuse") return run_refuse();
    if (mode == "self") return run_self();
    std::fprintf(stderr, "usage: facet_host eval <in> <out> | refuse | self\n");
    return 2;
}
