// labels_host.cpp -- the host statements of the label column under sanitizers (tests/test_labels_host.py builds this
// file with g++ -fsanitize=address,undefined; no HIP, no GPU).
//
//   labels_host eval <in> <out>   runs label_filters_host and labels_to_internal_host on the caller's data, on
//                                 exact-size heap buffers (a read or write one element too far is an ASAN report):
//                                 <in>  = u64 n, u64 m, i32 labels[n], i32 lo[m], i32 hi[m], u32 rows[n]
//                                 <out> = u32 words[m][(n + 31) / 32], u64 counts[m], i32 internal[n]
//                                 The test compares <out> with numpy.
//   labels_host self              the same two functions against a bit-by-bit loop, every output buffer pre-filled with
//                                 garbage (every word must be written, the bits behind n clear)
//
// Exit code 0 = all good.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <numeric>
#include <random>
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

static int run_eval(const std::string& in, const std::string& out) {
    std::ifstream f(in, std::ios::binary);
    REQUIRE(f.good());
    const std::vector<uint64_t> hdr = read_vec<uint64_t>(f, 2);
    const size_t n = hdr[0], m = hdr[1], nw = (n + 31) / 32;
    const std::vector<int32_t> labels = read_vec<int32_t>(f, n), lo = read_vec<int32_t>(f, m), hi = read_vec<int32_t>(f, m);
    const std::vector<uint32_t> rows = read_vec<uint32_t>(f, n);
    std::vector<uint32_t> words(m * nw, 0xDEADBEEFu);
    std::vector<uint64_t> counts(m, 0xDEADBEEFull);
    std::vector<int32_t> internal(n, 0x5EADBEEF);
    label_filters_host(labels.data(), n, lo.data(), hi.data(), m, words.data(), counts.data());
    REQUIRE(is_row_permutation(rows.data(), n));
    labels_to_internal_host(labels.data(), rows.data(), n, internal.data());
    std::ofstream o(out, std::ios::binary | std::ios::trunc);
    write_vec(o, words);
    write_vec(o, counts);
    write_vec(o, internal);
    REQUIRE(o.good());
    std::printf("eval: ok\n");
    return 0;
}

static int run_self() {
    std::mt19937_64 rng(105);
    const int32_t special[] = {INT32_MIN, -1, 0, 1, 5, INT32_MAX};
    int cases = 0;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)31, (size_t)32, (size_t)33, (size_t)63, (size_t)64, (size_t)65, (size_t)2047,
                     (size_t)2048, (size_t)2049, (size_t)4100}) {
        const size_t nw = (n + 31) / 32;
        std::vector<int32_t> labels(n);
        for (auto& x : labels) x = rng() % 3 ? special[rng() % 6] : (int32_t)(uint32_t)rng();
        for (size_t m : {(size_t)1, (size_t)3, (size_t)70}) {
            std::vector<int32_t> lo(m), hi(m);
            for (size_t j = 0; j < m; ++j) {
                switch (j % 7) {
                    case 0: lo[j] = hi[j] = special[(j / 7) % 6]; break;                   // equality
                    case 1: lo[j] = -1; hi[j] = 5; break;                                   // a range
                    case 2: lo[j] = 5; hi[j] = -1; break;                                   // lo > hi: empty
                    case 3: lo[j] = INT32_MIN; hi[j] = INT32_MAX; break;                    // everything
                    case 4: lo[j] = hi[j] = 123456789; break;                               // (almost surely) nobody's
                    case 5: lo[j] = 0; hi[j] = INT32_MAX; break;                            // overlaps case 1
                    default: lo[j] = (int32_t)(uint32_t)rng(); hi[j] = (int32_t)(uint32_t)rng(); break;
                }
            }
            std::vector<uint32_t> words(m * nw, 0xDEADBEEFu);
            std::vector<uint64_t> counts(m, 0xDEADBEEFull);
            label_filters_host(labels.data(), n, lo.data(), hi.data(), m, words.data(), counts.data());
            for (size_t j = 0; j < m; ++j) {
                uint64_t want = 0;
                for (size_t i = 0; i < n; ++i) {
                    const uint32_t bit = (int64_t)labels[i] >= (int64_t)lo[j] && (int64_t)labels[i] <= (int64_t)hi[j];
                    REQUIRE(((words[j * nw + i / 32] >> (i % 32)) & 1u) == bit);
                    want += bit;
                }
                REQUIRE(counts[j] == want);
                if (n % 32) REQUIRE((words[j * nw + nw - 1] >> (n % 32)) == 0u);
                if (j % 7 == 2) REQUIRE(want == 0);
                if (j % 7 == 3) REQUIRE(want == n);
                ++cases;
            }
        }
        // input rows -> internal order
        std::vector<uint32_t> rows(n);
        std::iota(rows.begin(), rows.end(), 0u);
        std::shuffle(rows.begin(), rows.end(), rng);
        std::vector<int32_t> internal(n, 0x5EADBEEF);
        labels_to_internal_host(labels.data(), rows.data(), n, internal.data());
        for (size_t i = 0; i < n; ++i) REQUIRE(internal[i] == labels[rows[i]]);
    }
    std::printf("self: ok (%d filters)\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "eval" && argc == 4) return run_eval(argv[2], argv[3]);
    if (mode == "self") return run_self();
    std::fprintf(stderr, "usage: labels_host eval <in> <out> | self\n");
    return 2;
}
