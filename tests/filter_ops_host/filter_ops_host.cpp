// filter_ops_host.cpp -- the host statement of the filter algebra under sanitizers (tests/test_filter_ops_host.py builds
// this file with g++ -fsanitize=address,undefined; no HIP, no GPU).
//
//   filter_ops_host eval <in> <out>   runs filter_combine_host on the caller's data, on exact-size heap buffers (a read or
//                                     write one word too far is an ASAN report), the outputs pre-filled with garbage:
//                                     <in>  = u64 op, u64 n_bits, u64 m, u64 b_broadcast, u32 a[m][nw],
//                                             u32 b[m or 1][nw] (absent for NOT), nw = (n_bits + 31) / 32
//                                     <out> = u32 words[m][nw], u64 counts[m]
//                                     The test compares <out> with numpy.
//   filter_ops_host self              the same function against a bit-by-bit loop: every size, m, op and both forms of b,
//                                     inputs with dirty bits behind n_bits
//
// Exit code 0 = all good.
#include <cstdio>
#include <cstdlib>
#include <fstream>
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
    const std::vector<uint64_t> hdr = read_vec<uint64_t>(f, 4);
    const int op = (int)hdr[0];
    const size_t n_bits = hdr[1], m = hdr[2], nw = (n_bits + 31) / 32;
    const bool bc = hdr[3] != 0;
    REQUIRE(op >= 0 && op < kFilterOps);
    const std::vector<uint32_t> a = read_vec<uint32_t>(f, m * nw);
    const std::vector<uint32_t> b = op == kFilterNot ? std::vector<uint32_t>() : read_vec<uint32_t>(f, (bc ? 1 : m) * nw);
    std::vector<uint32_t> words(m * nw, 0xDEADBEEFu);
    std::vector<uint64_t> counts(m, 0xDEADBEEFull);
    filter_combine_host(op, a.data(), op == kFilterNot ? nullptr : b.data(), bc, n_bits, m, words.data(), counts.data());
    std::ofstream o(out, std::ios::binary | std::ios::trunc);
    write_vec(o, words);
    write_vec(o, counts);
    REQUIRE(o.good());
    std::printf("eval: ok\n");
    return 0;
}

static uint32_t bit_of(const std::vector<uint32_t>& w, size_t base, size_t i) { return (w[base + i / 32] >> (i % 32)) & 1u; }

static int run_self() {
    std::mt19937_64 rng(108);
    int cases = 0;
    for (size_t n_bits : {(size_t)0, (size_t)1, (size_t)31, (size_t)32, (size_t)33, (size_t)127, (size_t)128, (size_t)129, (size_t)2047,
                          (size_t)2049, (size_t)4100}) {
        const size_t nw = (n_bits + 31) / 32;
        for (size_t m : {(size_t)1, (size_t)3, (size_t)70}) {
            // random words, dirty behind n_bits; filter 1 all ones and filter 2 all zeros where there are that many
            std::vector<uint32_t> a(m * nw), b(m * nw);
            for (auto& x : a) x = (uint32_t)rng();
            for (auto& x : b) x = (uint32_t)rng();
            if (m > 2)
                for (size_t w = 0; w < nw; ++w) { a[nw + w] = 0xFFFFFFFFu; a[2 * nw + w] = 0u; b[2 * nw + w] = 0xFFFFFFFFu; }
            for (int op = 0; op < kFilterOps; ++op)
                for (int bc = 0; bc < 2; ++bc) {
                    if (op == kFilterNot && bc) continue;
                    const std::vector<uint32_t> bb(b.begin(), b.begin() + (long)((bc ? 1 : m) * nw));     // exact size
                    std::vector<uint32_t> words(m * nw, 0xDEADBEEFu);
                    std::vector<uint64_t> counts(m, 0xDEADBEEFull);
                    filter_combine_host(op, a.data(), op == kFilterNot ? nullptr : bb.data(), bc != 0, n_bits, m, words.data(),
                                        counts.data());
                    for (size_t j = 0; j < m; ++j) {
                        uint64_t want = 0;
                        for (size_t i = 0; i < n_bits; ++i) {
                            const uint32_t x = bit_of(a, j * nw, i), y = op == kFilterNot ? 0u : bit_of(bb, bc ? 0 : j * nw, i);
                            uint32_t bit = 0;
                            switch (op) {
                                case kFilterAnd: bit = x & y; break;
                                case kFilterOr: bit = x | y; break;
                                case kFilterAndNot: bit = x & (y ^ 1u); break;
                                case kFilterXor: bit = x ^ y; break;
                                default: bit = x ^ 1u; break;
                            }
                            REQUIRE(bit_of(words, j * nw, i) == bit);
                            want += bit;
                        }
                        REQUIRE(counts[j] == want);
                        if (n_bits % 32) REQUIRE((words[j * nw + nw - 1] >> (n_bits % 32)) == 0u);     // dirty tails do not leak
                        ++cases;
                    }
                }
        }
    }
    std::printf("self: ok (%d filters)\n", cases);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "eval" && argc == 4) return run_eval(argv[2], argv[3]);
    if (mode == "self") return run_self();
    std::fprintf(stderr, "usage: filter_ops_host eval <in> <out> | self\n");
    return 2;
}
