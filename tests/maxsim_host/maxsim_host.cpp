// Stand-alone driver of csrc/host_maxsim.h for the CPU tests (tests/test_maxsim_host.py): built with plain g++ and
// -fsanitize=address,undefined, run as a child process.  It reads the cases the Python test wrote -- candidate rows, token
// counts, keys, an optional row map and the outputs tests/maxsim_model.py expects -- runs maxsim_rows_host on heap buffers
// of exactly the stated sizes and compares every output byte.
//
// File: u64 n_cases, then per case u64 {n, T, C, k, n_keys, has_rows, has_tokens} and the arrays
//   ids i64[n*T*C], dist f32[n*T*C], n_tokens i32[n] (if has_tokens), key_of i32[n_keys], rows u32[n_keys] (if has_rows),
//   keys i32[n*k], score f32[n*k], hits i32[n*k], rows i64[n*k*T], found i32[n]   (expected)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../rabitq-ann-search_amd/csrc/host_maxsim.h"

namespace {

template <class T>
std::unique_ptr<T[]> read_array(FILE* f, uint64_t count) {
    std::unique_ptr<T[]> a(new T[count]);               // exactly `count` elements: an overrun is the sanitizer's to find
    if (count && std::fread(a.get(), sizeof(T), count, f) != count) {
        std::fprintf(stderr, "short read\n");
        std::exit(2);
    }
    return a;
}

template <class T>
std::unique_ptr<T[]> poisoned(uint64_t count) {
    std::unique_ptr<T[]> a(new T[count]);
    std::memset(a.get(), 0xA5, count * sizeof(T));      // (nothing depends on what the outputs held)
    return a;
}

template <class T>
bool same(const std::unique_ptr<T[]>& a, const std::unique_ptr<T[]>& b, uint64_t count) {
    return std::memcmp(a.get(), b.get(), count * sizeof(T)) == 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: maxsim_host <cases file>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    const uint64_t n_cases = read_array<uint64_t>(f, 1)[0];
    for (uint64_t c = 0; c < n_cases; ++c) {
        const auto hd = read_array<uint64_t>(f, 7);
        const uint64_t n = hd[0], T = hd[1], C = hd[2], k = hd[3], n_keys = hd[4], has_rows = hd[5], has_tokens = hd[6];
        const auto ids = read_array<int64_t>(f, n * T * C);
        const auto dist = read_array<float>(f, n * T * C);
        const auto n_tokens = read_array<int32_t>(f, has_tokens ? n : 0);
        const auto key_of = read_array<int32_t>(f, n_keys);
        const auto rows = read_array<uint32_t>(f, has_rows ? n_keys : 0);
        const auto want_keys = read_array<int32_t>(f, n * k);
        const auto want_score = read_array<float>(f, n * k);
        const auto want_hits = read_array<int32_t>(f, n * k);
        const auto want_rows = read_array<int64_t>(f, n * k * T);
        const auto want_found = read_array<int32_t>(f, n);
        auto o_keys = poisoned<int32_t>(n * k), o_hits = poisoned<int32_t>(n * k), o_found = poisoned<int32_t>(n);
        auto o_score = poisoned<float>(n * k);
        auto o_rows = poisoned<int64_t>(n * k * T);
        cph::maxsim_rows_host(ids.get(), dist.get(), n, (uint32_t)T, has_tokens ? n_tokens.get() : nullptr, (uint32_t)C, key_of.get(), n_keys,
                              has_rows ? rows.get() : nullptr, (uint32_t)k, o_keys.get(), o_score.get(), o_hits.get(), o_rows.get(),
                              o_found.get());
        if (!same(o_keys, want_keys, n * k) || !same(o_score, want_score, n * k) || !same(o_hits, want_hits, n * k) ||
            !same(o_rows, want_rows, n * k * T) || !same(o_found, want_found, n)) {
            std::printf("maxsim: case %llu differs (n=%llu T=%llu C=%llu k=%llu rows=%llu tokens=%llu)\n", (unsigned long long)c,
                        (unsigned long long)n, (unsigned long long)T, (unsigned long long)C, (unsigned long long)k,
                        (unsigned long long)has_rows, (unsigned long long)has_tokens);
            return 1;
        }
    }
    std::fclose(f);
    std::printf("maxsim: ok (%llu cases)\n", (unsigned long long)n_cases);
    return 0;
}
