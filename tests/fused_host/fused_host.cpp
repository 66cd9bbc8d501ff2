// Stand-alone driver of csrc/host_fused.h for the CPU tests (tests/test_fused_host.py): built with plain g++ and
// -fsanitize=address,undefined -ffp-contract=off, run as a child process.  It reads the cases the Python test wrote --
// candidate rows, live counts, weights, padded query vectors, stored vectors, norms, an optional row map, and the outputs
// tests/fused_model.py expects -- runs fused_rows_host on heap buffers of exactly the stated sizes and compares every output
// byte.
//
// File: u64 n_cases, then per case u64 {n, T, C, n_ids, D, k, has_rows} and the arrays
//   cand i64[n*T*C], n_vectors i32[n], weights f32[n*T], qpad f32[n*T*D], raw f32[n_ids*D], norm_sq f32[n_ids],
//   rows u32[n_ids] (if has_rows), ids i64[n*k], score f32[n*k], hits i32[n*k]   (expected).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../rabitq-ann-search_amd/csrc/host_fused.h"

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
        std::fprintf(stderr, "usage: fused_host <cases file>\n");
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
        const uint64_t n = hd[0], T = hd[1], C = hd[2], n_ids = hd[3], D = hd[4], k = hd[5], has_rows = hd[6];
        const auto cand = read_array<int64_t>(f, n * T * C);
        const auto nv = read_array<int32_t>(f, n);
        const auto w = read_array<float>(f, n * T);
        const auto qpad = read_array<float>(f, n * T * D);
        const auto raw = read_array<float>(f, n_ids * D);
        const auto norm = read_array<float>(f, n_ids);
        const auto rows = read_array<uint32_t>(f, has_rows ? n_ids : 0);
        const auto want_ids = read_array<int64_t>(f, n * k);
        const auto want_score = read_array<float>(f, n * k);
        const auto want_hits = read_array<int32_t>(f, n * k);
        auto o_ids = poisoned<int64_t>(n * k);
        auto o_score = poisoned<float>(n * k);
        auto o_hits = poisoned<int32_t>(n * k);
        cph::fused_rows_host(cand.get(), n, (uint32_t)T, nv.get(), w.get(), (uint32_t)C, qpad.get(), raw.get(), norm.get(), n_ids,
                             (uint32_t)D, has_rows ? rows.get() : nullptr, (uint32_t)k, o_ids.get(), o_score.get(), o_hits.get());
        if (!same(o_ids, want_ids, n * k) || !same(o_score, want_score, n * k) || !same(o_hits, want_hits, n * k)) {
            std::printf("fused: case %llu differs (n=%llu T=%llu C=%llu D=%llu k=%llu rows=%llu)\n", (unsigned long long)c,
                        (unsigned long long)n, (unsigned long long)T, (unsigned long long)C, (unsigned long long)D, (unsigned long long)k,
                        (unsigned long long)has_rows);
            return 1;
        }
    }
    std::fclose(f);
    std::printf("fused: ok (%llu cases)\n", (unsigned long long)n_cases);
    return 0;
}
