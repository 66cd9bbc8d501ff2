// Stand-alone driver of csrc/host_diverse.h for the CPU tests (tests/test_diverse_host.py): built with plain g++,
// -fsanitize=address,undefined and -ffp-contract=off, run as a child process.  It reads the cases the Python test wrote --
// candidate rows, vectors, norms, an optional row map and the outputs tests/diverse_model.py expects -- runs
// diverse_rows_host on heap buffers of exactly the stated sizes and compares every output byte.
//
// File: u64 n_cases, then per case u64 {n, C, k, n_ids, D, has_rows}, f32 lam and the arrays
//   ids i64[n*C], dist f32[n*C], raw f32[n_ids*D], norm_sq f32[n_ids], rows u32[n_ids] (if has_rows),
//   ids i64[n*k], dist f32[n*k], gap f32[n*k]   (expected)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../rabitq-ann-search_amd/csrc/host_diverse.h"

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
bool same(const std::unique_ptr<T[]>& a, const std::unique_ptr<T[]>& b, uint64_t count) {
    return std::memcmp(a.get(), b.get(), count * sizeof(T)) == 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: diverse_host <cases file>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    const uint64_t n_cases = read_array<uint64_t>(f, 1)[0];
    for (uint64_t c = 0; c < n_cases; ++c) {
        const auto hd = read_array<uint64_t>(f, 6);
        const uint64_t n = hd[0], C = hd[1], k = hd[2], n_ids = hd[3], D = hd[4], has_rows = hd[5];
        const float lam = read_array<float>(f, 1)[0];
        const auto ids = read_array<int64_t>(f, n * C);
        const auto dist = read_array<float>(f, n * C);
        const auto raw = read_array<float>(f, n_ids * D);
        const auto norm = read_array<float>(f, n_ids);
        const auto rows = read_array<uint32_t>(f, has_rows ? n_ids : 0);
        const auto want_ids = read_array<int64_t>(f, n * k);
        const auto want_dist = read_array<float>(f, n * k);
        const auto want_gap = read_array<float>(f, n * k);
        std::unique_ptr<int64_t[]> o_ids(new int64_t[n * k]);
        std::unique_ptr<float[]> o_dist(new float[n * k]), o_gap(new float[n * k]);
        std::memset(o_ids.get(), 0xA5, n * k * 8);      // (nothing depends on what the outputs held)
        std::memset(o_dist.get(), 0xA5, n * k * 4);
        std::memset(o_gap.get(), 0xA5, n * k * 4);
        cph::diverse_rows_host(ids.get(), dist.get(), n, (uint32_t)C, raw.get(), norm.get(), n_ids, (uint32_t)D,
                               has_rows ? rows.get() : nullptr, (uint32_t)k, lam, o_ids.get(), o_dist.get(), o_gap.get());
        if (!same(o_ids, want_ids, n * k) || !same(o_dist, want_dist, n * k) || !same(o_gap, want_gap, n * k)) {
            std::printf("diverse: case %llu differs (n=%llu C=%llu k=%llu D=%llu lam=%g rows=%llu)\n", (unsigned long long)c,
                        (unsigned long long)n, (unsigned long long)C, (unsigned long long)k, (unsigned long long)D, (double)lam,
                        (unsigned long long)has_rows);
            return 1;
        }
    }
    std::fclose(f);
    std::printf("diverse: ok (%llu cases)\n", (unsigned long long)n_cases);
    return 0;
}
