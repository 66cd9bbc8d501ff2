// Stand-alone driver of csrc/host_group.h for the CPU tests (tests/test_group_host.py): built with plain g++ and
// -fsanitize=address,undefined, run as a child process.  It reads the cases the Python test wrote -- candidate rows, keys,
// an optional row map and the outputs tests/group_model.py expects -- runs group_rows_host on heap buffers of exactly the
// stated sizes and compares every output byte.
//
// File: u64 n_cases, then per case u64 {n, C, k, g, n_keys, has_rows} and the arrays
//   ids i64[n*C], dist f32[n*C], key_of i32[n_keys], rows u32[n_keys] (if has_rows),
//   ids i64[n*k*g], dist f32[n*k*g], keys i32[n*k], counts i32[n*k], complete u8[n]   (expected)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../rabitq-ann-search_amd/csrc/host_group.h"

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
        std::fprintf(stderr, "usage: group_host <cases file>\n");
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
        const uint64_t n = hd[0], C = hd[1], k = hd[2], g = hd[3], n_keys = hd[4], has_rows = hd[5];
        const auto ids = read_array<int64_t>(f, n * C);
        const auto dist = read_array<float>(f, n * C);
        const auto key_of = read_array<int32_t>(f, n_keys);
        const auto rows = read_array<uint32_t>(f, has_rows ? n_keys : 0);
        const auto want_ids = read_array<int64_t>(f, n * k * g);
        const auto want_dist = read_array<float>(f, n * k * g);
        const auto want_keys = read_array<int32_t>(f, n * k);
        const auto want_counts = read_array<int32_t>(f, n * k);
        const auto want_complete = read_array<uint8_t>(f, n);
        std::unique_ptr<int64_t[]> o_ids(new int64_t[n * k * g]);
        std::unique_ptr<float[]> o_dist(new float[n * k * g]);
        std::unique_ptr<int32_t[]> o_keys(new int32_t[n * k]), o_counts(new int32_t[n * k]);
        std::unique_ptr<uint8_t[]> o_complete(new uint8_t[n]);
        std::memset(o_ids.get(), 0xA5, n * k * g * 8);   // (nothing depends on what the outputs held)
        std::memset(o_dist.get(), 0xA5, n * k * g * 4);
        std::memset(o_keys.get(), 0xA5, n * k * 4);
        std::memset(o_counts.get(), 0xA5, n * k * 4);
        std::memset(o_complete.get(), 0xA5, n);
        cph::group_rows_host(ids.get(), dist.get(), n, (uint32_t)C, key_of.get(), has_rows ? rows.get() : nullptr, (uint32_t)k,
                             (uint32_t)g, o_ids.get(), o_dist.get(), o_keys.get(), o_counts.get(), o_complete.get());
        if (!same(o_ids, want_ids, n * k * g) || !same(o_dist, want_dist, n * k * g) || !same(o_keys, want_keys, n * k) ||
            !same(o_counts, want_counts, n * k) || !same(o_complete, want_complete, n)) {
            std::printf("group: case %llu differs (n=%llu C=%llu k=%llu g=%llu rows=%llu)\n", (unsigned long long)c, (unsigned long long)n,
                        (unsigned long long)C, (unsigned long long)k, (unsigned long long)g, (unsigned long long)has_rows);
            return 1;
        }
    }
    std::fclose(f);
    std::printf("group: ok (%llu cases)\n", (unsigned long long)n_cases);
    return 0;
}
