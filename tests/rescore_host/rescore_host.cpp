// Stand-alone driver of csrc/host_rescore.h for the CPU tests (tests/test_rescore_host.py): built with plain g++,
// -fsanitize=address,undefined and -ffp-contract=off, run as a child process.  It reads the cases the Python test wrote,
// runs rescore_rows_in_host / rescore_rows_host on heap buffers of exactly the stated sizes and compares every output byte
// with what tests/rescore_model.py expects.
//
// File: u64 n_cases, then per case a u64 kind and
//   kind 0 (rows in): u64 {n, dim, f32, has_map, n_map}; rows f32[n*dim], map u32[n_map] (if has_map);
//                     expected: stored u8[n*stride], norms f32[n], u64 {bad, first_bad}
//   kind 1 (rescore): u64 {n, C, k, n_ids, dim, f32, ip}; ids i64[n*C], dist f32[n*C], fq f32[n*dim],
//                     stored u8[n_ids*stride], norms f32[n_ids], rows u32[n_ids];
//                     expected without the row map, then with it: ids i64[n*k], score f32[n*k], first f32[n*k]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../rabitq-ann-search_amd/csrc/host_rescore.h"

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

bool rows_in_case(FILE* f) {
    const auto hd = read_array<uint64_t>(f, 5);
    const uint64_t n = hd[0], dim = hd[1], f32 = hd[2], has_map = hd[3], n_map = hd[4];
    const cph::RescoreLayout L = cph::rescore_layout((uint32_t)dim, f32 != 0);
    const auto rows = read_array<float>(f, n * dim);
    const auto map = read_array<uint32_t>(f, has_map ? n_map : 0);
    const auto want_stored = read_array<uint8_t>(f, n * L.stride);
    const auto want_norms = read_array<float>(f, n);
    const auto want_bad = read_array<uint64_t>(f, 2);
    std::unique_ptr<uint8_t[]> stored(new uint8_t[n * L.stride]);
    std::unique_ptr<float[]> norms(new float[n]);
    std::memset(stored.get(), 0xA5, n * L.stride);
    std::memset(norms.get(), 0xA5, n * 4);
    std::vector<uint32_t> inv;
    if (has_map) inv = cph::rescore_inverse_rows(map.get(), n_map, n);
    unsigned long long first_bad = 0;
    const uint64_t bad = cph::rescore_rows_in_host(rows.get(), n, (uint32_t)dim, f32 != 0, has_map ? inv.data() : nullptr, stored.get(),
                                                   norms.get(), &first_bad);
    return same(stored, want_stored, n * L.stride) && same(norms, want_norms, n) && bad == want_bad[0] && first_bad == want_bad[1];
}

bool rescore_case(FILE* f) {
    const auto hd = read_array<uint64_t>(f, 7);
    const uint64_t n = hd[0], C = hd[1], k = hd[2], n_ids = hd[3], dim = hd[4], f32 = hd[5], ip = hd[6];
    const cph::RescoreLayout L = cph::rescore_layout((uint32_t)dim, f32 != 0);
    const auto ids = read_array<int64_t>(f, n * C);
    const auto dist = read_array<float>(f, n * C);
    const auto fq = read_array<float>(f, n * dim);
    const auto stored = read_array<uint8_t>(f, n_ids * L.stride);
    const auto norms = read_array<float>(f, n_ids);
    const auto rows = read_array<uint32_t>(f, n_ids);
    bool ok = true;
    for (int with_rows = 0; with_rows < 2; ++with_rows) {
        const auto want_ids = read_array<int64_t>(f, n * k);
        const auto want_score = read_array<float>(f, n * k);
        const auto want_first = read_array<float>(f, n * k);
        std::unique_ptr<int64_t[]> o_ids(new int64_t[n * k]);
        std::unique_ptr<float[]> o_score(new float[n * k]), o_first(new float[n * k]);
        std::memset(o_ids.get(), 0xA5, n * k * 8);      // (nothing depends on what the outputs held)
        std::memset(o_score.get(), 0xA5, n * k * 4);
        std::memset(o_first.get(), 0xA5, n * k * 4);
        cph::rescore_rows_host(ids.get(), dist.get(), n, (uint32_t)C, fq.get(), (uint32_t)dim, stored.get(), norms.get(), n_ids, f32 != 0,
                               ip != 0, with_rows ? rows.get() : nullptr, (uint32_t)k, o_ids.get(), o_score.get(), o_first.get());
        ok = ok && same(o_ids, want_ids, n * k) && same(o_score, want_score, n * k) && same(o_first, want_first, n * k);
    }
    return ok;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: rescore_host <cases file>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    const uint64_t n_cases = read_array<uint64_t>(f, 1)[0];
    for (uint64_t c = 0; c < n_cases; ++c) {
        const uint64_t kind = read_array<uint64_t>(f, 1)[0];
        if (!(kind == 0 ? rows_in_case(f) : rescore_case(f))) {
            std::printf("rescore: case %llu (kind %llu) differs\n", (unsigned long long)c, (unsigned long long)kind);
            return 1;
        }
    }
    std::fclose(f);
    std::printf("rescore: ok (%llu cases)\n", (unsigned long long)n_cases);
    return 0;
}
