// Stand-alone driver of csrc/host_maxsim_rescore.h for the CPU tests (tests/test_maxsim_rescore_host.py): built with plain
// g++ and -fsanitize=address,undefined -ffp-contract=off, run as a child process.  It reads the cases the Python test wrote
// -- candidates, token rows, vectors, norms, keys, optional bitmaps and row map, and the outputs
// tests/maxsim_rescore_model.py expects -- runs maxsim_rescore_host on heap buffers of exactly the stated sizes and compares
// every output byte; then key columns with their expected inverted form, through key_rows_host.
//
// File: u64 n_cases, then per case u64 {n, R, T, dim, n_ids, D, k, has_allow, has_rows} and the arrays
//   cand_keys i32[n*R], cand_lb f32[n*R], cand_found i32[n], tokens f32[n*T*dim], n_tokens i32[n], raw f32[n_ids*D],
//   norm_sq f32[n_ids], key_of i32[n_ids], allow u32[n*ceil(n_ids/32)] (if has_allow), rows u32[n_ids] (if has_rows),
//   keys i32[n*k], score f32[n*k], hits i32[n*k], rows i64[n*k*T], found i32[n], certified i32[n]   (expected);
// then u64 n_columns, per column u64 {n, n_keys} and keys i32[n], ids u32[n], distinct i32[n_keys], offsets u32[n_keys+1].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../rabitq-ann-search_amd/csrc/host_maxsim_rescore.h"

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
        std::fprintf(stderr, "usage: maxsim_rescore_host <cases file>\n");
        return 2;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    const uint64_t n_cases = read_array<uint64_t>(f, 1)[0];
    for (uint64_t c = 0; c < n_cases; ++c) {
        const auto hd = read_array<uint64_t>(f, 9);
        const uint64_t n = hd[0], R = hd[1], T = hd[2], dim = hd[3], n_ids = hd[4], D = hd[5], k = hd[6], has_allow = hd[7], has_rows = hd[8];
        const uint64_t nw = (n_ids + 31) / 32;
        const auto ck = read_array<int32_t>(f, n * R);
        const auto lb = read_array<float>(f, n * R);
        const auto cf = read_array<int32_t>(f, n);
        const auto tok = read_array<float>(f, n * T * dim);
        const auto nt = read_array<int32_t>(f, n);
        const auto raw = read_array<float>(f, n_ids * D);
        const auto norm = read_array<float>(f, n_ids);
        const auto key_of = read_array<int32_t>(f, n_ids);
        const auto allow = read_array<uint32_t>(f, has_allow ? n * nw : 0);
        const auto rows = read_array<uint32_t>(f, has_rows ? n_ids : 0);
        const auto want_keys = read_array<int32_t>(f, n * k);
        const auto want_score = read_array<float>(f, n * k);
        const auto want_hits = read_array<int32_t>(f, n * k);
        const auto want_rows = read_array<int64_t>(f, n * k * T);
        const auto want_found = read_array<int32_t>(f, n);
        const auto want_cert = read_array<int32_t>(f, n);
        auto o_keys = poisoned<int32_t>(n * k), o_hits = poisoned<int32_t>(n * k), o_found = poisoned<int32_t>(n), o_cert = poisoned<int32_t>(n);
        auto o_score = poisoned<float>(n * k);
        auto o_rows = poisoned<int64_t>(n * k * T);
        cph::maxsim_rescore_host(ck.get(), lb.get(), cf.get(), n, (uint32_t)R, tok.get(), (uint32_t)T, (uint32_t)dim, nt.get(), raw.get(),
                                 norm.get(), n_ids, (uint32_t)D, key_of.get(), has_allow ? allow.get() : nullptr,
                                 has_rows ? rows.get() : nullptr, (uint32_t)k, o_keys.get(), o_score.get(), o_hits.get(), o_rows.get(),
                                 o_found.get(), o_cert.get());
        if (!same(o_keys, want_keys, n * k) || !same(o_score, want_score, n * k) || !same(o_hits, want_hits, n * k) ||
            !same(o_rows, want_rows, n * k * T) || !same(o_found, want_found, n) || !same(o_cert, want_cert, n)) {
            std::printf("maxsim rescore: case %llu differs (n=%llu R=%llu T=%llu D=%llu k=%llu allow=%llu rows=%llu)\n", (unsigned long long)c,
                        (unsigned long long)n, (unsigned long long)R, (unsigned long long)T, (unsigned long long)D, (unsigned long long)k,
                        (unsigned long long)has_allow, (unsigned long long)has_rows);
            return 1;
        }
    }
    const uint64_t n_cols = read_array<uint64_t>(f, 1)[0];
    for (uint64_t c = 0; c < n_cols; ++c) {
        const auto hd = read_array<uint64_t>(f, 2);
        const uint64_t n = hd[0], nk = hd[1];
        const auto keys = read_array<int32_t>(f, n);
        const auto want_ids = read_array<uint32_t>(f, n);
        const auto want_keys = read_array<int32_t>(f, nk);
        const auto want_offs = read_array<uint32_t>(f, nk + 1);
        auto ids = poisoned<uint32_t>(n), offs = poisoned<uint32_t>(n + 1);
        auto ukeys = poisoned<int32_t>(n);
        const uint64_t got = cph::key_rows_host(keys.get(), n, ids.get(), ukeys.get(), offs.get());
        if (got != nk || !same(ids, want_ids, n) || !same(ukeys, want_keys, nk) || !same(offs, want_offs, nk + 1)) {
            std::printf("maxsim rescore: key column %llu differs (n=%llu)\n", (unsigned long long)c, (unsigned long long)n);
            return 1;
        }
    }
    std::fclose(f);
    std::printf("maxsim rescore: ok (%llu cases, %llu key columns)\n", (unsigned long long)n_cases, (unsigned long long)n_cols);
    return 0;
}
