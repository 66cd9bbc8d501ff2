// Stand-alone driver of csrc/host_knn.h for the CPU tests (tests/test_knn_host.py): built with plain g++ and
// -fsanitize=address,undefined -ffp-contract=off, run as a child process.  It reads the cases the Python test wrote -- rows,
// optional queries, optional q_ids, and the ids, distances and fallback count the library's cph_host_knn gave for them -- runs
// knn_host on heap buffers of exactly the stated sizes and compares every output byte.
//
// File: u64 n_cases, then per case u64 {n, dim, nq, has_q_ids, path, fallback_rows} and the arrays
//   vectors f32[n*dim], queries f32[nq*dim], q_ids u32[nq] (if has_q_ids), ids u32[rows*32], dist f32[rows*32]   (expected;
//   rows = nq, or n where nq = 0: the self-join).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../rabitq-ann-search_amd/csrc/host_knn.h"

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

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: knn_host <cases file>\n");
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
        const uint64_t n = hd[0], dim = hd[1], nq = hd[2], has_q_ids = hd[3], path = hd[4], want_redo = hd[5];
        const uint64_t rows = nq ? nq : n;
        const auto x = read_array<float>(f, n * dim);
        const auto q = read_array<float>(f, nq * dim);
        const auto q_ids = read_array<uint32_t>(f, has_q_ids ? nq : 0);
        const auto want_ids = read_array<uint32_t>(f, rows * 32);
        const auto want_dist = read_array<float>(f, rows * 32);
        auto ids = poisoned<uint32_t>(rows * 32);
        auto dist = poisoned<float>(rows * 32);
        auto cand = poisoned<uint32_t>(path == 1 ? n : 0);
        cph::knn_debug_check(x.get(), n, dim, nq ? q.get() : nullptr, nq, has_q_ids ? q_ids.get() : nullptr, has_q_ids ? 1 : 0, (int)path,
                             ids.get(), dist.get());
        const uint32_t redo = cph::knn_host(x.get(), n, dim, nq ? q.get() : nullptr, nq, has_q_ids ? q_ids.get() : nullptr, (int)path,
                                            ids.get(), dist.get(), path == 1 ? cand.get() : nullptr);
        if (std::memcmp(ids.get(), want_ids.get(), rows * 128) != 0 || std::memcmp(dist.get(), want_dist.get(), rows * 128) != 0 ||
            redo != want_redo) {
            std::printf("knn: case %llu differs (n=%llu dim=%llu nq=%llu q_ids=%llu path=%llu)\n", (unsigned long long)c, (unsigned long long)n,
                        (unsigned long long)dim, (unsigned long long)nq, (unsigned long long)has_q_ids, (unsigned long long)path);
            return 1;
        }
    }
    std::fclose(f);
    std::printf("knn: ok (%llu cases)\n", (unsigned long long)n_cases);
    return 0;
}
