// add_host.cpp -- the host code of added rows under sanitizers (tests/test_add_host.py builds this file with
// g++ -fsanitize=address,undefined; no HIP, no GPU).
//
//   add_host fold       tail_fold_host (the statement of tail_fold_kernel) on exact-size buffers against a stable sort
//                       of the concatenated row: k in {1, 10, 64, 65, 1000, 1024}, P in {1, 2, 5}, n = 7; tail counts 0,
//                       1, < k, == k and every list full; graph rows full, partly padding, all padding, with duplicate
//                       ids; values that occur on both sides (the graph's entry first); equal distance bits inside the
//                       tail (by id); out-of-place and in place
//   add_host capacity   tail_capacity: never below the need, no change while the rows fit, O(log m) growths for m
//                       single-row adds, never beyond the id space
//
// Exit code 0 = all good.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../../rabitq-ann-search_amd/csrc/host_tail.h"

using namespace cph;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static uint64_t key_of(float d, uint32_t id) {
    uint32_t b;
    std::memcpy(&b, &d, 4);
    return ((uint64_t)b << 32) | id;
}

struct Entry {
    float d;
    int64_t id;
};

static int run_fold() {
    const uint64_t n = 7;
    const uint32_t base = 100000;
    int cases = 0;
    for (uint64_t k : {1u, 10u, 64u, 65u, 1000u, 1024u})
        for (uint32_t P : {1u, 2u, 5u}) {
            std::mt19937_64 rng(k * 31 + P);
            std::uniform_real_distribution<float> U(0.0f, 4.0f);
            uint32_t C = 128;
            while (C < 2 * k) C *= 2;
            std::vector<int64_t> g_ids(n * k, -1), out_ids(n * k, -7);
            std::vector<float> g_dist(n * k, FLT_MAX), out_dist(n * k, -7.0f);
            std::vector<uint64_t> pools((size_t)P * n * C, ~0ull);
            std::vector<uint32_t> counts((size_t)P * n, 0);
            std::vector<std::vector<Entry>> want(n);
            for (uint64_t q = 0; q < n; ++q) {
                const uint64_t gn_of[7] = {k, k / 2, 0, k, k, k, k / 3}, tn_of[7] = {1, (k - 1) / 2, k, 0, k, P * k, 0};
                const uint64_t gn = gn_of[q], tn = tn_of[q];
                std::vector<float> gd(gn);
                for (auto& x : gd) x = U(rng);
                std::sort(gd.begin(), gd.end());
                for (uint64_t i = 0; i < gn; ++i) {
                    g_dist[q * k + i] = gd[i];
                    g_ids[q * k + i] = (int64_t)(rng() % base);
                }
                if (q == 3 && gn >= 2) { g_ids[q * k + 1] = g_ids[q * k]; g_dist[q * k + 1] = g_dist[q * k]; }
                std::vector<uint64_t> keys(tn);
                for (uint64_t i = 0; i < tn; ++i) {
                    float d = U(rng);
                    if (q == 4 && i < (tn + 1) / 2) d = gd[rng() % gn];        // a value the graph's row holds too
                    if (q == 4 && i >= tn / 2) d = 2.5f;                      // equal bits inside the tail
                    keys[i] = key_of(d, base + (uint32_t)i * 3 + (uint32_t)(rng() % 3));
                }
                std::sort(keys.begin(), keys.end());
                std::vector<uint32_t> fill(P, 0);
                for (uint64_t i = 0; i < tn; ++i) {
                    uint32_t p = tn <= k ? (uint32_t)(rng() % P) : (uint32_t)(i % P);
                    pools[((size_t)p * n + q) * C + fill[p]++] = keys[i];
                }
                for (uint32_t p = 0; p < P; ++p) { REQUIRE(fill[p] <= k); counts[(size_t)p * n + q] = fill[p]; }
                // the statement, independently: the concatenated row, stably sorted by the float value
                std::vector<Entry> all;
                for (uint64_t i = 0; i < k; ++i) all.push_back(Entry{g_dist[q * k + i], g_ids[q * k + i]});
                for (uint64_t i = 0; i < std::min<uint64_t>(tn, k); ++i) {
                    const uint32_t b = (uint32_t)(keys[i] >> 32);
                    float d;
                    std::memcpy(&d, &b, 4);
                    all.push_back(Entry{d, (int64_t)(uint32_t)keys[i]});
                }
                std::stable_sort(all.begin(), all.end(), [](const Entry& x, const Entry& y) { return x.d < y.d; });
                all.resize(k);
                want[q] = all;
            }
            auto check = [&](const int64_t* ids, const float* dist) {
                for (uint64_t q = 0; q < n; ++q)
                    for (uint64_t i = 0; i < k; ++i) {
                        REQUIRE(ids[q * k + i] == want[q][i].id);
                        REQUIRE(std::memcmp(&dist[q * k + i], &want[q][i].d, 4) == 0);
                    }
            };
            tail_fold_host(g_ids.data(), g_dist.data(), n, k, pools.data(), counts.data(), P, C, out_ids.data(), out_dist.data());
            check(out_ids.data(), out_dist.data());
            // rows 2 and 6 of the shapes: an all-padding graph row is the tail's list; an empty tail leaves the row alone
            for (uint64_t i = 0; i < k; ++i) REQUIRE(out_ids[6 * k + i] == g_ids[6 * k + i] && out_ids[3 * k + i] == g_ids[3 * k + i]);
            REQUIRE(out_ids[2 * k] >= (int64_t)base);
            tail_fold_host(g_ids.data(), g_dist.data(), n, k, pools.data(), counts.data(), P, C, g_ids.data(), g_dist.data());   // in place
            check(g_ids.data(), g_dist.data());
            ++cases;
        }
    std::printf("fold: ok (%d cases)\n", cases);
    return 0;
}

static int run_capacity() {
    for (uint64_t cap : {0ull, 1ull, 300ull, 1000000ull, 4000000000ull})
        for (uint64_t need : {0ull, 1ull, 299ull, 300ull, 301ull, 2000000ull, 4294967294ull}) {
            const uint64_t c = tail_capacity(cap, need);
            if (need <= cap) REQUIRE(c == cap);
            else REQUIRE(c >= need && c <= 0xFFFFFFFFull && (c >= cap + cap / 2 || c == 0xFFFFFFFFull));
        }
    uint64_t cap = 300, growths = 0;
    for (uint64_t size = 300; size < 1300000; ++size)              // a million single-row adds
        if (size + 1 > cap) { cap = tail_capacity(cap, size + 1); ++growths; }
    REQUIRE(cap >= 1300000 && growths <= 30);      // log_1.5(1,300,000 / 1,024) = 17.6, plus the first steps of 1,024 rows
    std::printf("capacity: ok (%llu growths)\n", (unsigned long long)growths);
    return 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "fold") return run_fold();
    if (mode == "capacity") return run_capacity();
    std::fprintf(stderr, "usage: add_host fold | capacity\n");
    return 2;
}
