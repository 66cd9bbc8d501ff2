// part_host.cpp — csrc/partitioned.h without a GPU: the part bounds, the mask cut and the fan-out over the parts, driven
// with a stand-in part (tests/test_partition_host.py builds this under ThreadSanitizer and AddressSanitizer + UBSan).
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../rabitq-ann-search_amd/csrc/host_parallel.h"
#include "../../rabitq-ann-search_amd/csrc/partitioned.h"

using namespace cph;

#define REQUIRE(cond)                                                                     \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "%s:%d: requirement failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                                 \
        }                                                                                 \
    } while (0)

static void test_bounds() {
    for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 6001ull, 1000003ull})
        for (uint32_t P : {1u, 2u, 3u, 7u, 16u}) {
            const std::vector<uint64_t> b = all_part_bounds(n, P);
            REQUIRE(b.size() == P + 1 && b[0] == 0 && b[P] == n);
            uint64_t lo_size = ~0ull, hi_size = 0;
            for (uint32_t p = 0; p < P; ++p) {
                const PartBounds pb = part_bounds(n, P, p);
                REQUIRE(pb.lo == b[p] && pb.hi == b[p + 1] && pb.hi >= pb.lo);
                lo_size = std::min(lo_size, pb.hi - pb.lo);
                hi_size = std::max(hi_size, pb.hi - pb.lo);
                if (p + 1 < P) REQUIRE((pb.hi - pb.lo) >= (b[p + 2] - b[p + 1]));   // the longer parts come first
            }
            REQUIRE(hi_size - lo_size <= 1);
        }
    REQUIRE(part_bounds(6001, 3, 0).hi == 2001 && part_bounds(6001, 3, 1).hi == 4001);
    bool threw = false;
    try { (void)part_bounds(10, 3, 3); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
    std::puts("bounds: ok");
}

// The cut against a bit-by-bit restatement, at bounds that are not multiples of 32 (and some that are).  The input
// vector has exactly (n + 31) / 32 words: a read past the last wanted word is an AddressSanitizer report.
static void test_mask_cut() {
    std::mt19937_64 rng(7);
    for (uint64_t n : {1ull, 31ull, 32ull, 33ull, 95ull, 6001ull, 4000ull}) {
        std::vector<uint32_t> words((n + 31) / 32);
        for (uint32_t& w : words) w = (uint32_t)rng();
        auto bit = [&](uint64_t i) { return (words[i >> 5] >> (i & 31)) & 1u; };
        std::vector<std::pair<uint64_t, uint64_t>> cuts = {{0, n}, {0, 0}, {n, n}, {n / 3, n}, {n / 3, 2 * n / 3}, {0, n / 2}};
        for (uint32_t P : {2u, 3u, 7u, 16u})
            for (uint32_t p = 0; p < P; ++p) cuts.push_back({part_bounds(n, P, p).lo, part_bounds(n, P, p).hi});
        for (auto [lo, hi] : cuts) {
            const std::vector<uint32_t> out = cut_mask(words.data(), lo, hi);
            REQUIRE(out.size() == (hi - lo + 31) / 32);
            for (uint64_t i = 0; i < out.size() * 32; ++i) {
                const uint32_t got = (out[i >> 5] >> (i & 31)) & 1u;
                REQUIRE(got == (i < hi - lo ? bit(lo + i) : 0u));
            }
        }
    }
    // the slices of a partition hold every bit exactly once: the popcounts add up
    const uint64_t n = 6001;
    std::vector<uint32_t> words((n + 31) / 32);
    for (uint32_t& w : words) w = (uint32_t)rng();
    words.back() &= (1u << (n & 31)) - 1u;
    uint64_t all = 0, sum = 0;
    for (uint32_t w : words) all += (uint64_t)__builtin_popcount(w);
    for (uint32_t p = 0; p < 3; ++p)
        for (uint32_t w : cut_mask(words.data(), part_bounds(n, 3, p).lo, part_bounds(n, 3, p).hi)) sum += (uint64_t)__builtin_popcount(w);
    REQUIRE(all == sum);
    bool threw = false;
    try { (void)cut_mask(words.data(), 5, 4); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
    std::puts("mask_cut: ok");
}

// Every part runs exactly once per call, part p on worker p, all at once; the call returns after the last one.
static void test_fan_out() {
    for (uint32_t P : {1u, 3u, 16u}) {
        std::vector<std::thread::id> worker(P);
        ReplicaPool pool(P, [&](uint32_t r) { worker[r] = std::this_thread::get_id(); });
        for (int round = 0; round < 20; ++round) {
            std::vector<int> runs(P, 0);
            std::vector<uint64_t> rows(P * 8, 0);
            std::atomic<uint32_t> inside{0}, peak{0};
            std::string err;
            const int rc = run_on_parts(pool, P, [&](uint32_t p, std::string&) {
                const uint32_t now = ++inside;
                uint32_t seen = peak.load();
                while (now > seen && !peak.compare_exchange_weak(seen, now)) {}
                std::this_thread::sleep_for(std::chrono::microseconds(200 + 100 * ((p * 7 + (uint32_t)round) % 5)));
                REQUIRE(std::this_thread::get_id() == worker[p]);
                ++runs[p];
                for (int j = 0; j < 8; ++j) rows[p * 8 + (size_t)j] = (uint64_t)p * 100 + (uint64_t)j;   // the part's own rows only
                --inside;
                return 0;
            }, err);
            REQUIRE(rc == 0 && err.empty() && inside.load() == 0);
            for (uint32_t p = 0; p < P; ++p) {
                REQUIRE(runs[p] == 1);
                for (int j = 0; j < 8; ++j) REQUIRE(rows[p * 8 + (size_t)j] == (uint64_t)p * 100 + (uint64_t)j);
            }
            REQUIRE(peak.load() >= 1 && peak.load() <= P);
        }
    }
    {
        ReplicaPool pool(2, nullptr);
        std::string err;
        bool threw = false;
        try { (void)run_on_parts(pool, 3, [](uint32_t, std::string&) { return 0; }, err); } catch (const std::invalid_argument&) { threw = true; }
        REQUIRE(threw);
    }
    std::puts("fan_out: ok");
}

// One part fails with a status, one throws: the call returns only after every part has finished, with the status and
// the message of the lowest-numbered failing part; the pool serves the next call as if nothing had happened.
static void test_errors() {
    const uint32_t P = 5;
    ReplicaPool pool(P, nullptr);
    std::atomic<uint32_t> finished{0};
    auto part = [&](uint32_t fail_at, uint32_t throw_at, bool invalid) {
        return [&, fail_at, throw_at, invalid](uint32_t p, std::string& e) -> int {
            std::this_thread::sleep_for(std::chrono::microseconds(p == fail_at ? 100 : 1500));   // the failing part finishes first
            ++finished;
            if (p == throw_at) {
                if (invalid) throw std::invalid_argument("part " + std::to_string(p) + " threw invalid_argument");
                throw std::runtime_error("part " + std::to_string(p) + " threw");
            }
            if (p == fail_at) {
                e = "part " + std::to_string(p) + " failed";
                return 2;
            }
            return 0;
        };
    };
    std::string err;
    finished = 0;
    int rc = run_on_parts(pool, P, part(3, 1, false), err);
    REQUIRE(finished.load() == P);                       // nobody still runs when the call has returned
    REQUIRE(rc == 2 && err == "part 1 threw");           // part 1 < part 3
    finished = 0;
    rc = run_on_parts(pool, P, part(2, 4, true), err);
    REQUIRE(finished.load() == P && rc == 2 && err == "part 2 failed");
    finished = 0;
    rc = run_on_parts(pool, P, part(4, 0, true), err);
    REQUIRE(finished.load() == P && rc == 1 && err == "part 0 threw invalid_argument");
    finished = 0;
    err.clear();
    rc = run_on_parts(pool, P, part(99, 99, false), err);
    REQUIRE(finished.load() == P && rc == 0 && err.empty());
    std::puts("errors: ok");
}

// Several callers share the workers: every call still sees every part exactly once.
static void test_concurrent() {
    const uint32_t P = 4, callers = 6;
    ReplicaPool pool(P, nullptr);
    std::vector<std::thread> th;
    std::atomic<uint32_t> bad{0};
    for (uint32_t c = 0; c < callers; ++c)
        th.emplace_back([&, c] {
            for (int round = 0; round < 25; ++round) {
                std::vector<uint32_t> mine(P, 0);
                std::string err;
                const int rc = run_on_parts(pool, P, [&](uint32_t p, std::string&) { mine[p] += c + 1; return 0; }, err);
                if (rc != 0) ++bad;
                for (uint32_t p = 0; p < P; ++p)
                    if (mine[p] != c + 1) ++bad;
            }
        });
    for (auto& t : th) t.join();
    REQUIRE(bad.load() == 0);
    std::puts("concurrent: ok");
}

// The copy without peer access: a stand-in stream (a thread) is still writing the part's rows when the copy is asked
// for.  sync_source waits for it; the blocking copies read the rows after that.  Left out or called late, the read
// races with the writer (a ThreadSanitizer report) and the rows arrive incomplete.
static void test_copy_order() {
    for (int round = 0; round < 10; ++round) {
        const size_t n = 4096;
        std::vector<int64_t> rows(n, -1), pinned(n, -2), home(n, -3);
        std::thread stream([&] {
            std::this_thread::sleep_for(std::chrono::microseconds(300));
            for (size_t i = 0; i < n; ++i) rows[i] = (int64_t)i;
        });
        std::vector<std::string> order;
        CrossDeviceCopy ops;
        ops.peer_async = [&] { order.push_back("peer"); };
        ops.sync_source = [&] { stream.join(); order.push_back("sync"); };
        ops.to_host = [&] { pinned = rows; order.push_back("to_host"); };
        ops.from_host = [&] { home = pinned; order.push_back("from_host"); };
        cross_device_copy(false, ops);
        REQUIRE((order == std::vector<std::string>{"sync", "to_host", "from_host"}));
        for (size_t i = 0; i < n; ++i) REQUIRE(home[i] == (int64_t)i);
    }
    {   // with peer access: one command on the part's stream, nothing blocking
        std::vector<std::string> order;
        CrossDeviceCopy ops;
        ops.peer_async = [&] { order.push_back("peer"); };
        ops.sync_source = ops.to_host = ops.from_host = [&] { order.push_back("blocking"); };
        cross_device_copy(true, ops);
        REQUIRE((order == std::vector<std::string>{"peer"}));
    }
    std::puts("copy_order: ok");
}

// A builder that shares the host threads with P - 1 others: the divided count holds on the builder's thread, on the
// workers of run_threads, and on a bare std::thread that adopts the share (the upper-layer job of builder_pipeline.h);
// a thread that does not adopt it sees the whole budget, and the share ends with its scope.
static void test_thread_share() {
    REQUIRE(setenv("CPH_BUILD_THREADS", "12", 1) == 0);
    REQUIRE(host_threads() == 12);
    {
        HostThreadsShare share(4);
        REQUIRE(host_threads() == 3);
        std::vector<size_t> seen(5, 0);
        run_threads(5, [&](size_t t) { seen[t] = host_threads(); });
        for (size_t v : seen) REQUIRE(v == 3);
        size_t nested = 0;
        run_threads(2, [&](size_t t) {
            if (t == 1) run_threads(2, [&](size_t u) { if (u == 1) nested = host_threads(); });
        });
        REQUIRE(nested == 3);
        size_t adopted = 0, bare = 0;
        const size_t inherited = host_threads_divisor();
        std::thread a([&, inherited] {
            HostThreadsShare mine(inherited);
            adopted = host_threads();
        });
        std::thread b([&] { bare = host_threads(); });
        a.join();
        b.join();
        REQUIRE(adopted == 3 && bare == 12);
        {
            HostThreadsShare more(100);           // more sharers than threads: one each
            REQUIRE(host_threads() == 1);
        }
        REQUIRE(host_threads() == 3);
    }
    REQUIRE(host_threads() == 12);
    // P builders at once, as cph_parts_finalize runs them: together they stay within the budget
    const uint32_t P = 4;
    ReplicaPool pool(P, nullptr);
    std::vector<size_t> per(P, 0);
    std::string err;
    const int rc = run_on_parts(pool, P, [&](uint32_t p, std::string&) {
        HostThreadsShare share(P);
        const size_t inherited = host_threads_divisor();
        std::thread job([&, inherited, p] {
            HostThreadsShare mine(inherited);
            per[p] = host_threads();
        });
        job.join();
        return 0;
    }, err);
    REQUIRE(rc == 0);
    size_t total = 0;
    for (size_t v : per) total += v;
    REQUIRE(total == 12);
    REQUIRE(unsetenv("CPH_BUILD_THREADS") == 0);
    std::puts("thread_share: ok");
}

int main() {
    test_bounds();
    test_mask_cut();
    test_fan_out();
    test_errors();
    test_concurrent();
    test_copy_order();
    test_thread_share();
    std::puts("part_host: ok");
    return 0;
}
