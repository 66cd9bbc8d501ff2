// multi_host.cpp -- the query split and the replica worker pool of csrc/multi_device.h with a stand-in launch (no HIP,
// no GPU).  tests/test_multi_device_host.py builds it twice with plain g++: -fsanitize=thread and
// -fsanitize=address,undefined.  Exit code 0 = every check passed; a sanitizer report makes the binary exit non-zero.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../rabitq-ann-search_amd/csrc/multi_device.h"

using namespace cph;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

static void sleep_us(int us) { std::this_thread::sleep_for(std::chrono::microseconds(us)); }

// Shard sizes of a plan, in query order, and the replicas they run on.
static void check_plan(uint64_t n, uint32_t R, uint64_t min_shard, uint32_t first, const std::vector<uint64_t>& sizes,
                       const std::vector<uint32_t>& reps) {
    const std::vector<Shard> p = plan_shards(n, R, min_shard, first);
    REQUIRE(p.size() == sizes.size());
    uint64_t at = 0;
    for (size_t j = 0; j < p.size(); ++j) {
        REQUIRE(p[j].lo == at);
        REQUIRE(p[j].hi - p[j].lo == sizes[j]);
        REQUIRE(p[j].replica == reps[j]);
        at = p[j].hi;
    }
    REQUIRE(at == n);
}

// Rows of every call: out[row] = 1000 * replica + 1 (once), counted per row.
struct Rows {
    std::vector<int> out;
    std::vector<std::atomic<int>> writes;
    explicit Rows(size_t n) : out(n, -1), writes(n) { for (auto& w : writes) w = 0; }
};

static ReplicaPool::Launch writer(Rows& rows, uint64_t seed, int max_sleep_us) {
    return [&rows, seed, max_sleep_us](const Shard& s, std::string&) {
        std::mt19937_64 rng(seed ^ (s.lo * 0x9E3779B97F4A7C15ULL) ^ s.replica);
        sleep_us((int)(rng() % (uint64_t)(max_sleep_us + 1)));
        for (uint64_t r = s.lo; r < s.hi; ++r) {
            rows.out[r] = 1000 * (int)s.replica + 1;
            rows.writes[r].fetch_add(1);
        }
        return 0;
    };
}

static void check_rows(const Rows& rows, const std::vector<Shard>& plan) {
    for (const Shard& s : plan)
        for (uint64_t r = s.lo; r < s.hi; ++r) {
            REQUIRE(rows.writes[r].load() == 1);
            REQUIRE(rows.out[r] == 1000 * (int)s.replica + 1);
        }
}

static std::atomic<int> g_inits{0}, g_exits{0};
struct ExitMark {
    bool armed = false;
    ~ExitMark() { if (armed) g_exits.fetch_add(1); }
};
static void init_worker(uint32_t) {
    thread_local ExitMark m;
    m.armed = true;
    g_inits.fetch_add(1);
}

int main() {
    // ---- shard bounds --------------------------------------------------------------------------------------------
    {
        check_plan(10, 3, 1, 0, {4, 3, 3}, {0, 1, 2});
        check_plan(11, 4, 1, 2, {3, 3, 3, 2}, {2, 3, 0, 1});
        check_plan(2, 4, 1, 1, {1, 1}, {1, 2});
        check_plan(1, 4, 1, 3, {1}, {3});
        check_plan(0, 4, 1, 1, {0}, {1});
        check_plan(2047, 4, 1024, 2, {2047}, {2});
        check_plan(2048, 4, 1024, 0, {1024, 1024}, {0, 1});
        check_plan(3000, 4, 1024, 0, {1500, 1500}, {0, 1});
        check_plan(10000, 4, 1024, 1, {2500, 2500, 2500, 2500}, {1, 2, 3, 0});
        check_plan(10000, 16, 1024, 0, {1112, 1111, 1111, 1111, 1111, 1111, 1111, 1111, 1111}, {0, 1, 2, 3, 4, 5, 6, 7, 8});
        check_plan(5, 1, 1, 7, {5}, {0});                             // one replica: `first` wraps
        bool threw = false;
        try { plan_shards(5, 0, 1, 0); } catch (const std::invalid_argument&) { threw = true; }
        REQUIRE(threw);
        std::printf("plans: ok\n");
    }
    // ---- every row written once, by its shard's replica; nothing written after return ----------------------------
    {
        ReplicaPool pool(4, init_worker);
        REQUIRE(pool.size() == 4);
        std::mt19937_64 rng(7);
        for (int it = 0; it < 60; ++it) {
            const uint64_t n = rng() % 300;
            const uint64_t ms = 1 + rng() % 40;
            const std::vector<Shard> plan = plan_shards(n, 4, ms, (uint32_t)(rng() % 4));
            auto rows = std::make_unique<Rows>(n);
            std::string err;
            REQUIRE(pool.run(plan, writer(*rows, rng(), 300), err) == 0);
            check_rows(*rows, plan);
            rows.reset();                 // a late write would now touch freed memory (AddressSanitizer)
        }
        std::printf("rows: ok\n");
    }
    // ---- errors: the lowest-numbered failing replica's status and message, only after every shard has finished ----
    {
        ReplicaPool pool(4, nullptr);
        const std::vector<Shard> plan = plan_shards(400, 4, 1, 0);
        std::atomic<int> finished{0};
        std::string err;
        const int rc = pool.run(plan, [&](const Shard& s, std::string& e) {
            sleep_us(s.replica == 0 ? 20000 : 1000 * (int)s.replica);    // the successful shard is the slowest
            finished.fetch_add(1);
            if (s.replica == 2) { e = "replica two failed"; return 2; }
            if (s.replica == 3) throw std::invalid_argument("replica three failed");
            return 0;
        }, err);
        REQUIRE(finished.load() == 4);
        REQUIRE(rc == 2);
        REQUIRE(err == "replica two failed");
        // an exception is a status too: invalid_argument -> 1, bad_alloc -> 3, anything else -> 2
        std::string err2;
        const int rc2 = pool.run(plan, [&](const Shard& s, std::string&) -> int {
            if (s.replica == 1) throw std::invalid_argument("bad shard");
            if (s.replica == 3) throw std::bad_alloc();
            return 0;
        }, err2);
        REQUIRE(rc2 == 1 && err2 == "bad shard");
        std::string err3;
        const int rc3 = pool.run(plan_shards(400, 4, 1, 0), [&](const Shard& s, std::string&) -> int {
            if (s.replica >= 2) throw std::bad_alloc();
            return 0;
        }, err3);
        REQUIRE(rc3 == 3 && err3 == "out of memory");
        // the pool is still usable after failures
        Rows rows(50);
        std::string ok_err;
        const std::vector<Shard> p2 = plan_shards(50, 4, 1, 1);
        REQUIRE(pool.run(p2, writer(rows, 3, 100), ok_err) == 0);
        check_rows(rows, p2);
        std::printf("errors: ok\n");
    }
    // ---- 8 callers at once share the workers ---------------------------------------------------------------------
    {
        ReplicaPool pool(3, nullptr);
        std::atomic<int> bad{0};
        std::vector<std::thread> th;
        for (int t = 0; t < 8; ++t)
            th.emplace_back([&, t] {
                std::mt19937_64 rng(100 + t);
                for (int it = 0; it < 40; ++it) {
                    const uint64_t n = 1 + rng() % 200;
                    const std::vector<Shard> plan = plan_shards(n, 3, 1 + rng() % 20, (uint32_t)(rng() % 3));
                    Rows rows(n);
                    std::string err;
                    if (pool.run(plan, writer(rows, rng(), 200), err) != 0) { bad.fetch_add(1); continue; }
                    for (const Shard& s : plan)
                        for (uint64_t r = s.lo; r < s.hi; ++r)
                            if (rows.writes[r].load() != 1 || rows.out[r] != 1000 * (int)s.replica + 1) bad.fetch_add(1);
                }
            });
        for (auto& x : th) x.join();
        REQUIRE(bad.load() == 0);
        std::printf("concurrent: ok\n");
    }
    // ---- destroy joins the workers ---------------------------------------------------------------------------------
    {
        g_inits = 0;
        g_exits = 0;
        {
            ReplicaPool pool(5, init_worker);
            Rows rows(100);
            std::string err;
            const std::vector<Shard> plan = plan_shards(100, 5, 1, 0);
            REQUIRE(pool.run(plan, writer(rows, 9, 100), err) == 0);
            check_rows(rows, plan);
        }
        REQUIRE(g_inits.load() == 5);
        REQUIRE(g_exits.load() == 5);       // every worker thread has exited when the destructor returns
        bool threw = false;
        try { ReplicaPool bad(0, nullptr); } catch (const std::invalid_argument&) { threw = true; }
        REQUIRE(threw);
        threw = false;
        try { ReplicaPool bad(kMaxReplicas + 1, nullptr); } catch (const std::invalid_argument&) { threw = true; }
        REQUIRE(threw);
        std::printf("destroy: ok\n");
    }
    std::printf("multi_host: ok\n");
    return 0;
}
