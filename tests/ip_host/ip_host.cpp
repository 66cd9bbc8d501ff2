// Stand-alone driver of csrc/host_ip.h for the CPU tests (tests/test_ip_host.py): built with plain g++,
// -fsanitize=address,undefined and -ffp-contract=off, run as a child process.  It reads the cases the Python test wrote --
// inputs and the outputs tests/ip_model.py expects -- runs the host twin on heap buffers of exactly the stated sizes and
// compares every output byte and every counter.  It also pins the native file's metric record (csrc/native_file.h): a
// reader that knows formats up to 4 refuses a format-5 record by its version, before it reads the bytes behind the
// first 16.
//
// File: u64 n_cases, then per case u64 {kind, n, w, bad, over, first}, f32 m2 and the arrays
//   kind 0 (rows, bound m2), 1 (rows, bound from the data; m2 = the bound expected):  x f32[n*w], out f32[n*(w+1)] (expected)
//   kind 2 (queries against m2):  x f32[n*w], out f32[n*(w+1)], c f32[n] (both expected)
//   kind 3 (epilogue, w = k):  ids i64[n*w], dist f32[n*w], c f32[n], scores f32[n*w] (expected)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "../../rabitq-ann-search_amd/csrc/host_ip.h"
#include "../../rabitq-ann-search_amd/csrc/native_file.h"

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

#define REQUIRE(cond)                                                          \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("ip: line %d: %s does not hold\n", __LINE__, #cond);   \
            return 1;                                                          \
        }                                                                      \
    } while (0)

template <class F>
std::string attempt(F&& f) {
    try { f(); return ""; } catch (const std::exception& e) { return std::string("!") + e.what(); }
}

// The metric record of the native file: what a format-4 reader and a format-5 reader make of each record.
int check_metric_record() {
    using namespace cph;
    const NativeMetricIpExt ip{kNativeMetricMagic, kNativeVersionIp, kNativeMetricIp, 12.5f, 0u};
    const NativeMetricExt cosine{kNativeMetricMagic, kNativeVersionMetric, kNativeMetricCosine};
    std::unique_ptr<uint8_t[]> r5(new uint8_t[sizeof(ip)]), r4(new uint8_t[sizeof(cosine)]);     // exact sizes
    std::memcpy(r5.get(), &ip, sizeof(ip));
    std::memcpy(r4.get(), &cosine, sizeof(cosine));
    uint32_t metric = 99;
    float m2 = -1.0f;
    // the format-5 reader
    REQUIRE(read_metric_record(r5.get(), sizeof(ip), 5, &metric, &m2) == 24 && metric == kNativeMetricIp && m2 == 12.5f);
    REQUIRE(read_metric_record(r4.get(), sizeof(cosine), 5, &metric, &m2) == 16 && metric == kNativeMetricCosine && m2 == 0.0f);
    // the format-4 reader: the cosine record as before, the format-5 record refused by its version -- also when only
    // the 16 bytes such a reader knows are readable
    REQUIRE(read_metric_record(r4.get(), sizeof(cosine), 4, &metric, &m2) == 16 && metric == kNativeMetricCosine);
    metric = 99;
    const std::string e = attempt([&] { read_metric_record(r5.get(), sizeof(ip), 4, &metric, &m2); });
    REQUIRE(e.find("Unsupported native index file version: 5") != std::string::npos && metric == 99);
    REQUIRE(attempt([&] { read_metric_record(r5.get(), 16, 4, &metric, &m2); }).find("version: 5") != std::string::npos);
    // damage: no magic is no record; a truncated or mislabelled format-5 record, a bad bound and a set reserved word are refused
    REQUIRE(read_metric_record(r5.get() + 8, 16, 5, &metric, &m2) == 0 && read_metric_record(r5.get(), 15, 5, &metric, &m2) == 0);
    REQUIRE(!attempt([&] { read_metric_record(r5.get(), 16, 5, &metric, &m2); }).empty());
    auto damaged = [&](size_t off, uint32_t value) {
        std::unique_ptr<uint8_t[]> g(new uint8_t[sizeof(ip)]);
        std::memcpy(g.get(), &ip, sizeof(ip));
        std::memcpy(g.get() + off, &value, 4);
        return attempt([&] { read_metric_record(g.get(), sizeof(ip), 5, &metric, &m2); });
    };
    REQUIRE(!damaged(8, 6).empty() && !damaged(12, 1).empty() && !damaged(20, 1).empty());
    REQUIRE(!damaged(16, 0x7FC00000u).empty() && !damaged(16, 0x7F800000u).empty() && !damaged(16, 0xBF800000u).empty());
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: ip_host <cases file>\n");
        return 2;
    }
    if (check_metric_record() != 0) return 1;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    const uint64_t n_cases = read_array<uint64_t>(f, 1)[0];
    for (uint64_t c = 0; c < n_cases; ++c) {
        const auto hd = read_array<uint64_t>(f, 6);
        const uint64_t kind = hd[0], n = hd[1], w = hd[2];
        const float m2 = read_array<float>(f, 1)[0];
        bool ok = false;
        if (kind == 3) {
            const uint64_t cells = n * w;
            const auto ids = read_array<int64_t>(f, cells);
            const auto dist = read_array<float>(f, cells);
            const auto cq = read_array<float>(f, n);
            const auto want = read_array<float>(f, cells);
            cph::ip_epilogue_host(ids.get(), dist.get(), n, w, cq.get());
            ok = std::memcmp(dist.get(), want.get(), cells * 4) == 0;
        } else {
            const uint64_t cells = n * w, ocells = n * (w + 1);
            const auto x = read_array<float>(f, cells);
            const auto want = read_array<float>(f, ocells);
            const auto want_c = read_array<float>(f, kind == 2 ? n : 0);
            std::unique_ptr<float[]> out(new float[ocells]), cq(new float[kind == 2 ? n : 0]);
            std::memset(out.get(), 0xA5, ocells * 4);       // (nothing depends on what the outputs held)
            uint64_t cnt[3] = {0, 0, cph::kIpNoRow};
            const float bound = kind == 1 ? cph::ip_max_sq_norm_host(x.get(), n, (uint32_t)w, nullptr) : m2;
            cph::ip_augment_host(x.get(), n, (uint32_t)w, bound, out.get(), kind == 2 ? cq.get() : nullptr, cnt);
            cph::ip_augment_host(x.get(), n, (uint32_t)w, bound, out.get(), kind == 2 ? cq.get() : nullptr, nullptr);    // (null counters are allowed)
            ok = std::memcmp(out.get(), want.get(), ocells * 4) == 0 && std::memcmp(&bound, &m2, 4) == 0 && cnt[0] == hd[3] &&
                 cnt[1] == hd[4] && cnt[2] == hd[5] && (kind != 2 || std::memcmp(cq.get(), want_c.get(), n * 4) == 0);
        }
        if (!ok) {
            std::printf("ip: case %llu differs (kind=%llu n=%llu w=%llu)\n", (unsigned long long)c, (unsigned long long)kind,
                        (unsigned long long)n, (unsigned long long)w);
            return 1;
        }
    }
    std::fclose(f);
    std::printf("ip: ok (%llu cases)\n", (unsigned long long)n_cases);
    return 0;
}
