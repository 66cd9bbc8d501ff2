// partitioned.h — one index split across several devices (cph_parts_*): the host policy (host only, no HIP).
//
// A partitioned index is P independent single-device indexes over contiguous slices of the input rows; every query goes
// to all of them and the P result rows are merged on the device (device_merge.h).  This file holds what needs no GPU:
// the part bounds, the cut of a global allowed-row bitmap into one bitmap per part, and the fan-out that runs one
// callable on every part at once, on the persistent workers of multi_device.h's ReplicaPool (worker p = part p).
//
// What a part DOES is a callable, as in multi_device.h, so that the policy can be exercised without a GPU:
// tests/partitioned_host runs it under ThreadSanitizer and AddressSanitizer with a stand-in part.
#pragma once
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "multi_device.h"

namespace cph {

constexpr uint64_t kMinPartRows = 64;    // a part smaller than this is refused (the builder calibrates on >= 50 nodes)

struct PartBounds {
    uint64_t lo, hi;    // input rows [lo, hi)
};

// Rows of part p of P over n input rows (dist.shard_bounds: contiguous, sizes differ by at most one).
inline PartBounds part_bounds(uint64_t n, uint32_t P, uint32_t p) {
    if (P == 0 || p >= P) throw std::invalid_argument("part out of range");
    const uint64_t base = n / P, rem = n % P;
    const uint64_t lo = p * base + (p < rem ? p : rem);
    return PartBounds{lo, lo + base + (p < rem ? 1 : 0)};
}

// bounds[P + 1]: part p holds rows [bounds[p], bounds[p + 1]).
inline std::vector<uint64_t> all_part_bounds(uint64_t n, uint32_t P) {
    std::vector<uint64_t> b(P + 1);
    for (uint32_t p = 0; p < P; ++p) b[p] = part_bounds(n, P, p).lo;
    b[P] = n;
    return b;
}

// The mask cut: bits [lo, hi) of `words` (bit i & 31 of word i >> 5) as a bitmap of their own, bit 0 = row lo;
// (hi - lo + 31) / 32 words, the bits of the last word behind hi - lo clear.  lo and hi need not be multiples of 32.
inline std::vector<uint32_t> cut_mask(const uint32_t* words, uint64_t lo, uint64_t hi) {
    if (hi < lo) throw std::invalid_argument("mask cut: hi < lo");
    const uint64_t n = hi - lo, nw = (n + 31) / 32;
    std::vector<uint32_t> out(nw);
    const uint64_t w0 = lo >> 5, last = hi ? (hi - 1) >> 5 : 0;   // last: the last input word that holds a wanted bit
    const uint32_t sh = (uint32_t)(lo & 31);
    for (uint64_t w = 0; w < nw; ++w) {
        uint32_t x = words[w0 + w] >> sh;
        if (sh && w0 + w + 1 <= last) x |= words[w0 + w + 1] << (32 - sh);
        out[w] = x;
    }
    if (n & 31) out[nw - 1] &= (1u << (n & 31)) - 1u;
    return out;
}

// A copy between a part's device and the home device, as the steps the library fills in.  With peer access it is one
// command on the part's stream, ordered there behind the search that wrote the source.  Without, it goes through pinned
// host memory with BLOCKING copies, which do not wait for the part's (non-blocking) stream: the stream has to be
// synchronised first, or the copy reads rows the search has not written yet.  The order is the policy; it is stated
// here so that it can be run without a GPU.
struct CrossDeviceCopy {
    std::function<void()> peer_async;     // enqueue the peer copy on the part's stream
    std::function<void()> sync_source;    // wait for everything enqueued on the part's stream
    std::function<void()> to_host;        // blocking: source -> pinned host buffer
    std::function<void()> from_host;      // blocking: pinned host buffer -> destination
};
inline void cross_device_copy(bool peer, const CrossDeviceCopy& ops) {
    if (peer) {
        ops.peer_async();
        return;
    }
    ops.sync_source();
    ops.to_host();
    ops.from_host();
}

// Runs work(p, err) for every part p = 0..P-1 at once, part p on worker p of `pool`, and returns when all of them have
// finished -- on error too, so that no worker touches the caller's memory afterwards.  work returns a status (0 = ok)
// and fills err on failure; an exception escaping it is turned into a status by the pool.  Returns 0, or the status of
// the lowest-numbered failing part, its message in `err`.
inline int run_on_parts(ReplicaPool& pool, uint32_t P, const std::function<int(uint32_t, std::string&)>& work, std::string& err) {
    if (P == 0 || P > pool.size()) throw std::invalid_argument("more parts than workers");
    std::vector<Shard> plan(P);
    for (uint32_t p = 0; p < P; ++p) plan[p] = Shard{p, 0, 0};
    return pool.run(plan, [&work](const Shard& s, std::string& e) { return work(s.replica, e); }, err);
}

}  // namespace cph
