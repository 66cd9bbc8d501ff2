// device_group.h — grouped search (cph_search_grouped*): the k best key groups of a candidate row, up to g rows of each.
//
// The statement is host_group.h's: walk the row front to back, skip padding and repeated ids, open a group for a new key
// while fewer than k exist, append to a group with fewer than g members, drop the rest.  group_rows_kernel does that walk
// with one wave per row, 64 entries at a time, against a small group table in LDS:
//     g_key[k], g_cnt[k]   key and member count of every group opened so far
//     g_mem[k][g]          the members' INTERNAL ids (the output may carry input rows)
// A chunk's 64 entries are resolved against the table (a lane scans the keys, then its group's members for its own id)
// and against each other (one round of 64 lane reads gives every lane the mask of the chunk's lanes with its key, and
// whether a lower lane holds its id).  From the two masks a lane knows, without another pass: whether it is the first of a
// new key (and so which group index the key gets: the groups so far plus the first-of-new-key lanes below it), its rank
// inside the key, and whether it is kept.  A repeated id is only recognised when its earlier copy was KEPT or sits in
// the same chunk; an earlier copy that was dropped was dropped because its group was full or could not be opened, which
// stays true, so the later copy is dropped by the same rule and the outputs are those of the statement.
// The walk stops at the first chunk after which k groups are full: nothing behind it can change an output.  That is the
// common case (k = 10, g = 3 out of C = 128: one or two chunks); the worst case (k = 1024 groups of one) scans a table of
// up to 1,024 keys for each of 16 chunks.
// Every output slot is written here: members as they are kept, the rest as padding at the end.  Nothing depends on a
// memset.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_buf.h"
#include "host_group.h"

namespace cph {

struct GroupArgs {
    const int64_t* ids;                   // [n][C] candidate rows: internal ids, -1 = padding
    const float* dist;                    // [n][C]
    uint32_t C, k, g;                     // 1 <= k, 1 <= g, k * g <= C <= kGroupMaxCandidates
    const int32_t* key_of;                // [n_ids]
    uint32_t n_ids;                       // ids at or above this are treated as padding (no search returns one)
    const uint32_t* rows;                 // [n_ids] row map, or null: ids are written as they are
    int64_t* out_ids;                     // [n][k][g]
    float* out_dist;                      // [n][k][g]
    int32_t* out_keys;                    // [n][k]
    int32_t* out_counts;                  // [n][k]
    uint8_t* out_complete;                // [n]
};

inline size_t group_lds_bytes(uint32_t k, uint32_t g) {
    return ((size_t)2 * k + (size_t)k * g) * 4;          // at most 12 KiB
}

// Grid n, one wave per workgroup; LDS: group_lds_bytes(k, g).
__global__ __launch_bounds__(64) void group_rows_kernel(GroupArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    int32_t* g_key = reinterpret_cast<int32_t*>(smem);
    uint32_t* g_cnt = reinterpret_cast<uint32_t*>(smem) + a.k;
    uint32_t* g_mem = g_cnt + a.k;
    const uint32_t C = a.C, k = a.k, g = a.g;
    const int lane = threadIdx.x;
    const size_t q = blockIdx.x;
    const int64_t* __restrict__ row_ids = a.ids + q * C;
    const uint32_t* __restrict__ row_dist = reinterpret_cast<const uint32_t*>(a.dist) + q * C;
    int64_t* __restrict__ out_ids = a.out_ids + q * k * g;
    uint32_t* __restrict__ out_dist = reinterpret_cast<uint32_t*>(a.out_dist) + q * k * g;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t n_groups = 0, n_full = 0, n_valid = 0;      // (wave-uniform)
    bool all_full = false;

    for (uint32_t base = 0; base < C; base += 64) {
        const uint32_t j = base + lane;
        const int64_t id64 = j < C ? row_ids[j] : -1;
        const bool valid = id64 >= 0 && (unsigned long long)id64 < a.n_ids;
        const uint32_t id = (uint32_t)id64;
        const uint32_t dbits = j < C ? row_dist[j] : 0u;
        const int32_t key = valid ? a.key_of[id] : 0;
        const unsigned long long vmask = __ballot(valid);
        n_valid += (uint32_t)__popcll(vmask);
        if (vmask == 0) continue;

        // against the table: the key's group, its members so far, my id among them
        int gi = -1;
        for (uint32_t t = 0; t < n_groups; ++t)
            if (g_key[t] == key) gi = (int)t;             // (keys of the table are distinct)
        if (!valid) gi = -1;
        const uint32_t before = gi >= 0 ? g_cnt[gi] : 0u;
        bool dup = false;
        for (uint32_t m = 0; m < before; ++m) dup |= g_mem[(uint32_t)gi * g + m] == id;

        // against the chunk: the lanes with my key, my id in a lower lane
        unsigned long long same = 0;
        for (unsigned long long rest = vmask; rest; rest &= rest - 1ull) {
            const int jj = __builtin_ctzll(rest);         // (uniform)
            const int32_t kj = __shfl(key, jj);
            const uint32_t idj = __shfl(id, jj);
            if (kj == key) same |= 1ull << jj;
            if (idj == id && jj < lane) dup = true;
        }
        if (!valid) same = 1ull << lane;                  // (unused; keeps the bit scans below defined)
        const unsigned long long dmask = __ballot(valid && dup);
        const int first = __builtin_ctzll(same), last = 63 - __builtin_clzll(same);
        const unsigned long long fnmask = __ballot(valid && gi < 0 && first == lane);     // first entries of new keys

        int G = gi;
        if (valid && gi < 0) {
            const uint32_t idx = n_groups + (uint32_t)__popcll(fnmask & ((1ull << first) - 1ull));
            G = idx < k ? (int)idx : -1;
        }
        const unsigned long long live = same & ~dmask;    // the chunk's entries of my key that are no repeats
        const uint32_t rank = before + (uint32_t)__popcll(live & below);
        if (valid && !dup && G >= 0 && rank < g) {
            const uint32_t o = (uint32_t)G * g + rank;
            out_ids[o] = (int64_t)(a.rows ? a.rows[id] : id);
            out_dist[o] = dbits;
            g_mem[o] = id;
        }
        // the key's last lane of the chunk keeps the table
        const bool keeper = valid && G >= 0 && last == lane;
        const uint32_t total = before + (uint32_t)__popcll(live);
        const uint32_t now = total < g ? total : g;
        if (keeper) {
            g_cnt[G] = now;
            if (gi < 0) g_key[G] = key;
        }
        n_full += (uint32_t)__popcll(__ballot(keeper && before < g && now == g));
        n_groups += (uint32_t)__popcll(fnmask);
        if (n_groups > k) n_groups = k;
        __syncthreads();
        if (n_full == k) {
            all_full = true;
            break;
        }
    }

    __syncthreads();
    for (uint32_t t = lane; t < k * g; t += 64) {
        const uint32_t G = t / g, r = t - G * g;
        if (G >= n_groups || r >= g_cnt[G]) {
            out_ids[t] = -1;
            out_dist[t] = 0x7F7FFFFFu;                    // FLT_MAX
        }
    }
    for (uint32_t G = lane; G < k; G += 64) {
        a.out_keys[q * k + G] = G < n_groups ? g_key[G] : 0;
        a.out_counts[q * k + G] = G < n_groups ? (int32_t)g_cnt[G] : 0;
    }
    if (lane == 0) a.out_complete[q] = (all_full || n_valid < C) ? 1 : 0;
}

// Enqueues the pass over n rows (n >= 1).
inline void group_rows(const GroupArgs& a, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(group_rows_kernel, dim3(n), dim3(64), group_lds_bytes(a.k, a.g), st, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
