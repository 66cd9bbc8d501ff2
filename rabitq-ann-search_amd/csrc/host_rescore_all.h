// host_rescore_all.h — how an exhaustive int8 rescoring call is cut (cph_search_rescored_all; device_rescore_i8_all.h holds
// the kernels): no HIP call, so the CPU tier reaches it through cph_host_plan_rescore_all.
//
// The scan's grid is (query tiles of kRescoreAllTile) x (P row parts); a part is a whole number of 128-row steps, so every
// 32-row block a wave owns starts at an id that is a multiple of 32 and one bitmap word masks it.  Per (part, query) the
// scan keeps a pool of C = 2 Kp sort words in scratch, P x tile_q x C x 8 bytes per launch.  Kp = max(128, pow2(k)), not the 64 of
// the exact scan: a step hands a query up to 128 words at once, and a pool cut to k <= Kp must take them (C - 128 >= k).
//     P        about one workgroup per CU over all query tiles of a launch (a workgroup holds 72 KiB of query planes in
//              LDS, one fits a CU), at most kRescoreAllMaxParts: the select kernel folds one list per part and query
//     tile_q   queries per launch: the whole batch, or -- scratch above the budget -- whole query tiles, halved until it fits;
//              a budget below one tile's pools at P = 1 is exceeded by exactly that much
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace cph {

constexpr uint32_t kRescoreAllTile = 128;           // queries per workgroup, rows per step
constexpr uint32_t kRescoreAllMaxK = 1024;
constexpr uint32_t kRescoreAllMaxParts = 256;
constexpr uint32_t kRescoreAllChunk = 128;          // bytes of K staged per LDS buffer once the planes do not fit whole
constexpr uint32_t kRescoreAllResident = 256;       // K_pad up to this: the planes of a tile stay in LDS for the whole part

// Bytes of one query plane row: the stored row rounded up to 32 (one MFMA k-step), and to whole chunks once chunked.
inline uint32_t rescore_all_kpad(uint32_t row_bytes) {
    const uint32_t k32 = (row_bytes + 31u) / 32u * 32u;
    return k32 <= kRescoreAllResident ? k32 : (k32 + kRescoreAllChunk - 1u) / kRescoreAllChunk * kRescoreAllChunk;
}

struct RescoreAllPlan {
    uint32_t Kp, C;        // pool geometry
    uint32_t P;            // row parts
    uint64_t part;         // rows per part, a multiple of 128
    uint32_t tile_q;       // queries per launch (a multiple of 128 unless it is the whole batch)
    uint64_t pool_keys;    // P * tile_q * C
};

// parts: a forced part count (the test hook), 0: the plan decides.
inline RescoreAllPlan plan_rescore_all(uint64_t size, uint64_t n, uint32_t k, int num_cus, uint64_t scratch_bytes, uint32_t parts = 0) {
    RescoreAllPlan pl{};
    pl.Kp = kRescoreAllTile;
    while (pl.Kp < k) pl.Kp <<= 1;
    pl.C = 2 * pl.Kp;
    const uint64_t blocks = std::max<uint64_t>(1, (size + kRescoreAllTile - 1) / kRescoreAllTile);
    auto cut = [&](uint64_t want) {
        want = std::max<uint64_t>(1, std::min<uint64_t>({want, blocks, (uint64_t)kRescoreAllMaxParts}));
        pl.part = (blocks + want - 1) / want * kRescoreAllTile;
        pl.P = (uint32_t)std::max<uint64_t>(1, (size + pl.part - 1) / pl.part);
        pl.pool_keys = (uint64_t)pl.P * pl.tile_q * pl.C;
    };
    pl.tile_q = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, 65535ull * kRescoreAllTile));     // (tiles of a launch: the grid's x)
    for (;;) {
        const uint64_t tiles = (pl.tile_q + kRescoreAllTile - 1) / kRescoreAllTile;
        cut(parts ? parts : ((uint64_t)std::max(1, num_cus) + tiles - 1) / tiles);
        if (pl.pool_keys * 8 <= scratch_bytes || pl.tile_q <= kRescoreAllTile) break;
        pl.tile_q = std::max<uint32_t>(kRescoreAllTile, (pl.tile_q / 2 + kRescoreAllTile - 1) / kRescoreAllTile * kRescoreAllTile);
    }
    if (!parts && pl.pool_keys * 8 > scratch_bytes) cut(scratch_bytes / ((uint64_t)pl.tile_q * pl.C * 8));
    return pl;
}

}  // namespace cph
