// device_maxsim.h — multi-vector (late-interaction, MaxSim) search (cph_search_maxsim*): the k best keys of a query of T
// token rows by the sum, over the live tokens, of each token's best row of the key.
//
// The statement is host_maxsim.h's.  maxsim_rows_kernel runs one 256-thread workgroup per query, over the E = L * C entries
// of the query's live rows and P = the power of two >= max(E, 64):
//   load     an entry (t, j) that is valid becomes the 64-bit word  (key ^ 0x80000000) << 32 | t << 16 | j ; everything else
//            (padding, ids >= n_ids, the tail up to P) the all-ones word, which no entry has.  A wave reads 64 consecutive
//            entries of a row; key_of[id] is gathered once per entry.  The last valid position of every row goes to LDS
//            with one atomicMax per run of valid entries (one per row when the padding is at the end): floor_t.
//   sort     bitonic, ascending, in LDS.  A segment of equal high halves is a key; inside it the low halves ascend, so the
//            tokens come in order and the first entry of every (key, token) run is pos_t(key).
//   compact  segment heads and run heads by neighbour compares; every wave counts the heads of its quarter with ballots,
//            the four totals give the offsets, a second walk writes the run heads (position, token, distance) and, for
//            every segment, the index of its first run head.  Two short arrays replace the sorted words from here on.
//   score    one lane per segment walks the tokens 0 .. L - 1 and its at most L run heads and forms the sequential float32
//            sum, floor_t where the key has no run; it writes orderable(score) << 32 | segment over the sorted words.
//            (One lane per segment over RAW entries would walk 8,192 of them when a query's candidates share one key.)
//   select   the same bitonic sort over the power of two >= the number of segments.  Segments are in key order already, so
//            this orders by (score, key); orderable() is the usual sign flip (a distance can be slightly negative).
//   write    the first min(k, segments) words are the answer: key, score, hits per slot, and rows [k][T] with one
//            thread per (slot, token), which finds its run head by bisection over the segment's tokens.  Every output
//            slot is written here, padding included; nothing depends on a memset.
// LDS (maxsim_lds_bytes, sized by the actual power of two): 17 bytes per element of P plus 580: 1.6 KiB at P = 64,
// 35 KiB at P = 2,048 (T = 32, C = 64), 137 KiB at P = 8,192, which leaves one workgroup per CU.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "device_buf.h"
#include "device_wg_primitives.h"
#include "host_maxsim.h"

namespace cph {

struct MaxsimArgs {
    const int64_t* ids;                   // [n][T][C] candidate rows: internal ids, -1 = padding
    const float* dist;                    // [n][T][C]
    const int32_t* n_tokens;              // [n] live tokens of every query (clamped to [1, T] here), or null: T
    uint32_t T, C, k;                     // T <= kMaxsimMaxTokens, C <= kMaxsimMaxCandidates, T * C <= kMaxsimMaxEntries
    const int32_t* key_of;                // [n_ids]
    uint32_t n_ids;                       // ids at or above this are treated as padding (no search returns one)
    const uint32_t* rows;                 // [n_ids] row map, or null: ids are written as they are
    int32_t* out_keys;                    // [n][k]
    float* out_score;                     // [n][k]
    int32_t* out_hits;                    // [n][k]
    int64_t* out_rows;                    // [n][k][T], or null: not written
    int32_t* out_found;                   // [n]
};

constexpr uint32_t kMaxsimThreads = kWgSortThreads;

// words u64 [P] | run distance f32 [P] | run position u16 [P] | segment's first run u16 [P + 2] | run token u8 [P] |
// floors f32 [64] | last valid position i32 [64] | counters u32 [16]
inline size_t maxsim_lds_bytes(uint32_t T, uint32_t C) {
    const size_t P = wg_sort_len(T * C);
    return P * 8 + P * 4 + P * 2 + (P + 2) * 2 + P + 64 * 4 + 64 * 4 + 16 * 4;
}

// Grid n, kMaxsimThreads threads; LDS: maxsim_lds_bytes(T, C).
__global__ __launch_bounds__(kMaxsimThreads) void maxsim_rows_kernel(MaxsimArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    const uint32_t T = a.T, C = a.C, k = a.k, Pmax = wg_sort_len(T * C);
    unsigned long long* w = reinterpret_cast<unsigned long long*>(smem);
    float* rd = reinterpret_cast<float*>(w + Pmax);
    uint16_t* rh = reinterpret_cast<uint16_t*>(rd + Pmax);
    uint16_t* sf = rh + Pmax;
    uint8_t* rt = reinterpret_cast<uint8_t*>(sf + Pmax + 2);
    float* fl = reinterpret_cast<float*>(rt + Pmax);
    int* last = reinterpret_cast<int*>(fl + 64);
    uint32_t* cnt = reinterpret_cast<uint32_t*>(last + 64);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t q = blockIdx.x;
    const int64_t* __restrict__ qi = a.ids + q * T * C;
    const float* __restrict__ qd = a.dist + q * T * C;
    uint32_t L = T;
    if (a.n_tokens) {
        const int32_t l = a.n_tokens[q];
        L = l < 1 ? 1u : ((uint32_t)l > T ? T : (uint32_t)l);
    }
    const uint32_t E = L * C, P = wg_sort_len(E);

    // load
    if (tid < 64) last[tid] = -1;
    __syncthreads();
    for (uint32_t e = tid; e < P; e += kMaxsimThreads) {
        unsigned long long word = kSortNone;
        if (e < E) {
            const int64_t id = qi[e];
            if (id >= 0 && (unsigned long long)id < a.n_ids) {
                const uint32_t t = e / C, j = e - t * C;
                bool next_valid = false;
                if (j + 1 < C) {
                    const int64_t nx = qi[e + 1];
                    next_valid = nx >= 0 && (unsigned long long)nx < a.n_ids;
                }
                if (!next_valid) atomicMax(&last[t], (int)j);
                const uint32_t key = (uint32_t)a.key_of[id] ^ 0x80000000u;
                word = ((unsigned long long)key << 32) | (t << 16) | j;
            }
        }
        w[e] = word;
    }
    __syncthreads();
    if (tid < L) fl[tid] = last[tid] >= 0 ? qd[tid * C + (uint32_t)last[tid]] : 0.0f;

    wg_sort(w, P, tid);

    // compact: wave v owns [v * span, (v + 1) * span) of the sorted words
    const uint32_t span = P / 4 < 64 ? 64 : P / 4;
    const uint32_t w_lo = wave * span < P ? wave * span : P, w_hi = w_lo + span < P ? w_lo + span : P;
    const unsigned long long below = (1ull << lane) - 1;
    uint32_t runs = 0, segs = 0;
    for (uint32_t base = w_lo; base < w_hi; base += 64) {
        const uint32_t i = base + lane;
        const unsigned long long x = w[i], pv = i ? w[i - 1] : kSortNone;
        const bool valid = x != kSortNone;
        const bool seg = valid && (i == 0 || (uint32_t)(pv >> 32) != (uint32_t)(x >> 32));
        const bool run = valid && (seg || ((uint32_t)pv >> 16) != ((uint32_t)x >> 16));
        runs += (uint32_t)__popcll(__ballot(run));
        segs += (uint32_t)__popcll(__ballot(seg));
    }
    if (lane == 0) {
        cnt[wave] = runs;
        cnt[4 + wave] = segs;
    }
    __syncthreads();
    uint32_t r0 = 0, s0 = 0;
    for (uint32_t v = 0; v < wave; ++v) {
        r0 += cnt[v];
        s0 += cnt[4 + v];
    }
    const uint32_t n_runs = cnt[0] + cnt[1] + cnt[2] + cnt[3], n_segs = cnt[4] + cnt[5] + cnt[6] + cnt[7];
    for (uint32_t base = w_lo; base < w_hi; base += 64) {
        const uint32_t i = base + lane;
        const unsigned long long x = w[i], pv = i ? w[i - 1] : kSortNone;
        const bool valid = x != kSortNone;
        const bool seg = valid && (i == 0 || (uint32_t)(pv >> 32) != (uint32_t)(x >> 32));
        const bool run = valid && (seg || ((uint32_t)pv >> 16) != ((uint32_t)x >> 16));
        const unsigned long long run_m = __ballot(run), seg_m = __ballot(seg);
        if (run) {
            const uint32_t r = r0 + (uint32_t)__popcll(run_m & below);
            const uint32_t t = ((uint32_t)x >> 16) & 0xFFu, pos = t * C + ((uint32_t)x & 0xFFFFu);
            rh[r] = (uint16_t)pos;
            rt[r] = (uint8_t)t;
            rd[r] = qd[pos];
            if (seg) sf[s0 + (uint32_t)__popcll(seg_m & below)] = (uint16_t)r;
        }
        r0 += (uint32_t)__popcll(run_m);
        s0 += (uint32_t)__popcll(seg_m);
    }
    if (tid == 0) sf[n_segs] = (uint16_t)n_runs;
    __syncthreads();                                      // (also: nobody reads the sorted words any more)

    // score
    const uint32_t P2 = wg_sort_len(n_segs);
    for (uint32_t s = tid; s < P2; s += kMaxsimThreads) {
        unsigned long long word = kSortNone;
        if (s < n_segs) {
            uint32_t r = sf[s];
            const uint32_t r_end = sf[s + 1];
            float sum = 0.0f;
            for (uint32_t t = 0; t < L; ++t) {
                float term = fl[t];
                if (r < r_end && rt[r] == t) term = rd[r++];
                sum = __fadd_rn(sum, term);
            }
            word = ((unsigned long long)orderable(sum) << 32) | s;
        }
        w[s] = word;
    }
    __syncthreads();

    // select
    wg_sort(w, P2, tid);

    // write
    const uint32_t found = k < n_segs ? k : n_segs;
    if (tid == 0) a.out_found[q] = (int32_t)found;
    for (uint32_t o = tid; o < k; o += kMaxsimThreads) {
        int32_t key = 0, hits = 0;
        uint32_t score = 0x7F7FFFFFu;                     // FLT_MAX
        if (o < found) {
            const unsigned long long x = w[o];
            const uint32_t s = (uint32_t)x, r = sf[s];
            key = a.key_of[qi[rh[r]]];
            hits = (int32_t)(sf[s + 1] - r);
            score = __float_as_uint(from_orderable((uint32_t)(x >> 32)));
        }
        a.out_keys[q * k + o] = key;
        reinterpret_cast<uint32_t*>(a.out_score)[q * k + o] = score;
        a.out_hits[q * k + o] = hits;
    }
    if (!a.out_rows) return;                              // (the rescored search keeps keys and scores only)
    int64_t* __restrict__ out_rows = a.out_rows + q * k * T;
    for (uint32_t idx = tid; idx < k * T; idx += kMaxsimThreads) {
        const uint32_t o = idx / T, t = idx - o * T;
        int64_t val = -1;
        if (o < found && t < L) {
            const uint32_t s = (uint32_t)w[o];
            uint32_t lo = sf[s], hi = sf[s + 1];
            const uint32_t r_end = hi;
            while (lo < hi) {                             // the first run of the segment whose token is >= t
                const uint32_t mid = (lo + hi) >> 1;
                if (rt[mid] < t) lo = mid + 1;
                else hi = mid;
            }
            if (lo < r_end && rt[lo] == t) {
                const int64_t id = qi[rh[lo]];
                val = a.rows ? (int64_t)a.rows[id] : id;
            }
        }
        out_rows[idx] = val;
    }
}

// Enqueues the pass over n queries (n >= 1) on `device`, the current device.  A query of more than 2,048 entries needs
// more dynamic LDS than a plain launch accepts: the function's limit is raised to the largest shape's, once per device.
inline void maxsim_rows(const MaxsimArgs& a, uint32_t n, int device, hipStream_t st) {
    static std::atomic<bool> raised[64];
    const size_t lds = maxsim_lds_bytes(a.T, a.C);
    if (lds > 48 * 1024 && !(device >= 0 && device < 64 && raised[device].load())) {
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&maxsim_rows_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)maxsim_lds_bytes(kMaxsimMaxTokens, kMaxsimMaxEntries / kMaxsimMaxTokens)));
        if (device >= 0 && device < 64) raised[device].store(true);
    }
    hipLaunchKernelGGL(maxsim_rows_kernel, dim3(n), dim3(kMaxsimThreads), lds, st, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cph
