// device_filter_ops.h — the filter algebra (cph_filters_combine): out[j] = a[j] OP b[j] for m allowed-id bitmaps in one
// launch, OP one of AND, OR, ANDNOT (a & ~b), XOR, NOT (~a, no b), and counts[j] = popcount(out[j]).
//
// The operands live wherever their filters were made (a cph_filter_create buffer, a view into a label-filter slab, an
// earlier combine output), so the kernel reads two tables of m device pointers; b is m entries, or ONE that every j
// reads (b_step = 0: many tenant bitmaps AND one common mask -- the mask stays in L2 after its first reader).  out[j] is
// out + j * stride.  Every operand base and `out + j * stride` is 16 B aligned: hipMalloc bases, and slabs whose stride
// is a multiple of 64 words (256 B); combine_tables checks the operands on the host before they go up.
//
// Grid (quads, filters).  A thread owns four consecutive words: one 16 B load per operand, one 16 B store -- a wave
// moves 1 KiB per instruction, the widest access there is -- and the thread behind the last full quad walks the
// nw % 4 words left over one by one.  The last word is masked to n_bits for every op (NOT is the one that sets tail bits,
// and dirty operands must not leak theirs); every word below nw is written, so nothing depends on what the slab held.
// The pointers a[j], b[j] are block-uniform loads.  Counting is tomb_block_add (device_tombstone.h): __popc per word,
// the wave's sum by __shfl_xor, the block's through LDS, ONE atomicAdd per block and filter; no thread returns before
// that barrier.  A pure streaming kernel: its floor is the bytes it moves, (2 or 3) m nw 4 B (broadcast b: 2 m nw 4 + nw 4).
// The host statement is host_index.h: filter_combine_host.
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "device_buf.h"
#include "device_tombstone.h"
#include "host_index.h"

namespace cph {

constexpr uint32_t kCombineBlock = kTombBlock;      // 256 threads = 256 quads = 1,024 words = 32,768 ids per block
constexpr uint32_t kCombineMaxY = 65535;            // filters per launch (grid.y); more: one launch per chunk

typedef uint32_t combine_u32x4 __attribute__((ext_vector_type(4)));      // four words = one 16 B load

__device__ __forceinline__ uint32_t combine_word(int op, uint32_t a, uint32_t b) {
    switch (op) {                                   // (op is kernel-uniform: a scalar branch)
        case kFilterAnd: return a & b;
        case kFilterOr: return a | b;
        case kFilterAndNot: return a & ~b;
        case kFilterXor: return a ^ b;
        default: return ~a;
    }
}

// a: [>= j0 + gridDim.y] pointers; b: the same, or one pointer (b_step = 0), or null for kFilterNot; filter j = j0 +
// blockIdx.y; counts zeroed by the launcher.  n_bits >= 1.
__global__ __launch_bounds__(kCombineBlock) void filter_combine_kernel(int op, const uint32_t* const* __restrict__ a,
                                                                       const uint32_t* const* __restrict__ b, uint32_t b_step,
                                                                       uint64_t n_bits, uint32_t j0, uint32_t* __restrict__ out,
                                                                       uint64_t stride, unsigned long long* __restrict__ counts) {
    const uint64_t j = (uint64_t)j0 + blockIdx.y;
    const uint64_t nw = (n_bits + 31) / 32, nq = nw / 4;
    const uint64_t q = (uint64_t)blockIdx.x * kCombineBlock + threadIdx.x;
    const uint32_t last = (n_bits & 31) ? (1u << (uint32_t)(n_bits & 31)) - 1u : 0xFFFFFFFFu;
    const uint32_t* __restrict__ pa = a[j];
    const uint32_t* __restrict__ pb = op == kFilterNot ? nullptr : b[j * b_step];
    uint32_t* __restrict__ po = out + j * stride;
    uint32_t c = 0;
    if (q < nq) {
        // (a pointer read from a table has no address space the compiler can see: say "global", or the loads are flat)
        const combine_u32x4 va = ((const __attribute__((address_space(1))) combine_u32x4*)pa)[q];
        combine_u32x4 vb = {0u, 0u, 0u, 0u};
        if (pb) vb = ((const __attribute__((address_space(1))) combine_u32x4*)pb)[q];
        uint4 r;
        r.x = combine_word(op, va.x, vb.x);
        r.y = combine_word(op, va.y, vb.y);
        r.z = combine_word(op, va.z, vb.z);
        r.w = combine_word(op, va.w, vb.w) & (4 * q + 3 == nw - 1 ? last : 0xFFFFFFFFu);
        reinterpret_cast<uint4*>(po)[q] = r;
        c = (uint32_t)(__popc(r.x) + __popc(r.y) + __popc(r.z) + __popc(r.w));
    } else if (q == nq) {                              // the nw % 4 words behind the last quad (none: the loop is empty)
        for (uint64_t w = 4 * nq; w < nw; ++w) {
            uint32_t x = combine_word(op, pa[w], pb ? pb[w] : 0u);
            if (w == nw - 1) x &= last;
            po[w] = x;
            c += (uint32_t)__popc(x);
        }
    }
    tomb_block_add(c, &counts[j]);
}

// The operand tables of one call, checked and sent up on `st`: tab = [a: m pointers | b: n_b pointers] (n_b = m, 1 or
// 0).  Every pointer must be 16 B aligned -- the kernel reads 16 B per lane from it.  The host arrays must stay valid
// until `st` has drained.
inline void combine_tables(const uint32_t* const* h_a, uint32_t m, const uint32_t* const* h_b, uint32_t n_b,
                           DevBuf<const uint32_t*>& tab, hipStream_t st) {
    for (uint32_t j = 0; j < m; ++j)
        if (!h_a[j] || (reinterpret_cast<uintptr_t>(h_a[j]) & 15u)) throw std::runtime_error("filter combine: operand bitmap is not 16 B aligned");
    for (uint32_t j = 0; j < n_b; ++j)
        if (!h_b[j] || (reinterpret_cast<uintptr_t>(h_b[j]) & 15u)) throw std::runtime_error("filter combine: operand bitmap is not 16 B aligned");
    tab.alloc((size_t)m + n_b);
    HIP_CHECK(hipMemcpyAsync(tab.p, h_a, (size_t)m * sizeof(*h_a), hipMemcpyHostToDevice, st));
    if (n_b) HIP_CHECK(hipMemcpyAsync(tab.p + m, h_b, (size_t)n_b * sizeof(*h_b), hipMemcpyHostToDevice, st));
}

// Enqueues the pass on `st` (counts zeroed first); every pointer lives on the current device.  d_a: m pointers; d_b: m,
// or one (b_broadcast), or null for kFilterNot; d_out: m bitmaps at `stride` words (stride % 4 == 0, stride >= nw, d_out
// 16 B aligned); m >= 1.
inline void filter_combine(int op, const uint32_t* const* d_a, const uint32_t* const* d_b, bool b_broadcast, uint64_t n_bits,
                           uint32_t m, uint32_t* d_out, uint64_t stride, unsigned long long* d_counts, hipStream_t st) {
    if (op < 0 || op >= kFilterOps) throw std::invalid_argument("filter combine: unknown op");
    const uint64_t nw = (n_bits + 31) / 32;
    if ((stride & 3u) || stride < nw || (reinterpret_cast<uintptr_t>(d_out) & 15u))
        throw std::runtime_error("filter combine: output slab is not 16 B aligned per bitmap");
    HIP_CHECK(hipMemsetAsync(d_counts, 0, (size_t)m * 8, st));
    if (n_bits == 0) return;
    const uint64_t threads = nw / 4 + (nw % 4 ? 1 : 0);
    const uint32_t gx = (uint32_t)((threads + kCombineBlock - 1) / kCombineBlock);
    for (uint32_t j0 = 0; j0 < m; j0 += kCombineMaxY) {
        const uint32_t gy = m - j0 < kCombineMaxY ? m - j0 : kCombineMaxY;
        hipLaunchKernelGGL(filter_combine_kernel, dim3(gx, gy), dim3(kCombineBlock), 0, st, op, d_a, d_b, b_broadcast ? 0u : 1u,
                           n_bits, j0, d_out, stride, d_counts);
        HIP_CHECK(hipGetLastError());
    }
}

}  // namespace cph
