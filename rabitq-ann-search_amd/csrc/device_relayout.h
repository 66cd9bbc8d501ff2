// device_relayout.h — converts the codes of 4-bit wide blocks between the plane-major storage layout and the
// neighbour-major nibble layout they are resident in (cph_core.h, `nib`).  Aux, ids and count are not touched.
//
// One wave per block, grid-stride: the block's codes (16 D bytes, at most 32 KiB) are copied into LDS, and every
// output dword is then built from LDS and written back in place.  Bandwidth-bound: one read and one
// write of the codes.  The host restatement is host_index.h: block_plane_to_nib / block_nib_to_plane.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cph_core.h"
#include "device_buf.h"

namespace cph {

template <bool TO_NIB>
__global__ __launch_bounds__(64) void relayout_kernel(uint8_t* blocks, uint64_t n_blocks, DevLayout L) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint4* s4 = reinterpret_cast<uint4*>(smem);
    const uint8_t* sb = smem;
    const int lane = threadIdx.x;
    const uint32_t chunks = L.codes_bytes / 16, dwords = L.codes_bytes / 4;
    const uint32_t NW = L.D / 8;   // nibble words per neighbour
    for (uint64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const uint4* in = reinterpret_cast<const uint4*>(blocks + b * L.stride);
        uint32_t* out = reinterpret_cast<uint32_t*>(blocks + b * L.stride);
        for (uint32_t j = lane; j < chunks; j += 64) s4[j] = in[j];
        __syncthreads();
        for (uint32_t o = lane; o < dwords; o += 64) {
            if constexpr (TO_NIB) {
                // output dword o = nibble word w of neighbour i (contiguous writes)
                const uint32_t i = o / NW, w = o % NW;
                uint32_t p[4];
#pragma unroll
                for (uint32_t pl = 0; pl < 4; ++pl)
                    p[pl] = *reinterpret_cast<const uint32_t*>(sb + plane_dword_offset(L, pl, w / 4, i));
                out[o] = nib_word_from_planes(p[0], p[1], p[2], p[3], w);
            } else {
                // output dword o = plane pl, 32-dim word pw of neighbour i (i fastest)
                const uint32_t i = o % 32, t = o / 32, pl = t / L.PW, pw = t % L.PW;
                const uint4 nw = *reinterpret_cast<const uint4*>(sb + ((size_t)i * NW + 4 * pw) * 4);
                out[plane_dword_offset(L, pl, pw, i) / 4] = plane_dword_from_nibs(nw.x, nw.y, nw.z, nw.w, pl);
            }
        }
        __syncthreads();
    }
}

// In place over n blocks in HBM (no-op unless L.nib), on the null stream.
inline void relayout_blocks(uint8_t* blocks, uint64_t n, const DevLayout& L, bool to_nib) {
    if (!L.nib || n == 0) return;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n, 1u << 16);
    if (to_nib) hipLaunchKernelGGL(relayout_kernel<true>, dim3(grid), dim3(64), L.codes_bytes, nullptr, blocks, n, L);
    else hipLaunchKernelGGL(relayout_kernel<false>, dim3(grid), dim3(64), L.codes_bytes, nullptr, blocks, n, L);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
}

// n resident blocks -> host, in the storage layout.  The resident copy is left as it is: nibble blocks go through
// a device staging buffer and are converted there.
inline void download_blocks(const uint8_t* blocks, uint64_t n, const DevLayout& L, uint8_t* host) {
    if (!L.nib) {
        HIP_CHECK(hipMemcpy(host, blocks, n * L.stride, hipMemcpyDeviceToHost));
        return;
    }
    const uint64_t chunk = std::max<uint64_t>(1, std::min<uint64_t>(n, (64u << 20) / L.stride));
    DevBuf<uint8_t> stage(chunk * L.stride);
    for (uint64_t base = 0; base < n; base += chunk) {
        const uint64_t c = std::min(chunk, n - base);
        HIP_CHECK(hipMemcpy(stage.p, blocks + base * L.stride, c * L.stride, hipMemcpyDeviceToDevice));
        relayout_blocks(stage.p, c, L, false);
        HIP_CHECK(hipMemcpy(host + base * L.stride, stage.p, c * L.stride, hipMemcpyDeviceToHost));
    }
}

}  // namespace cph
