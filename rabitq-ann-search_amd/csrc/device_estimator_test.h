// device_estimator_test.h — self-test hook for the N-bit estimator of the search kernels' expansion
// (device_search_expansion.inc: `estimate`): on real neighbour blocks of a loaded index it evaluates, for the same
// inputs, the path the expansion takes -- dqp_in_range, then lower_bounds_split + stage2_est_only with sqrt_in_range
// inside the range and the separate functions outside it -- and the separate functions alone (stage1_lower +
// stage2_est with __builtin_sqrtf: what the block hook and the streaming kernels run, compared bit for bit with the
// oracle), and returns both sets of bits.  The aux values of a block can be replaced by given ones, so that the edges of
// the arithmetic (ip_qo under the floor and under 1e-10, nop = 0, a cosine beyond +-1, a bound that rounds below 0)
// are reached at every distance, +inf included.  Test infrastructure (tests/test_gpu_estimator.py); not on the
// product path.
#pragma once
#include <hip/hip_runtime.h>

#include "device_fastscan.h"

namespace cph {

struct EstimatorTestArgs {
    const uint8_t* blocks;   // first block
    DevLayout L;
    const uint4* qmask;
    QP qp;
    const float* dqp;        // [n_dqp]
    const float* force;      // [n_sets][3] nop, ip_qo, ip_cp for every lane of the block ...
    const uint32_t* fmask;   // [n_sets] ... where bit 0 / 1 / 2 is set; the block's own value otherwise
    uint32_t n_dqp, n_sets;
    uint32_t* out;           // [block][set][dqp][6][32]: lo_stage1, lo_stage2, est of the expansion's path, then of the separate functions
};

template <int BW, int SD>
__global__ __launch_bounds__(64) void estimator_selftest_kernel(EstimatorTestArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    uint4* qm = reinterpret_cast<uint4*>(smem);
    const uint32_t PW = SD ? (SD >= 32 ? SD / 32 : 1) : a.L.PW;
    const int lane = threadIdx.x;
    for (uint32_t w = lane; w < PW; w += 64) qm[w] = qm_lds_word(a.qmask[w], nib_codes<BW, SD>(a.L));
    __syncthreads();
    if constexpr (BW >= 2) {
        LaneEst v0;
        load_block<BW, SD>(a.blocks + (size_t)blockIdx.x * a.L.stride, a.L, qm, lane, v0);
        const TailLanes tl = no_tail();
        const int i = lane & 31;
        const bool writer = (i < 16) ? (lane < 32) : (lane >= 32);   // both lane halves' copies are looked at
        for (uint32_t s = 0; s < a.n_sets; ++s) {
            LaneEst v = v0;
            const uint32_t m = a.fmask[s];
            if (m & 1u) v.nop = a.force[3 * s + 0];
            if (m & 2u) v.ip_qo = a.force[3 * s + 1];
            if (m & 4u) v.ip_cp = a.force[3 * s + 2];
            for (uint32_t j = 0; j < a.n_dqp; ++j) {
                const float dqp = a.dqp[j];
                float lo1, lo2, est, rlo2, rest;
                const float sq = __builtin_sqrtf(dqp);
                const float rlo1 = stage1_lower<BW>(a.qp, v, dqp, sq);
                stage2_est<BW>(a.qp, v, dqp, sq, rest, rlo2, tl);
                if (dqp_in_range(__builtin_amdgcn_readfirstlane(__float_as_uint(dqp)))) {
                    EstShared sh;
                    lower_bounds_split<BW>(a.qp, v, dqp, sqrt_in_range(dqp), lane, lo1, lo2, tl, sh);
                    est = stage2_est_only<BW>(a.qp, v, tl, sh);
                } else {
                    const float sq2 = sqrt_in_range(dqp);
                    lo1 = stage1_lower<BW>(a.qp, v, dqp, sq2);
                    stage2_est<BW>(a.qp, v, dqp, sq2, est, lo2, tl);
                }
                if (writer) {
                    uint32_t* o = a.out + ((((size_t)blockIdx.x * a.n_sets + s) * a.n_dqp + j) * 6) * 32 + i;
                    o[0] = __float_as_uint(lo1);
                    o[32] = __float_as_uint(lo2);
                    o[64] = __float_as_uint(est);
                    o[96] = __float_as_uint(rlo1);
                    o[128] = __float_as_uint(rlo2);
                    o[160] = __float_as_uint(rest);
                }
            }
        }
    }
}

}  // namespace cph
