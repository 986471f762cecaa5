// em2_wave.h -- what the lanes of one wave (64 lanes) do together, for every kernel that works a wave per row (device only).
#ifndef EM2_WAVE_H
#define EM2_WAVE_H

#include "em2_device.h"

namespace em2 {

// What one lane stored to LDS (or to memory only this workgroup touches) is what another lane of the wave loads next.
__device__ __forceinline__ void waveSync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// The same for arrays in global memory: what one lane stored must be what another lane of the wave loads next, and a
// lane's loads may not come from a line its L1 fetched before that store -- the agent-scope fence writes back and
// invalidates.
__device__ __forceinline__ void waveSyncGlobal()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");
    __builtin_amdgcn_wave_barrier();
}

// The lanes below this one that are set in a ballot mask: the lane's rank among the set lanes.
__device__ __forceinline__ uint32_t lanesBelow(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi(uint32_t(mask >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(mask), 0u));
}

// The sum of `value` over this lane and the lanes below it (blocks are one-dimensional and whole waves, as everywhere here).
__device__ __forceinline__ uint32_t waveInclusiveScan(uint32_t value)
{
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t step = 1u; step < 64u; step <<= 1) {
        const uint32_t below = uint32_t(__shfl_up(int(value), step, 64));
        if (lane >= step) value += below;
    }
    return value;
}

// The sum of `value` over the 64 lanes, in every lane, in one fixed order: lane l adds what lane l ^ 32 holds, then ^ 16,
// ... ^ 1 (both lanes of a pair add the same two numbers, so all lanes end with the same bits).
__device__ __forceinline__ double waveSum(double value)
{
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) value += __shfl_xor(value, step, 64);
    return value;
}

// The unused tail of a row's k result slots: the wave writes {0, 0.0f} into out[kept, k).
__device__ __forceinline__ void clearRowTail(PairOut* out, uint32_t kept, uint32_t k, uint32_t lane)
{
    for (uint32_t i = kept + lane; i < k; i += 64u) {
        PairOut zero;
        zero.cell = 0u;
        zero.similarity = 0.0f;
        out[i] = zero;
    }
}

}  // namespace em2

#endif
