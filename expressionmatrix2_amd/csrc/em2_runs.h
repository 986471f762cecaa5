// em2_runs.h -- runs of equal keys in a sorted array of 64-bit keys (device code): the flag at the head of every run, and the
// tables findSimilarPairs5 and findSimilarPairs7 build from the runs of their (slice or table, bucket) keys; with them the bit
// window of a signature both cut their keys from.  The kernels have internal linkage: every object that includes this has its own.
#ifndef EM2_RUNS_H
#define EM2_RUNS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace em2 {
namespace {

// Bits [slice * length, (slice + 1) * length) of a signature, counted from the most significant bit of word 0; length in [1, 64].
__device__ __forceinline__ uint64_t sliceValue64(const uint64_t* sig, uint32_t slice, uint32_t length)
{
    const uint32_t b0 = slice * length;
    const uint32_t w = b0 >> 6;
    const uint32_t o = b0 & 63u;
    uint64_t window = sig[w] << o;
    if (o + length > 64u) window |= sig[w + 1] >> (64u - o);
    return window >> (64u - length);
}

// flags[i] = 1 where a run of equal keys begins.
__global__ void __launch_bounds__(256)
headFlagsKernel(const uint64_t* __restrict__ sorted, uint64_t n, uint32_t* __restrict__ flags)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        flags[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1u : 0u;
    }
}

// runIndex[i] = (inclusive scan of flags)[i] - 1.  Records where each run starts (with total as the end of the last one) and
// which run every (table, cell) belongs to, the table being the key's bits from KeyShift up.  CellMajor: the run table is
// [cell][table] (a cell's descriptors are one contiguous read), else [table][cell]; each reads only the count it strides by.
template <uint32_t KeyShift, bool CellMajor>
__global__ void __launch_bounds__(256)
runTablesKernel(const uint64_t* __restrict__ sortedKeys, const uint32_t* __restrict__ sortedCells,
                const uint32_t* __restrict__ flags, const uint32_t* __restrict__ scan, uint64_t total,
                uint32_t cellCount, uint32_t tableCount, uint32_t* __restrict__ runStart, uint32_t* __restrict__ runOf)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t run = scan[i] - 1u;
        if (flags[i]) runStart[run] = uint32_t(i);
        const uint32_t t = uint32_t(sortedKeys[i] >> KeyShift);
        if (CellMajor) runOf[size_t(sortedCells[i]) * tableCount + t] = run;
        else runOf[size_t(t) * cellCount + sortedCells[i]] = run;
        if (i == total - 1) runStart[run + 1u] = uint32_t(total);
    }
}

}  // namespace
}  // namespace em2

#endif
