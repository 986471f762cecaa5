// em2_rank_genes.hip -- rank-sum (Mann-Whitney / Wilcoxon) marker genes: for every gene of a subset's CSR in device memory and
// every group of cells, the integers of the test "the group against the rest" (include/em2_lsh.h states the
// definition).  The reference has no such test.  All groups share one universe, so one sort serves them all:
//   * groupSizesKernel      an integer histogram of `group` (in LDS where groupCount fits, flushed with global atomics); a group
//                           id that is neither below groupCount nor kNoGroup raises an error word;
//   * entriesKernel         a wave per cell: key = gene << 32 | ordered(bits of count * float(normInverse)), payload = the cell's
//                           group; ordered() maps -0 to +0, then flips the sign bit of a non-negative value and all bits of a
//                           negative one, so that unsigned order is the order of the floats.  The input checks of the gene
//                           information's entriesKernel in its error words; NaN raises a word of its own;
//   * the radix sort of (key, group) on the bits in use, 32 + the bits of geneCount - 1.  Its stability is not relied upon:
//     equal keys are one tie group, and what is added for its members does not depend on their order;
//   * geneSearchesKernel    a thread per gene, three binary searches: the gene's segment, the first key >= ordered(+0) and the
//                           first key > ordered(+0).  They give neg and the stored zeros without atomics;
//   * headFlagsKernel (em2_runs.h), an inclusive scan and runStartsKernel: every entry knows its run's [a, b);
//   * a scan over the genes' chunk counts and chunkTableKernel (em2_chunks.h): a gene's segment is cut at multiples of the chunk
//     FROM ITS OWN START, so a gene present in every cell and a gene present in one keep the machine equally busy;
//   * accumulateKernel<LDS> a workgroup per chunk.  Every entry that is not zero adds twice its mid-rank and a 1 to its group's
//                           counters: in LDS (64-bit and 32-bit LDS atomics, flushed with global atomics for the counters that
//                           are not zero) where groupCount fits, straight to global memory where it does not.  The head of a
//                           run adds t^3 - t to the gene's tieSum.  No lane walks a run;
//   * finishKernel          a thread per (gene, group) adds the zeros' share (n_k - nonZeroCount) (2 neg + t0 + 1); a thread per
//                           gene adds t0^3 - t0; the group sizes go out.
// Integer atomics only: no sum has an order, and the result is a function of the input alone, equal bit for bit to the
// one-thread restatement of the tests.  The statistics (z, auc) are host arithmetic on the integers (em2_rank_genes_host.h).

#include "em2_device.h"
#include "em2_expression.h"
#include "em2_entry.h"
#include "em2_csr.h"
#include "em2_chunks.h"
#include "em2_runs.h"
#include "em2_primitives.h"
#include "em2_rank_genes_host.h"

#include <atomic>
#include <cstring>
#include <string>

namespace em2 {
namespace {

constexpr uint32_t kDefaultMaxBlocks = 16384u;
constexpr uint32_t kDefaultChunk = 2048u;                  // entries of a gene one workgroup accumulates
constexpr uint32_t kMaxLdsGroups = 4096u;                  // 12 bytes of LDS per group: 48 KiB
constexpr uint32_t kOrderedZero = 0x80000000u;             // ordered(+0)

constexpr uint32_t kBadValue = 8u, kBadGroup = 16u;        // bits of *inputError next to entriesKernel's 1, 2, 4

std::atomic<uint32_t> testMaxBlocks{0}, testChunk{0}, testLdsGroups{0};

uint32_t chunkEntries() { return testChunk.load() ? testChunk.load() : kDefaultChunk; }

uint32_t ldsGroupLimit()
{
    const uint32_t asked = testLdsGroups.load();
    return asked && asked < kMaxLdsGroups ? asked : kMaxLdsGroups;
}

// Blocks for `items` items at perBlock a block, at least 1 and at most the limit: every kernel here strides over its grid.
uint32_t blocksFor(uint64_t items, uint32_t perBlock)
{
    const uint64_t blocks = (items + perBlock - 1u) / perBlock;
    const uint32_t asked = testMaxBlocks.load();
    const uint32_t most = asked ? asked : kDefaultMaxBlocks;
    return uint32_t(blocks > most ? most : (blocks ? blocks : 1u));
}

__device__ __forceinline__ void add64(uint64_t* to, uint64_t value)
{
    atomicAdd(reinterpret_cast<unsigned long long*>(to), static_cast<unsigned long long>(value));
}

// sizes[k] = the cells of group k.  LDS: the block counts in counts[groupCount] of dynamic LDS first.
template <bool LDS>
__global__ void __launch_bounds__(256)
groupSizesKernel(const uint32_t* __restrict__ group, uint32_t cellCount, uint32_t groupCount, uint32_t* __restrict__ sizes,
                 uint32_t* __restrict__ words)
{
    extern __shared__ uint64_t lds[];
    uint32_t* counts = reinterpret_cast<uint32_t*>(lds);
    if (LDS) {
        for (uint32_t k = threadIdx.x; k < groupCount; k += blockDim.x) counts[k] = 0u;
        __syncthreads();
    }
    bool bad = false;
    for (uint64_t c = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; c < cellCount; c += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t k = group[c];
        if (k == kNoGroup) continue;
        if (k >= groupCount) bad = true;
        else atomicAdd(LDS ? counts + k : sizes + k, 1u);
    }
    if (bad) atomicOr(words + 2, 1u);
    if (LDS) {
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < groupCount; k += blockDim.x) {
            if (counts[k]) atomicAdd(sizes + k, counts[k]);
        }
    }
}

__device__ __forceinline__ uint32_t orderedBits(float value)
{
    const uint32_t bits = value == 0.f ? 0u : __float_as_uint(value);          // -0 counts as +0
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// words[0] |= the input error of the gene information's entriesKernel (1: a gene id is not below geneCount, 2: the gene ids of a
// cell do not ascend strictly, 4: toc does not cover exactly the entryCount entries, from 0 and ascending; such a cell writes
// nothing), words[1] |= 1 where a value is NaN.  normInverse NULL: no scaling.
__global__ void __launch_bounds__(256)
entriesKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint32_t cellCount, uint32_t geneCount,
              uint64_t entryCount, const double* __restrict__ normInverse, const uint32_t* __restrict__ group,
              uint64_t* __restrict__ keys, uint32_t* __restrict__ groups, uint32_t* __restrict__ words)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = uint64_t(gridDim.x) * (blockDim.x >> 6);
    uint32_t bad = 0u;
    bool notANumber = false;
    if (blockIdx.x == 0u && threadIdx.x == 0u && (toc[0] != 0u || toc[cellCount] != entryCount)) bad |= 4u;
    for (uint64_t cell = uint64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); cell < cellCount; cell += waves) {
        const uint64_t begin = toc[cell];
        uint64_t end = toc[cell + 1u];
        if (end > entryCount || begin > end) {                 // (a toc that descends: cells would write each other's entries)
            bad |= 4u;
            end = begin;
        }
        const float factor = normInverse ? float(normInverse[cell]) : 1.f;
        const uint32_t mine = group[cell];
        for (uint64_t p = begin + lane; p < end; p += 64u) {
            const CountIn e = data[p];
            if (e.gene >= geneCount) bad |= 1u;
            if (p != begin && e.gene <= data[p - 1u].gene) bad |= 2u;
            const float value = normInverse ? e.count * factor : e.count;
            if (value != value) notANumber = true;
            keys[p] = uint64_t(e.gene) << 32 | orderedBits(value);
            groups[p] = mine;
        }
    }
    if (bad) atomicOr(words, bad);
    if (notANumber) atomicOr(words + 1, 1u);
}

__device__ __forceinline__ uint64_t lowerBound(const uint64_t* __restrict__ sorted, uint64_t count, uint64_t key)
{
    uint64_t low = 0, high = count;
    while (low < high) {
        const uint64_t middle = low + (high - low) / 2u;
        if (sorted[middle] < key) low = middle + 1u;
        else high = middle;
    }
    return low;
}

// offsets[g] = the first entry of gene g in the sorted stream (offsets[geneCount] = count), zeroBegin[g] / zeroEnd[g] = the
// first entry of the gene that is >= 0 / > 0, chunkCounts[g] = its chunks (chunkCounts[geneCount] = 0, the scan's last input).
__global__ void __launch_bounds__(256)
geneSearchesKernel(const uint64_t* __restrict__ sortedKeys, uint64_t count, uint32_t geneCount, uint32_t chunk,
                   uint64_t* __restrict__ offsets, uint64_t* __restrict__ zeroBegin, uint64_t* __restrict__ zeroEnd,
                   uint64_t* __restrict__ chunkCounts)
{
    for (uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; g <= geneCount; g += uint64_t(gridDim.x) * blockDim.x) {
        if (g == geneCount) {
            offsets[g] = count;
            chunkCounts[g] = 0u;
            continue;
        }
        const uint64_t begin = lowerBound(sortedKeys, count, g << 32);
        const uint64_t end = lowerBound(sortedKeys, count, (g + 1u) << 32);
        offsets[g] = begin;
        zeroBegin[g] = lowerBound(sortedKeys, count, g << 32 | kOrderedZero);
        zeroEnd[g] = lowerBound(sortedKeys, count, (g << 32 | kOrderedZero) + 1u);
        chunkCounts[g] = (end - begin + chunk - 1u) / chunk;
    }
}

// runNumber: the inclusive scan of the head flags.  runStart[r] = the first entry of run r, runStart[runs] = count.
__global__ void __launch_bounds__(256)
runStartsKernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ runNumber, uint64_t count, uint32_t* __restrict__ runStart)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += uint64_t(gridDim.x) * blockDim.x) {
        if (flags[i]) runStart[runNumber[i] - 1u] = uint32_t(i);
        if (i == count - 1u) runStart[runNumber[i]] = uint32_t(count);
    }
}

// The chunks t = block, block + blocks, ...: every entry of the chunk that is not zero adds twice its mid-rank and a 1 to the
// counters of its group, the head of its run t^3 - t to the gene's tieSum.  LDS: sums[groupCount] (64 bits) and
// counts[groupCount] in dynamic LDS, zero between chunks, flushed where not zero.
template <bool LDS>
__global__ void __launch_bounds__(256)
accumulateKernel(const uint32_t* __restrict__ sortedGroups, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ runNumber,
                 const uint32_t* __restrict__ runStart, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ zeroBegin,
                 const uint64_t* __restrict__ zeroEnd, const uint64_t* __restrict__ chunkStarts, const ChunkRef* __restrict__ table,
                 uint32_t cellCount, uint32_t geneCount, uint32_t groupCount, uint32_t chunkSize, uint32_t* __restrict__ nonZeroCount,
                 uint64_t* __restrict__ rankSum2, uint64_t* __restrict__ tieSum)
{
    extern __shared__ uint64_t lds[];
    uint64_t* sums = lds;
    uint32_t* counts = reinterpret_cast<uint32_t*>(lds + groupCount);
    if (LDS) {
        for (uint32_t k = threadIdx.x; k < groupCount; k += blockDim.x) {
            sums[k] = 0u;
            counts[k] = 0u;
        }
        __syncthreads();
    }
    const uint64_t total = chunkStarts[geneCount];
    for (uint64_t t = blockIdx.x; t < total; t += gridDim.x) {
        const ChunkRef chunk = table[t];
        const uint64_t segment = offsets[chunk.gene], segmentEnd = offsets[chunk.gene + 1u];
        const uint64_t begin = segment + uint64_t(chunk.index) * chunkSize;
        const uint64_t end = begin + chunkSize < segmentEnd ? begin + chunkSize : segmentEnd;
        const uint64_t firstZero = zeroBegin[chunk.gene], firstPositive = zeroEnd[chunk.gene];
        const uint64_t absent2 = 2u * (uint64_t(cellCount) - (segmentEnd - segment));        // 2 z: the positives rank above them
        const size_t row = size_t(chunk.gene) * groupCount;
        for (uint64_t p = begin + threadIdx.x; p < end; p += blockDim.x) {
            if (p >= firstZero && p < firstPositive) continue;                                // a stored zero: finishKernel's
            const uint32_t run = runNumber[p] - 1u;
            const uint64_t a = runStart[run] - segment, b = runStart[run + 1u] - segment;
            const uint64_t twice = a + b + 1u + (p >= firstPositive ? absent2 : 0u);
            const uint32_t k = sortedGroups[p];
            if (k != kNoGroup) {
                if (LDS) {
                    add64(sums + k, twice);
                    atomicAdd(counts + k, 1u);
                } else {
                    add64(rankSum2 + row + k, twice);
                    atomicAdd(nonZeroCount + row + k, 1u);
                }
            }
            const uint64_t ties = b - a;
            if (flags[p] && ties > 1u) add64(tieSum + chunk.gene, ties * ties * ties - ties);
        }
        if (LDS) {
            __syncthreads();
            for (uint32_t k = threadIdx.x; k < groupCount; k += blockDim.x) {
                if (counts[k]) {
                    add64(rankSum2 + row + k, sums[k]);
                    atomicAdd(nonZeroCount + row + k, counts[k]);
                    sums[k] = 0u;
                    counts[k] = 0u;
                }
            }
            __syncthreads();
        }
    }
}

// The zeros, stored or not, are one tie group of t0 = N - (the gene's entries that are not zero) values above the neg negative
// ones: twice their mid-rank is 2 neg + t0 + 1.  A thread per (gene, group) adds it for the group's cells without a nonzero
// entry; a thread per gene adds t0^3 - t0; a thread per group writes its size.
__global__ void __launch_bounds__(256)
finishKernel(const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ zeroBegin, const uint64_t* __restrict__ zeroEnd,
             const uint32_t* __restrict__ sizes, uint32_t cellCount, uint32_t geneCount, uint32_t groupCount,
             const uint32_t* __restrict__ nonZeroCount, uint64_t* __restrict__ rankSum2, uint64_t* __restrict__ tieSum,
             uint32_t* __restrict__ groupSize)
{
    const uint64_t first = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x, stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = first; i < uint64_t(geneCount) * groupCount; i += stride) {
        const uint64_t g = i / groupCount, k = i - g * groupCount;
        const uint64_t negative = zeroBegin[g] - offsets[g];
        const uint64_t zeros = cellCount - ((offsets[g + 1u] - offsets[g]) - (zeroEnd[g] - zeroBegin[g]));
        rankSum2[i] += (uint64_t(sizes[k]) - nonZeroCount[i]) * (2u * negative + zeros + 1u);
    }
    for (uint64_t g = first; g < geneCount; g += stride) {
        const uint64_t zeros = cellCount - ((offsets[g + 1u] - offsets[g]) - (zeroEnd[g] - zeroBegin[g]));
        tieSum[g] += zeros * zeros * zeros - zeros;
    }
    for (uint64_t k = first; k < groupCount; k += stride) groupSize[k] = sizes[k];
}

uint32_t geneBitsOf(uint32_t geneCount)
{
    uint32_t bits = 0;
    while (bits < 32u && (1ull << bits) < geneCount) ++bits;
    return bits;
}

// Chunks of the whole problem at most: a gene wastes less than one.
uint64_t chunkBound(uint64_t entryCount, uint32_t geneCount, uint32_t chunk) { return entryCount / chunk + geneCount; }

// After the sort the alternate key buffer holds the head flags and the run numbers, the alternate group buffer the run starts.
struct Layout {
    size_t words, sizes, keysA, keysB, groupsA, groupsB, offsets, zeroBegin, zeroEnd, chunkCounts, chunkStarts, table, sortTemp, scanTemp,
        runScanTemp, total;
    size_t sortTempBytes, scanTempBytes, runScanTempBytes;
    uint32_t chunk;
};

hipError_t layoutOf(uint64_t entryCount, uint32_t geneCount, uint32_t groupCount, Layout& l)
{
    ArenaPlan plan;
    const size_t perGene = (size_t(geneCount) + 1u) * sizeof(uint64_t);
    l.chunk = chunkEntries();
    l.words = plan.take(256);
    l.sizes = plan.takeFor<uint32_t>(groupCount);
    l.keysA = plan.takeFor<uint64_t>(entryCount);
    l.keysB = plan.takeFor<uint64_t>(entryCount);
    l.groupsA = plan.takeFor<uint32_t>(entryCount + 1u);
    l.groupsB = plan.takeFor<uint32_t>(entryCount + 1u);
    l.offsets = plan.take(perGene);
    l.zeroBegin = plan.take(perGene);
    l.zeroEnd = plan.take(perGene);
    l.chunkCounts = plan.take(perGene);
    l.chunkStarts = plan.take(perGene);
    l.table = plan.takeFor<ChunkRef>(chunkBound(entryCount, geneCount, l.chunk));
    l.sortTempBytes = l.runScanTempBytes = l.scanTempBytes = 0;
    if (entryCount) {
        EM2_TRY(sortPairsU64U32BufferBytes(size_t(entryCount), 0u, 32u + geneBitsOf(geneCount), l.sortTempBytes));
        EM2_TRY(inclusiveScanBytes(size_t(entryCount), l.runScanTempBytes));
    }
    EM2_TRY(exclusiveScanU64Bytes(size_t(geneCount) + 1u, l.scanTempBytes));
    l.sortTemp = plan.take(l.sortTempBytes);
    l.runScanTemp = plan.take(l.runScanTempBytes);
    l.scanTemp = plan.take(l.scanTempBytes);
    l.total = plan.bytes;
    return hipSuccess;
}

}  // namespace

void setRankGenesTestLimits(uint32_t maxBlocks, uint32_t chunk, uint32_t ldsGroups)
{
    testMaxBlocks.store(maxBlocks);
    testChunk.store(chunk);
    testLdsGroups.store(ldsGroups);
}

const char* rankGenesUnsupported(uint64_t cellCount, uint64_t geneCount, uint64_t entryCount, uint64_t groupCount)
{
    if (cellCount > kRankGenesMaxCells) return "more than 2^21 cells: the cube of a tie group's size would leave 64 bits";
    if (entryCount >= (1ull << 32)) return "2^32 entries or more";
    if (geneCount * groupCount > (1ull << 28)) return "geneCount * groupCount is above 2^28";
    return nullptr;
}

const char* rankGenesErrorText(uint32_t inputError)
{
    if (inputError & 4u) return "toc does not start at 0, does not end at entryCount or is not ascending";
    if (inputError & 3u) return inputErrorText(inputError & 3u);
    if (inputError & kBadValue) return "a value is not a number";
    return "a group id is neither below groupCount nor the no-group value";
}

size_t rankGenesWorkspaceBytes(uint64_t entryCount, uint32_t geneCount, uint32_t groupCount)
{
    Layout l;
    return layoutOf(entryCount, geneCount, groupCount, l) == hipSuccess ? l.total : 0;
}

hipError_t runRankGenes(const uint64_t* d_toc, const CountIn* d_data, uint32_t cellCount, uint32_t geneCount, uint64_t entryCount,
                        const double* d_normInverse, const uint32_t* d_group, uint32_t groupCount, uint32_t* d_groupSize,
                        uint32_t* d_nonZeroCount, uint64_t* d_rankSum2, uint64_t* d_tieSum, void* workspace, size_t workspaceBytes,
                        uint32_t* inputError, hipStream_t stream)
{
    *inputError = 0;
    Layout l;
    EM2_TRY(layoutOf(entryCount, geneCount, groupCount, l));
    if (workspaceBytes < l.total) return hipErrorInvalidValue;
    StageTimer timer("rankGenes");
    char* base = static_cast<char*>(workspace);
    uint32_t* words = arenaAt<uint32_t>(base, l.words);
    uint32_t* sizes = arenaAt<uint32_t>(base, l.sizes);
    uint64_t* offsets = arenaAt<uint64_t>(base, l.offsets);
    uint64_t* zeroBegin = arenaAt<uint64_t>(base, l.zeroBegin);
    uint64_t* zeroEnd = arenaAt<uint64_t>(base, l.zeroEnd);
    uint64_t* chunkCounts = arenaAt<uint64_t>(base, l.chunkCounts);
    uint64_t* chunkStarts = arenaAt<uint64_t>(base, l.chunkStarts);
    ChunkRef* table = arenaAt<ChunkRef>(base, l.table);
    DoubleBuffer<uint64_t> keys{arenaAt<uint64_t>(base, l.keysA), arenaAt<uint64_t>(base, l.keysB)};
    DoubleBuffer<uint32_t> groups{arenaAt<uint32_t>(base, l.groupsA), arenaAt<uint32_t>(base, l.groupsB)};
    const bool inLds = groupCount <= ldsGroupLimit();
    const size_t ldsBytes = inLds ? size_t(groupCount) * (sizeof(uint64_t) + sizeof(uint32_t)) : 0u;

    EM2_TRY(hipMemsetAsync(words, 0, 256, stream));
    EM2_TRY(hipMemsetAsync(sizes, 0, size_t(groupCount) * sizeof(uint32_t), stream));
    if (inLds) {
        groupSizesKernel<true><<<dim3(blocksFor(cellCount, 256u)), dim3(256), groupCount * sizeof(uint32_t), stream>>>(d_group, cellCount, groupCount,
                                                                                                                    sizes, words);
    } else {
        groupSizesKernel<false><<<dim3(blocksFor(cellCount, 256u)), dim3(256), 0, stream>>>(d_group, cellCount, groupCount, sizes, words);
    }
    entriesKernel<<<dim3(blocksFor(cellCount, 4u)), dim3(256), 0, stream>>>(d_toc, d_data, cellCount, geneCount, entryCount, d_normInverse,
                                                                            d_group, keys.current(), groups.current(), words);
    EM2_TRY(hipGetLastError());
    // the gene ids are the sort's keys and the segments' bounds, the groups index the counters: nothing goes on, and nothing
    // is written outside the workspace, before they are known to be good
    uint32_t found[3] = {0u, 0u, 0u};
    EM2_TRY(hipMemcpyAsync(found, words, sizeof(found), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    *inputError = found[0] | (found[1] ? kBadValue : 0u) | (found[2] ? kBadGroup : 0u);
    if (*inputError) return hipSuccess;
    EM2_TRY(timer.stage("entries", stream));

    if (entryCount) {
        EM2_TRY(sortPairs(base + l.sortTemp, l.sortTempBytes, keys, groups, size_t(entryCount), 0u, 32u + geneBitsOf(geneCount), stream));
    }
    EM2_TRY(timer.stage("sort", stream));

    uint32_t* flags = reinterpret_cast<uint32_t*>(keys.alternate());
    uint32_t* runNumber = flags + entryCount;
    uint32_t* runStart = groups.alternate();
    geneSearchesKernel<<<dim3(blocksFor(uint64_t(geneCount) + 1u, 256u)), dim3(256), 0, stream>>>(keys.current(), entryCount, geneCount, l.chunk,
                                                                                                 offsets, zeroBegin, zeroEnd, chunkCounts);
    EM2_TRY(hipGetLastError());
    if (entryCount) {
        headFlagsKernel<<<dim3(blocksFor(entryCount, 256u)), dim3(256), 0, stream>>>(keys.current(), entryCount, flags);
        EM2_TRY(hipGetLastError());
        EM2_TRY(inclusiveScan(base + l.runScanTemp, l.runScanTempBytes, flags, runNumber, size_t(entryCount), stream));
        runStartsKernel<<<dim3(blocksFor(entryCount, 256u)), dim3(256), 0, stream>>>(flags, runNumber, entryCount, runStart);
        EM2_TRY(hipGetLastError());
    }
    EM2_TRY(exclusiveScan(base + l.scanTemp, l.scanTempBytes, chunkCounts, chunkStarts, size_t(geneCount) + 1u, stream));
    const uint64_t bound = chunkBound(entryCount, geneCount, l.chunk);
    chunkTableKernel<<<dim3(blocksFor(bound, 256u)), dim3(256), 0, stream>>>(chunkStarts, geneCount, table);
    EM2_TRY(hipGetLastError());
    EM2_TRY(timer.stage("searches, runs and chunk table", stream));

    const size_t counters = size_t(geneCount) * groupCount;
    EM2_TRY(hipMemsetAsync(d_nonZeroCount, 0, counters * sizeof(uint32_t), stream));
    EM2_TRY(hipMemsetAsync(d_rankSum2, 0, counters * sizeof(uint64_t), stream));
    EM2_TRY(hipMemsetAsync(d_tieSum, 0, size_t(geneCount) * sizeof(uint64_t), stream));
    if (inLds) {
        accumulateKernel<true><<<dim3(blocksFor(bound, 1u)), dim3(256), ldsBytes, stream>>>(
            groups.current(), flags, runNumber, runStart, offsets, zeroBegin, zeroEnd, chunkStarts, table, cellCount, geneCount, groupCount,
            l.chunk, d_nonZeroCount, d_rankSum2, d_tieSum);
    } else {
        accumulateKernel<false><<<dim3(blocksFor(bound, 1u)), dim3(256), 0, stream>>>(
            groups.current(), flags, runNumber, runStart, offsets, zeroBegin, zeroEnd, chunkStarts, table, cellCount, geneCount, groupCount,
            l.chunk, d_nonZeroCount, d_rankSum2, d_tieSum);
    }
    EM2_TRY(hipGetLastError());
    EM2_TRY(timer.stage(inLds ? "accumulate (LDS counters)" : "accumulate (global counters)", stream));

    finishKernel<<<dim3(blocksFor(counters, 256u)), dim3(256), 0, stream>>>(offsets, zeroBegin, zeroEnd, sizes, cellCount, geneCount, groupCount,
                                                                           d_nonZeroCount, d_rankSum2, d_tieSum, d_groupSize);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(timer.stage("finish", stream));
    return hipSuccess;
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

void em2_set_rank_genes_test_limits(uint32_t maxBlocks, uint32_t chunkEntries, uint32_t ldsGroupLimit)
{
    em2::setRankGenesTestLimits(maxBlocks, chunkEntries, ldsGroupLimit);
}

size_t em2_dev_rank_genes_workspace(uint32_t cellCount, uint32_t geneCount, uint64_t entryCount, uint32_t groupCount)
{
    if (em2::rankGenesUnsupported(cellCount, geneCount, entryCount, groupCount)) return 0;
    return em2::rankGenesWorkspaceBytes(entryCount, geneCount, groupCount);
}

// The argument checks every layer shares, under the name of the entry point that makes them.
static int checkShape(const char* who, uint32_t cellCount, uint32_t geneCount, uint64_t entryCount, uint32_t groupCount)
{
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (cellCount == 0) return failArgument(who, "cellCount must be positive");
    if (groupCount == 0) return failArgument(who, "groupCount must be positive");
    if (const char* why = em2::rankGenesUnsupported(cellCount, geneCount, entryCount, groupCount)) {
        return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": " + why);
    }
    return EM2_OK;
}

// The device call under the name of the entry point that makes it.
static int devRankGenes(const char* who, const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, uint32_t geneCount,
                        uint64_t entryCount, const double* d_normInverse, const uint32_t* d_group, uint32_t groupCount, uint32_t* d_groupSize,
                        uint32_t* d_nonZeroCount, uint64_t* d_rankSum2, uint64_t* d_tieSum, void* d_workspace, size_t workspaceBytes,
                        void* stream)
{
    if (const int rc = checkShape(who, cellCount, geneCount, entryCount, groupCount)) return rc;
    if (!d_toc || !d_group || !d_groupSize || !d_nonZeroCount || !d_rankSum2 || !d_tieSum || !d_workspace || (!d_data && entryCount)) {
        return failNull(who);
    }
    if (!haveDevice()) return failNoDevice(who);
    if (workspaceBytes < em2::rankGenesWorkspaceBytes(entryCount, geneCount, groupCount)) return failArgument(who, "workspace too small");
    uint32_t inputError = 0;
    EM2_HIP(em2::runRankGenes(d_toc, reinterpret_cast<const em2::CountIn*>(d_data), cellCount, geneCount, entryCount, d_normInverse, d_group,
                              groupCount, d_groupSize, d_nonZeroCount, d_rankSum2, d_tieSum, d_workspace, workspaceBytes, &inputError,
                              static_cast<hipStream_t>(stream)));
    if (inputError) return failArgument(who, em2::rankGenesErrorText(inputError));
    return EM2_OK;
}

int em2_dev_rank_genes(const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, uint32_t geneCount, uint64_t entryCount,
                       const double* d_normInverse, const uint32_t* d_group, uint32_t groupCount, uint32_t* d_groupSize,
                       uint32_t* d_nonZeroCount, uint64_t* d_rankSum2, uint64_t* d_tieSum, void* d_workspace, size_t workspaceBytes,
                       void* stream)
{
    return devRankGenes("em2_dev_rank_genes", d_toc, d_data, cellCount, geneCount, entryCount, d_normInverse, d_group, groupCount,
                        d_groupSize, d_nonZeroCount, d_rankSum2, d_tieSum, d_workspace, workspaceBytes, stream);
}

// The device call on a CSR that is on the device already; the integers to the host, and the statistics from them.
static int rankGenesToHost(const char* who, const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, uint32_t geneCount,
                           uint64_t entryCount, const double* d_normInverse, const uint32_t* group, uint32_t groupCount, uint32_t* groupSize,
                           uint32_t* nonZeroCount, uint64_t* rankSum2, uint64_t* tieSum, double* zScore, double* auc)
{
    const size_t counters = size_t(geneCount) * groupCount;
    DeviceBuffer dGroup, dSize, dCount, dSum, dTie, dWorkspace;
    const size_t workspaceBytes = em2::rankGenesWorkspaceBytes(entryCount, geneCount, groupCount);
    EM2_HIP(dGroup.upload(group, cellCount));
    EM2_HIP(dSize.allocateFor<uint32_t>(groupCount));
    EM2_HIP(dCount.allocateFor<uint32_t>(counters));
    EM2_HIP(dSum.allocateFor<uint64_t>(counters));
    EM2_HIP(dTie.allocateFor<uint64_t>(geneCount));
    EM2_HIP(dWorkspace.allocate(workspaceBytes));
    const int rc = devRankGenes(who, d_toc, d_data, cellCount, geneCount, entryCount, d_normInverse, dGroup.as<uint32_t>(), groupCount,
                                dSize.as<uint32_t>(), dCount.as<uint32_t>(), dSum.as<uint64_t>(), dTie.as<uint64_t>(), dWorkspace.p,
                                workspaceBytes, nullptr);
    if (rc != EM2_OK) return rc;
    EM2_HIP(dSize.download(groupSize, groupCount));
    EM2_HIP(dCount.download(nonZeroCount, counters));
    EM2_HIP(dSum.download(rankSum2, counters));
    EM2_HIP(dTie.download(tieSum, geneCount));
    em2::rankGeneStatisticsOfAll(cellCount, geneCount, groupCount, groupSize, rankSum2, tieSum, zScore, auc);
    return EM2_OK;
}

int em2_rank_genes(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount, const double* normInverse,
                   const uint32_t* group, uint32_t groupCount, uint32_t* groupSize, uint32_t* nonZeroCount, uint64_t* rankSum2,
                   uint64_t* tieSum, double* zScore, double* auc)
{
    const char* who = "em2_rank_genes";
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (cellCount == 0) return failArgument(who, "cellCount must be positive");
    if (!toc || !group || !groupSize || !nonZeroCount || !rankSum2 || !tieSum) return failNull(who);
    em2::UploadedCsr csr;
    if (const char* error = csr.check(toc, reinterpret_cast<const em2::CountIn*>(data), cellCount)) return failArgument(who, error);
    if (const int rc = checkShape(who, cellCount, geneCount, csr.nnz, groupCount)) return rc;
    if (!haveDevice()) return failNoDevice(who);
    EM2_HIP(csr.upload());                     // (the device checks the gene ids before any kernel indexes with them)
    DeviceBuffer dNorm;
    if (normInverse) EM2_HIP(dNorm.upload(normInverse, cellCount));
    return rankGenesToHost(who, csr.toc.as<uint64_t>(), csr.data.as<em2_count>(), cellCount, geneCount, csr.nnz,
                           normInverse ? dNorm.as<double>() : nullptr, group, groupCount, groupSize, nonZeroCount, rankSum2, tieSum, zScore, auc);
}

// The matrix-level call (em2_host.cpp), as em2_internal_gene_information: the rows of the universe go to the device with their
// global gene ids; the cells' norm inverses are taken over those WHOLE rows there (or come from the Cells file:
// normInverseOfRows, one per row), the gene set is applied by the device subset, and the rest is em2_dev_rank_genes.  rowToc
// from 0; group in the order of the rows.  Internal to the library.
int em2_internal_rank_genes(const uint64_t* rowToc, const em2_count* rowData, uint32_t cellCount, const uint32_t* geneLocalIds,
                            uint32_t globalGeneCount, uint32_t geneCount, int normalizationMethod, const double* normInverseOfRows,
                            const uint32_t* group, uint32_t groupCount, uint32_t* groupSize, uint32_t* nonZeroCount, uint64_t* rankSum2,
                            uint64_t* tieSum, double* zScore, double* auc)
{
    const char* who = "em2_matrix_rank_genes";
    if (normalizationMethod < 0 || normalizationMethod > 2) return failArgument(who, "invalid normalization method (0 none, 1 L1, 2 L2)");
    em2::UploadedCsr rows;
    if (const char* error = rows.check(rowToc, reinterpret_cast<const em2::CountIn*>(rowData), cellCount)) return failArgument(who, error);
    // (the subset keeps at most the rows' entries: a shape refused here is refused before anything goes to the device)
    if (const char* why = em2::rankGenesUnsupported(cellCount, geneCount, 0u, groupCount)) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": " + why);
    if (!haveDevice()) return failNoDevice(who);
    EM2_HIP(rows.upload());
    DeviceBuffer dNorm, dLocalIds, dToc, dData, dSubsetWorkspace;
    if (normalizationMethod != 0) {
        if (normInverseOfRows) {
            EM2_HIP(dNorm.upload(normInverseOfRows, cellCount));
        } else {
            EM2_HIP(dNorm.allocateFor<double>(cellCount));
            // (a global gene id is checked by nothing here: the subset below drops what the gene set does not know)
            EM2_HIP(em2::launchCellNormInverses(rows.toc.as<uint64_t>(), rows.data.as<em2::CountIn>(), cellCount, 0xffffffffu,
                                                normalizationMethod, dNorm.as<double>(), nullptr));
        }
    }
    const size_t subsetBytes = em2::subsetWorkspaceBytes(cellCount);
    EM2_HIP(dLocalIds.upload(geneLocalIds, globalGeneCount));
    EM2_HIP(dToc.allocateFor<uint64_t>(size_t(cellCount) + 1));
    EM2_HIP(dSubsetWorkspace.allocate(subsetBytes));
    EM2_HIP(em2::launchSubsetCount(rows.toc.as<uint64_t>(), rows.data.as<em2::CountIn>(), nullptr, cellCount, dLocalIds.as<uint32_t>(),
                                   globalGeneCount, dToc.as<uint64_t>(), dSubsetWorkspace.p, subsetBytes, nullptr));
    uint64_t entryCount = 0;
    EM2_HIP(hipMemcpy(&entryCount, dToc.as<uint64_t>() + cellCount, sizeof(uint64_t), hipMemcpyDeviceToHost));
    EM2_HIP(dData.allocateFor<em2_count>(entryCount));
    EM2_HIP(em2::launchSubsetFill(rows.toc.as<uint64_t>(), rows.data.as<em2::CountIn>(), nullptr, cellCount, dLocalIds.as<uint32_t>(),
                                  globalGeneCount, dToc.as<uint64_t>(), dData.as<em2::CountIn>(), nullptr));
    return rankGenesToHost(who, dToc.as<uint64_t>(), dData.as<em2_count>(), cellCount, geneCount, entryCount,
                           normalizationMethod != 0 ? dNorm.as<double>() : nullptr, group, groupCount, groupSize, nonZeroCount, rankSum2, tieSum,
                           zScore, auc);
}

}  // extern "C"
