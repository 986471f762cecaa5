// em2_signature_graph.hip -- ExpressionMatrix::createSignatureGraph (src/ExpressionMatrixSignatureGraph.cpp:42-150),
// SignatureGraph::createEdges (src/SignatureGraph.cpp:23-48), the grouping of ExpressionMatrix::analyzeLshSignatures
// (src/ExpressionMatrixLsh.cpp:1421-1424) and the counts of Lsh::writeSignatureStatistics (src/Lsh.cpp:279-303) on signatures
// in device memory.  Integer work throughout: every output is bit-exact.
//
// The reference fills a std::map<BitSetPointer, vector<CellId>> cell by cell and, for the edges, runs one map::find per
// (vertex, zero bit).  Here:
//   * signatureKeysKernel      key = word w of every cell's signature, in the current order of the cells (the first pass also
//                              numbers the cells and checks that no bit at or beyond lshCount is set);
//   * rocPRIM's STABLE radix sort of (key, cell id): for one word a single sort over the lshCount significant bits (shifted to
//     the bottom of the key); for W words one sort per word from the last to the first, so the cells end in the map's order
//     (std::lexicographical_compare over the words, src/BitSet.hpp:157-160) with the cell ids of equal signatures ascending
//     (push_back in cell order, :73-75);
//   * groupHeadsKernel, a scan, groupStartsKernel      the first cell of every distinct signature;
//   * groupKeepKernel, two scans, groupCompactKernel   size >= minCellCount (:118-120) as an order-preserving compaction: the
//                              vertex of every kept group, its signature, its cells and their offsets;
//   * signatureEdgesKernel<0>  THE HOT PATH.  One wave per (vertex v0, 64-bit chunk c of the signature); lane b owns bit
//                              64 c + b.  A lane whose bit is 0 looks for v0's signature with that bit set by a binary search
//                              over the sorted vertex signatures ABOVE v0 (setting a bit makes the signature larger).  The
//                              ballot of the lanes that found one is kept per (v0, c) with its popcount;
//   * a scan over the popcounts, then signatureEdgesKernel<1>: the lanes of the ballot search once more and write (v0, v1) at
//     the scan's offset plus the lane's rank in the ballot.  The edge list is in (v0, bit) ascending order whatever the
//     scheduling: Boost's add_edge order for the reference's loop;
//   * signatureStatisticsKernel   a wave loads word w of 64 cells and takes 64 ballots; lane b keeps the count of bit 64 w + b
//                              over the wave's share of the cells and adds it with one integer atomic.
//
// For lshCount > 64 the reference itself is not defined (BitSet's copy allocates one word, src/BitSet.hpp:184, :200); the
// order and the neighbours here are the obvious continuation: lexicographic over the words, one-bit neighbours across all of
// them.

#include "em2_device.h"
#include "em2_entry.h"
#include "em2_primitives.h"
#include "em2_scratch.h"
#include "em2_wave.h"

#include <algorithm>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>

// What the device code and the C entry points at the end of this file share.
namespace em2 {

// The longest signature the grouping takes (1024 words of 64 bits).
constexpr uint32_t kSignatureGraphMaxLshCount = 65536;

// What ExpressionMatrix::createSignatureGraph (src/ExpressionMatrixSignatureGraph.cpp:42-150) leaves in the SignatureGraph,
// in host memory.  Vertices in the order of the reference's std::map (ascending by word 0, then word 1, ...); cells are ids
// local to the cell set, ascending within a vertex; edges in the order of SignatureGraph::createEdges (src/SignatureGraph.cpp:
// 23-48): vertex 0 ascending, then bit ascending.
struct SignatureGraphResult {
    uint32_t wordCount = 0;
    uint64_t distinctCount = 0;                  // groups before the minCellCount filter
    std::vector<uint64_t> vertexSignatures;      // [vertexCount][wordCount]
    std::vector<uint64_t> cellOffsets;           // [vertexCount + 1]
    std::vector<uint32_t> cells;                 // [cellOffsets[vertexCount]]
    std::vector<uint32_t> edgeVertex0, edgeVertex1;
};

// d_signatures [cellCount][wordCount] in device memory, cellCount > 0, 0 < lshCount <= kSignatureGraphMaxLshCount.
// withEdges false: the groups only (analyzeLshSignatures).  *inputError != 0: a signature has a bit set at or beyond lshCount,
// nothing was computed.  Takes its scratch from the cache of em2_scratch.h; synchronises the stream.
static hipError_t runSignatureGraph(const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount, uint64_t minCellCount, bool withEdges,
                                    SignatureGraphResult& out, uint32_t* inputError, hipStream_t stream);

// Lsh::writeSignatureStatistics (src/Lsh.cpp:279-303) without its text: d_setCount[i] = the cells with bit i set, i < lshCount.
// d_setCount is zeroed here.  Asynchronous on the stream.
static hipError_t launchSignatureStatistics(const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount,
                                            unsigned long long* d_setCount, hipStream_t stream);

namespace {

// keys[i] = word w of the signature of the i-th cell in the current order (order NULL: cell i, and ids[i] = i), shifted right
// by `shift`: the last word's significant bits come to lie at the bottom of the key.  padMask: the bits of word w at or beyond
// lshCount (0 for every word but the last); *error |= 1 where one is set.
__global__ void __launch_bounds__(256)
signatureKeysKernel(const uint64_t* __restrict__ signatures, uint32_t cellCount, uint32_t wordCount, uint32_t w,
                    const uint32_t* __restrict__ order, uint64_t padMask, uint32_t shift, uint64_t* __restrict__ keys,
                    uint32_t* __restrict__ ids, uint32_t* __restrict__ error)
{
    bool bad = false;
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < cellCount; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t cell = order ? order[i] : uint32_t(i);
        const uint64_t key = signatures[uint64_t(cell) * wordCount + w];
        bad = bad || (key & padMask) != 0u;
        keys[i] = key >> shift;
        if (!order) ids[i] = cell;
    }
    if (bad) atomicOr(error, 1u);
}

__device__ __forceinline__ bool sameSignature(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, uint32_t wordCount)
{
    for (uint32_t w = 0; w < wordCount; ++w) {
        if (a[w] != b[w]) return false;
    }
    return true;
}

// heads[i] = 1 where the i-th cell in sorted order starts a new signature, i < cellCount; heads[cellCount] = 0 (the scan's
// last input: its output there is the number of distinct signatures).
__global__ void __launch_bounds__(256)
groupHeadsKernel(const uint64_t* __restrict__ signatures, const uint32_t* __restrict__ order, uint32_t cellCount, uint32_t wordCount,
                 uint32_t* __restrict__ heads)
{
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= cellCount; i += uint64_t(gridDim.x) * blockDim.x) {
        uint32_t head = 0u;
        if (i < cellCount) {
            head = i == 0u || !sameSignature(signatures + uint64_t(order[i]) * wordCount, signatures + uint64_t(order[i - 1u]) * wordCount, wordCount);
        }
        heads[i] = head;
    }
}

// headsBefore: the exclusive scan of heads, [cellCount + 1].  groupStarts[g] = the sorted position of group g's first cell,
// groupStarts[groupCount] = cellCount.
__global__ void __launch_bounds__(256)
groupStartsKernel(const uint32_t* __restrict__ heads, const uint64_t* __restrict__ headsBefore, uint32_t cellCount,
                  uint32_t* __restrict__ groupStarts)
{
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= cellCount; i += uint64_t(gridDim.x) * blockDim.x) {
        if (i == cellCount || heads[i]) groupStarts[headsBefore[i]] = uint32_t(i);
    }
}

// keep[g] = 1 and keptCells[g] = the group's size where that size is at least minCellCount (a size_t comparison, :118), else 0;
// 0 for every g in [groupCount, cellCount] too (the scans run over cellCount + 1 entries).
__global__ void __launch_bounds__(256)
groupKeepKernel(const uint32_t* __restrict__ groupStarts, const uint64_t* __restrict__ headsBefore, uint32_t cellCount,
                uint64_t minCellCount, uint32_t* __restrict__ keep, uint32_t* __restrict__ keptCells)
{
    const uint64_t groupCount = headsBefore[cellCount];
    for (uint64_t g = blockIdx.x * blockDim.x + threadIdx.x; g <= cellCount; g += uint64_t(gridDim.x) * blockDim.x) {
        uint32_t size = 0u;
        if (g < groupCount) size = groupStarts[g + 1u] - groupStarts[g];
        const bool kept = g < groupCount && uint64_t(size) >= minCellCount;
        keep[g] = kept ? 1u : 0u;
        keptCells[g] = kept ? size : 0u;
    }
}

// vertexOfGroup / cellOffsetOfGroup: the exclusive scans of keep / keptCells.  A thread per sorted position: the cell goes to
// its place in its vertex; the first cell of a kept group also writes the vertex's signature and offset.
__global__ void __launch_bounds__(256)
groupCompactKernel(const uint64_t* __restrict__ signatures, const uint32_t* __restrict__ order, const uint32_t* __restrict__ heads,
                   const uint64_t* __restrict__ headsBefore, const uint32_t* __restrict__ groupStarts, const uint32_t* __restrict__ keep,
                   const uint64_t* __restrict__ vertexOfGroup, const uint64_t* __restrict__ cellOffsetOfGroup, uint32_t cellCount,
                   uint32_t wordCount, uint64_t* __restrict__ vertexSignatures, uint64_t* __restrict__ vertexCellOffsets,
                   uint32_t* __restrict__ cells)
{
    for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= cellCount; i += uint64_t(gridDim.x) * blockDim.x) {
        if (i == cellCount) {
            vertexCellOffsets[vertexOfGroup[cellCount]] = cellOffsetOfGroup[cellCount];
            continue;
        }
        const uint64_t g = headsBefore[i] + heads[i] - 1u;
        if (!keep[g]) continue;
        const uint64_t v = vertexOfGroup[g];
        const uint32_t cell = order[i];
        cells[cellOffsetOfGroup[g] + (i - groupStarts[g])] = cell;
        if (heads[i]) {
            vertexCellOffsets[v] = cellOffsetOfGroup[g];
            for (uint32_t w = 0; w < wordCount; ++w) vertexSignatures[v * wordCount + w] = signatures[uint64_t(cell) * wordCount + w];
        }
    }
}

// The vertex whose signature is that of v0 with `bit` of word c set, or vertexCount where there is none: the lower bound of
// that signature among the vertices above v0 (the vertex signatures ascend lexicographically, and the wanted one is larger than
// v0's), then the test for equality.
__device__ __forceinline__ uint64_t findNeighbour(const uint64_t* __restrict__ vertexSignatures, uint64_t vertexCount, uint32_t wordCount,
                                                  uint64_t v0, uint32_t c, uint64_t bit)
{
    const uint64_t* mine = vertexSignatures + v0 * wordCount;
    uint64_t low = v0 + 1u, high = vertexCount;
    while (low < high) {
        const uint64_t middle = low + (high - low) / 2u;
        const uint64_t* row = vertexSignatures + middle * wordCount;
        bool less = false;                                     // row < wanted
        for (uint32_t w = 0; w < wordCount; ++w) {
            const uint64_t wanted = w == c ? mine[w] | bit : mine[w];
            const uint64_t have = row[w];
            if (have != wanted) {
                less = have < wanted;
                break;
            }
        }
        if (less) low = middle + 1u;
        else high = middle;
    }
    if (low >= vertexCount) return vertexCount;
    const uint64_t* row = vertexSignatures + low * wordCount;
    for (uint32_t w = 0; w < wordCount; ++w) {
        if (row[w] != (w == c ? mine[w] | bit : mine[w])) return vertexCount;
    }
    return low;
}

// Item t = v0 * wordCount + c, one wave each.  WRITE 0: found[t] = the ballot of the lanes whose neighbour exists, counts[t] its
// popcount.  WRITE 1: the lanes of found[t] write their edge at offsets[t] + their rank in the ballot.
template <int WRITE>
__global__ void __launch_bounds__(256)
signatureEdgesKernel(const uint64_t* __restrict__ vertexSignatures, uint64_t vertexCount, uint32_t wordCount, uint32_t lshCount,
                     uint64_t* __restrict__ found, uint32_t* __restrict__ counts, const uint64_t* __restrict__ offsets,
                     uint32_t* __restrict__ edgeVertex0, uint32_t* __restrict__ edgeVertex1)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = uint64_t(gridDim.x) * (blockDim.x >> 6);
    const uint64_t items = vertexCount * wordCount;
    for (uint64_t t = uint64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); t < items; t += waves) {
        const uint64_t v0 = t / wordCount;
        const uint32_t c = uint32_t(t - v0 * wordCount);
        const uint64_t bit = 1ull << (63u - lane);             // the first bit is the most significant (src/BitSet.hpp:56-62)
        if (WRITE == 0) {
            const bool candidate = 64u * c + lane < lshCount && (vertexSignatures[t] & bit) == 0u;
            bool have = false;
            if (candidate) have = findNeighbour(vertexSignatures, vertexCount, wordCount, v0, c, bit) < vertexCount;
            const uint64_t ballot = __ballot(have);
            if (lane == 0u) {
                found[t] = ballot;
                counts[t] = uint32_t(__popcll(ballot));
            }
        } else {
            const uint64_t ballot = found[t];
            if ((ballot >> lane) & 1u) {                       // (lane b's bit of the ballot is bit b; its bit of the word is 63 - b)
                const uint64_t v1 = findNeighbour(vertexSignatures, vertexCount, wordCount, v0, c, bit);
                const uint64_t at = offsets[t] + lanesBelow(ballot);
                edgeVertex0[at] = uint32_t(v0);
                edgeVertex1[at] = uint32_t(v1);
            }
        }
    }
}

// Wave g of the grid counts word g % wordCount over the batches of 64 cells stripe, stripe + stripes, ... (stripe = g /
// wordCount): the waves of a block read neighbouring words of the same cells.  Lane b holds the count of bit 64 w + b.
__global__ void __launch_bounds__(256)
signatureStatisticsKernel(const uint64_t* __restrict__ signatures, uint32_t cellCount, uint32_t wordCount, uint32_t lshCount,
                          uint32_t stripes, unsigned long long* __restrict__ setCount)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = uint64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (wave >= uint64_t(stripes) * wordCount) return;
    const uint32_t w = uint32_t(wave % wordCount);
    const uint32_t stripe = uint32_t(wave / wordCount);
    unsigned long long mine = 0u;
    for (uint64_t first = uint64_t(stripe) * 64u; first < cellCount; first += uint64_t(stripes) * 64u) {
        const uint64_t cell = first + lane;
        const uint64_t word = cell < cellCount ? signatures[cell * wordCount + w] : 0u;
#pragma unroll 8
        for (uint32_t b = 0; b < 64u; ++b) {
            const uint32_t set = uint32_t(__popcll(__ballot((word >> (63u - b)) & 1u)));
            if (lane == b) mine += set;
        }
    }
    if (64u * w + lane < lshCount && mine != 0u) atomicAdd(setCount + 64u * w + lane, mine);
}

// The grouping's scratch: everything is sized by the cells, which bound the groups and the vertices.
struct GroupLayout {
    size_t error, keysA, keysB, idsA, idsB, heads, headsBefore, groupStarts, keep, keptCells, vertexOfGroup, cellOffsetOfGroup,
        vertexSignatures, vertexCellOffsets, cells, sortTemp, scanTemp, total;
    size_t sortTempBytes, scanTempBytes;
};

hipError_t groupLayoutOf(uint32_t cellCount, uint32_t wordCount, GroupLayout& l)
{
    ArenaPlan plan;
    const size_t n = cellCount, n1 = size_t(cellCount) + 1u;
    l.error = plan.take(256);
    l.keysA = plan.takeFor<uint64_t>(n);
    l.keysB = plan.takeFor<uint64_t>(n);
    l.idsA = plan.takeFor<uint32_t>(n);
    l.idsB = plan.takeFor<uint32_t>(n);
    l.heads = plan.takeFor<uint32_t>(n1);
    l.headsBefore = plan.takeFor<uint64_t>(n1);
    l.groupStarts = plan.takeFor<uint32_t>(n1);
    l.keep = plan.takeFor<uint32_t>(n1);
    l.keptCells = plan.takeFor<uint32_t>(n1);
    l.vertexOfGroup = plan.takeFor<uint64_t>(n1);
    l.cellOffsetOfGroup = plan.takeFor<uint64_t>(n1);
    l.vertexSignatures = plan.takeFor<uint64_t>(n * wordCount);
    l.vertexCellOffsets = plan.takeFor<uint64_t>(n1);
    l.cells = plan.takeFor<uint32_t>(n);
    l.sortTempBytes = 0;
    EM2_TRY(sortPairsU64U32BufferBytes(n, 0u, 64u, l.sortTempBytes));
    l.scanTempBytes = 0;
    EM2_TRY(exclusiveScanU32ToU64Bytes(n1, l.scanTempBytes));
    l.sortTemp = plan.take(l.sortTempBytes);
    l.scanTemp = plan.take(l.scanTempBytes);
    l.total = plan.bytes;
    return hipSuccess;
}

}  // namespace

hipError_t runSignatureGraph(const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount, uint64_t minCellCount, bool withEdges,
                             SignatureGraphResult& out, uint32_t* inputError, hipStream_t stream)
{
    *inputError = 0;
    const uint32_t wordCount = wordCountOf(lshCount);
    out = SignatureGraphResult();
    out.wordCount = wordCount;
    StageTimer timer("signatureGraph");
    GroupLayout l;
    EM2_TRY(groupLayoutOf(cellCount, wordCount, l));
    CachedBuffer arena, edgeArena, edges;
    EM2_TRY(arena.allocate(l.total));
    char* base = arena.as<char>();
    uint32_t* error = arenaAt<uint32_t>(base, l.error);
    uint32_t* heads = arenaAt<uint32_t>(base, l.heads);
    uint64_t* headsBefore = arenaAt<uint64_t>(base, l.headsBefore);
    uint32_t* groupStarts = arenaAt<uint32_t>(base, l.groupStarts);
    uint32_t* keep = arenaAt<uint32_t>(base, l.keep);
    uint32_t* keptCells = arenaAt<uint32_t>(base, l.keptCells);
    uint64_t* vertexOfGroup = arenaAt<uint64_t>(base, l.vertexOfGroup);
    uint64_t* cellOffsetOfGroup = arenaAt<uint64_t>(base, l.cellOffsetOfGroup);
    uint64_t* vertexSignatures = arenaAt<uint64_t>(base, l.vertexSignatures);
    uint64_t* vertexCellOffsets = arenaAt<uint64_t>(base, l.vertexCellOffsets);
    uint32_t* cells = arenaAt<uint32_t>(base, l.cells);
    DoubleBuffer<uint64_t> keys{arenaAt<uint64_t>(base, l.keysA), arenaAt<uint64_t>(base, l.keysB)};
    DoubleBuffer<uint32_t> ids{arenaAt<uint32_t>(base, l.idsA), arenaAt<uint32_t>(base, l.idsB)};
    const size_t n1 = size_t(cellCount) + 1u;
    const dim3 perCell(gridFor(n1)), threads(256);

    // the sort: the last word first; of the last word only the bits below lshCount (the others are checked to be zero), moved
    // to the bottom of the key -- a bit range that ends at 64 has to begin at 0: for sizes that rocPRIM sorts by merging, its
    // comparator masks the keys with (1 << (begin + bits)) - 1, a shift by 64
    EM2_TRY(hipMemsetAsync(error, 0, 256, stream));
    const uint32_t liveBitsOfLastWord = lshCount - 64u * (wordCount - 1u);
    for (uint32_t pass = 0; pass < wordCount; ++pass) {
        const uint32_t w = wordCount - 1u - pass;
        const uint32_t shift = pass == 0u ? 64u - liveBitsOfLastWord : 0u;
        const uint64_t padMask = shift ? (1ull << shift) - 1ull : 0ull;
        signatureKeysKernel<<<perCell, threads, 0, stream>>>(d_signatures, cellCount, wordCount, w, pass == 0u ? nullptr : ids.current(),
                                                            padMask, shift, keys.current(), pass == 0u ? ids.current() : nullptr, error);
        EM2_TRY(hipGetLastError());
        EM2_TRY(sortPairs(base + l.sortTemp, l.sortTempBytes, keys, ids, size_t(cellCount), 0u, pass == 0u ? liveBitsOfLastWord : 64u, stream));
    }
    EM2_TRY(hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    if (*inputError) {
        arena.idle = true;
        return hipSuccess;
    }
    EM2_TRY(timer.stage("sort", stream));
    const uint32_t* order = ids.current();

    groupHeadsKernel<<<perCell, threads, 0, stream>>>(d_signatures, order, cellCount, wordCount, heads);
    EM2_TRY(hipGetLastError());
    EM2_TRY(exclusiveScan(base + l.scanTemp, l.scanTempBytes, heads, headsBefore, n1, stream));
    groupStartsKernel<<<perCell, threads, 0, stream>>>(heads, headsBefore, cellCount, groupStarts);
    EM2_TRY(hipGetLastError());
    groupKeepKernel<<<perCell, threads, 0, stream>>>(groupStarts, headsBefore, cellCount, minCellCount, keep, keptCells);
    EM2_TRY(hipGetLastError());
    EM2_TRY(exclusiveScan(base + l.scanTemp, l.scanTempBytes, keep, vertexOfGroup, n1, stream));
    EM2_TRY(exclusiveScan(base + l.scanTemp, l.scanTempBytes, keptCells, cellOffsetOfGroup, n1, stream));
    groupCompactKernel<<<perCell, threads, 0, stream>>>(d_signatures, order, heads, headsBefore, groupStarts, keep, vertexOfGroup,
                                                       cellOffsetOfGroup, cellCount, wordCount, vertexSignatures, vertexCellOffsets, cells);
    EM2_TRY(hipGetLastError());
    uint64_t sizes[3] = {0, 0, 0};                             // distinct signatures, vertices, cells in vertices
    EM2_TRY(hipMemcpyAsync(sizes + 0, headsBefore + cellCount, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipMemcpyAsync(sizes + 1, vertexOfGroup + cellCount, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipMemcpyAsync(sizes + 2, cellOffsetOfGroup + cellCount, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(timer.stage("groups and vertices", stream));
    const uint64_t vertexCount = sizes[1];
    if (sizes[0] > cellCount || vertexCount > sizes[0] || sizes[2] > cellCount) {      // (the sizes of the host arrays below)
        arena.idle = true;
        return hipErrorUnknown;
    }
    out.distinctCount = sizes[0];
    out.vertexSignatures.resize(size_t(vertexCount) * wordCount);
    out.cellOffsets.resize(size_t(vertexCount) + 1u);
    out.cells.resize(size_t(sizes[2]));
    if (vertexCount) {
        EM2_TRY(hipMemcpyAsync(out.vertexSignatures.data(), vertexSignatures, out.vertexSignatures.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    }
    EM2_TRY(hipMemcpyAsync(out.cellOffsets.data(), vertexCellOffsets, out.cellOffsets.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    if (sizes[2]) EM2_TRY(hipMemcpyAsync(out.cells.data(), cells, out.cells.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));

    if (withEdges && vertexCount) {
        const uint64_t items = vertexCount * wordCount;
        ArenaPlan plan;
        const size_t offFound = plan.takeFor<uint64_t>(items);
        const size_t offCounts = plan.takeFor<uint32_t>(items + 1u);
        const size_t offOffsets = plan.takeFor<uint64_t>(items + 1u);
        size_t edgeScanBytes = 0;
        EM2_TRY(exclusiveScanU32ToU64Bytes(items + 1u, edgeScanBytes));
        const size_t offTemp = plan.take(edgeScanBytes);
        EM2_TRY(edgeArena.allocate(plan.bytes));
        char* edgeBase = edgeArena.as<char>();
        uint64_t* found = arenaAt<uint64_t>(edgeBase, offFound);
        uint32_t* counts = arenaAt<uint32_t>(edgeBase, offCounts);
        uint64_t* offsets = arenaAt<uint64_t>(edgeBase, offOffsets);
        EM2_TRY(hipMemsetAsync(counts + items, 0, sizeof(uint32_t), stream));
        signatureEdgesKernel<0><<<dim3(gridFor(items * 64u)), threads, 0, stream>>>(vertexSignatures, vertexCount, wordCount, lshCount, found,
                                                                                 counts, nullptr, nullptr, nullptr);
        EM2_TRY(hipGetLastError());
        EM2_TRY(exclusiveScan(edgeBase + offTemp, edgeScanBytes, counts, offsets, size_t(items) + 1u, stream));
        uint64_t edgeCount = 0;
        EM2_TRY(hipMemcpyAsync(&edgeCount, offsets + items, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        EM2_TRY(timer.stage("edges: count and scan", stream));
        if (edgeCount > items * 64u) {
            arena.idle = edgeArena.idle = true;
            return hipErrorUnknown;
        }
        out.edgeVertex0.resize(size_t(edgeCount));
        out.edgeVertex1.resize(size_t(edgeCount));
        if (edgeCount) {
            EM2_TRY(edges.allocate(2u * alignUp(edgeCount * sizeof(uint32_t))));
            uint32_t* edge0 = edges.as<uint32_t>();
            uint32_t* edge1 = reinterpret_cast<uint32_t*>(edges.as<char>() + alignUp(edgeCount * sizeof(uint32_t)));
            signatureEdgesKernel<1><<<dim3(gridFor(items * 64u)), threads, 0, stream>>>(vertexSignatures, vertexCount, wordCount, lshCount, found,
                                                                                     nullptr, offsets, edge0, edge1);
            EM2_TRY(hipGetLastError());
            EM2_TRY(hipMemcpyAsync(out.edgeVertex0.data(), edge0, edgeCount * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            EM2_TRY(hipMemcpyAsync(out.edgeVertex1.data(), edge1, edgeCount * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        }
    }
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(timer.stage(withEdges ? "edges: write; results to the host" : "results to the host", stream));
    arena.idle = edgeArena.idle = edges.idle = true;           // (everything that used the blocks has been waited for)
    return hipSuccess;
}

hipError_t launchSignatureStatistics(const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount,
                                     unsigned long long* d_setCount, hipStream_t stream)
{
    const uint32_t wordCount = wordCountOf(lshCount);
    EM2_TRY(hipMemsetAsync(d_setCount, 0, size_t(lshCount) * sizeof(unsigned long long), stream));
    // at most 2048 waves or so: every wave ends with one atomic per lane
    const uint64_t batches = (uint64_t(cellCount) + 63u) / 64u;
    const uint64_t most = wordCount >= 2048u ? 1u : 2048u / wordCount;
    const uint32_t stripes = uint32_t(batches < most ? batches : most);
    const uint64_t waves = uint64_t(stripes) * wordCount;
    signatureStatisticsKernel<<<dim3(uint32_t((waves + 3u) / 4u)), dim3(256), 0, stream>>>(d_signatures, cellCount, wordCount, lshCount,
                                                                                         stripes, d_setCount);
    return hipGetLastError();
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;
using em2::wordCountOf;

extern "C" {

struct em2_signature_graph {
    em2::SignatureGraphResult result;
};

// lshCount, then cellCount, then the pointer, then the device: none of them reaches a launch.
static int checkSignatureArguments(const char* who, const void* signatures, uint32_t cellCount, uint32_t lshCount)
{
    if (lshCount == 0) return failArgument(who, "lshCount must be positive");
    if (lshCount > em2::kSignatureGraphMaxLshCount) {
        return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": lshCount above " + std::to_string(em2::kSignatureGraphMaxLshCount) + " is not supported");
    }
    if (cellCount == 0) return failArgument(who, "cellCount must be positive");
    if (!signatures) return failNull(who);
    if (!haveDevice()) return failNoDevice(who);
    return EM2_OK;
}

static int signatureGroups(const char* who, const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount, uint64_t minCellCount,
                           bool withEdges, em2::SignatureGraphResult& result)
{
    uint32_t inputError = 0;
    EM2_HIP(em2::runSignatureGraph(d_signatures, cellCount, lshCount, minCellCount, withEdges, result, &inputError, nullptr));
    if (inputError) return failArgument(who, "a signature has a bit set at or beyond lshCount");
    return EM2_OK;
}

static int signatureGraphCreate(const char* who, bool onDevice, const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount,
                                uint64_t minCellCount, em2_signature_graph** graph)
{
    if (!graph) return failNull(who);
    *graph = nullptr;
    int rc = checkSignatureArguments(who, signatures, cellCount, lshCount);
    if (rc != EM2_OK) return rc;
    DeviceBuffer dSig;
    if (!onDevice) EM2_HIP(dSig.upload(signatures, size_t(cellCount) * wordCountOf(lshCount)));
    std::unique_ptr<em2_signature_graph> g(new em2_signature_graph);
    rc = signatureGroups(who, onDevice ? signatures : dSig.as<uint64_t>(), cellCount, lshCount, minCellCount, true, g->result);
    if (rc != EM2_OK) return rc;
    *graph = g.release();
    return EM2_OK;
}

int em2_signature_graph_create(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, uint64_t minCellCount,
                               em2_signature_graph** graph)
{
    return signatureGraphCreate("em2_signature_graph_create", false, signatures, cellCount, lshCount, minCellCount, graph);
}

int em2_dev_signature_graph_create(const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount, uint64_t minCellCount,
                                   em2_signature_graph** graph)
{
    return signatureGraphCreate("em2_dev_signature_graph_create", true, d_signatures, cellCount, lshCount, minCellCount, graph);
}

int em2_signature_graph_sizes(const em2_signature_graph* graph, uint64_t* distinctCount, uint32_t* vertexCount, uint32_t* wordCount,
                              uint64_t* cellCount, uint64_t* edgeCount)
{
    if (!graph) return failNull("em2_signature_graph_sizes");
    const em2::SignatureGraphResult& r = graph->result;
    if (distinctCount) *distinctCount = r.distinctCount;
    if (vertexCount) *vertexCount = uint32_t(r.cellOffsets.size() - 1u);
    if (wordCount) *wordCount = r.wordCount;
    if (cellCount) *cellCount = r.cells.size();
    if (edgeCount) *edgeCount = r.edgeVertex0.size();
    return EM2_OK;
}

int em2_signature_graph_get(const em2_signature_graph* graph, uint64_t* vertexSignatures, uint64_t* cellOffsets, uint32_t* cells,
                            uint32_t* edgeVertex0, uint32_t* edgeVertex1)
{
    if (!graph) return failNull("em2_signature_graph_get");
    const em2::SignatureGraphResult& r = graph->result;
    if (vertexSignatures) std::copy(r.vertexSignatures.begin(), r.vertexSignatures.end(), vertexSignatures);
    if (cellOffsets) std::copy(r.cellOffsets.begin(), r.cellOffsets.end(), cellOffsets);
    if (cells) std::copy(r.cells.begin(), r.cells.end(), cells);
    if (edgeVertex0) std::copy(r.edgeVertex0.begin(), r.edgeVertex0.end(), edgeVertex0);
    if (edgeVertex1) std::copy(r.edgeVertex1.begin(), r.edgeVertex1.end(), edgeVertex1);
    return EM2_OK;
}

void em2_signature_graph_free(em2_signature_graph* graph) { delete graph; }

// setCount[lshCount] on the host from signatures that are on the device.
static int signatureStatisticsToHost(const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount, uint64_t* setCount)
{
    DeviceBuffer dCounts;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the kernel's counters are the caller's uint64_t");
    EM2_HIP(dCounts.allocateFor<uint64_t>(lshCount));
    EM2_HIP(em2::launchSignatureStatistics(d_signatures, cellCount, lshCount, dCounts.as<unsigned long long>(), nullptr));
    EM2_HIP(dCounts.download(setCount, lshCount));
    return EM2_OK;
}

static int signatureStatistics(const char* who, bool onDevice, const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount,
                               uint64_t* setCount)
{
    const int rc = checkSignatureArguments(who, setCount ? static_cast<const void*>(signatures) : nullptr, cellCount, lshCount);
    if (rc != EM2_OK) return rc;
    DeviceBuffer dSig;
    if (!onDevice) EM2_HIP(dSig.upload(signatures, size_t(cellCount) * wordCountOf(lshCount)));
    return signatureStatisticsToHost(onDevice ? signatures : dSig.as<uint64_t>(), cellCount, lshCount, setCount);
}

int em2_lsh_signature_statistics(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, uint64_t* setCount)
{
    return signatureStatistics("em2_lsh_signature_statistics", false, signatures, cellCount, lshCount, setCount);
}

int em2_dev_lsh_signature_statistics(const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount, uint64_t* setCount)
{
    return signatureStatistics("em2_dev_lsh_signature_statistics", true, d_signatures, cellCount, lshCount, setCount);
}

int em2_analyze_lsh_signatures(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, const char* directory)
{
    const char* who = "em2_analyze_lsh_signatures";
    int rc = checkSignatureArguments(who, signatures, cellCount, lshCount);
    if (rc != EM2_OK) return rc;
    const uint32_t words = wordCountOf(lshCount);
    DeviceBuffer dSig;
    EM2_HIP(dSig.upload(signatures, size_t(cellCount) * words));
    em2::SignatureGraphResult groups;                           // src/ExpressionMatrixLsh.cpp:1421-1424: the map, nothing filtered
    rc = signatureGroups(who, dSig.as<uint64_t>(), cellCount, lshCount, 0u, false, groups);
    if (rc != EM2_OK) return rc;
    std::vector<uint64_t> setCount(lshCount);
    rc = signatureStatisticsToHost(dSig.as<uint64_t>(), cellCount, lshCount, setCount.data());
    if (rc != EM2_OK) return rc;
    dSig.release();

    const std::string prefix = directory && directory[0] ? std::string(directory) + "/" : std::string();
    const size_t groupCount = groups.cellOffsets.size() - 1u;
    // :1428-1435: (signature, size) in map order, std::sort by size descending -- not stable: the host's own std::sort
    std::vector<std::pair<uint64_t, uint64_t>> table(groupCount);
    for (size_t g = 0; g < groupCount; ++g) table[g] = std::make_pair(uint64_t(g), groups.cellOffsets[g + 1u] - groups.cellOffsets[g]);
    std::sort(table.begin(), table.end(),
              [](const std::pair<uint64_t, uint64_t>& x, const std::pair<uint64_t, uint64_t>& y) { return x.second > y.second; });
    {
        const std::string path = prefix + "Signatures.csv";                                  // :1440-1447
        std::ofstream csv(path);
        if (!csv) return fail(EM2_ERROR_RUNTIME, std::string(who) + ": cannot open " + path);
        std::string line(size_t(lshCount), '_');
        for (const std::pair<uint64_t, uint64_t>& p : table) {
            const uint64_t* signature = groups.vertexSignatures.data() + size_t(p.first) * words;
            for (uint32_t i = 0; i < lshCount; ++i) line[i] = (signature[i >> 6] >> (63u - (i & 63u))) & 1u ? 'x' : '_';
            csv << line << "," << p.second << "\n";
        }
    }
    {
        const std::string path = prefix + "Histogram.csv";                                   // :1451-1467
        std::ofstream csv(path);
        if (!csv) return fail(EM2_ERROR_RUNTIME, std::string(who) + ": cannot open " + path);
        std::map<uint64_t, uint64_t> groupsOfSize;               // the sizes that occur, ascending
        for (size_t g = 0; g < groupCount; ++g) groupsOfSize[groups.cellOffsets[g + 1u] - groups.cellOffsets[g]] += 1u;
        uint64_t cellsSoFar = 0;
        for (const std::pair<const uint64_t, uint64_t>& entry : groupsOfSize) {
            cellsSoFar += entry.first * entry.second;
            csv << entry.first << "," << entry.second << "," << entry.first * entry.second << "," << cellsSoFar << "\n";
        }
    }
    {
        const std::string path = prefix + "LshSignatureStatistics.csv";                      // src/Lsh.cpp:284-301
        std::ofstream csv(path);
        if (!csv) return fail(EM2_ERROR_RUNTIME, std::string(who) + ": cannot open " + path);
        csv << "Bit,Set,Unset,Total\n";
        for (uint32_t i = 0; i < lshCount; ++i) {
            csv << i << "," << setCount[i] << "," << uint64_t(cellCount) - setCount[i] << "," << cellCount << "\n";
        }
    }
    return EM2_OK;
}

}  // extern "C"
