// em2_graph_compare.hip -- two things that walk every edge of a cell graph and end in a set of integer pairs:
//
// compareCellGraphs (src/ExpressionMatrixHttpServerGraphs.cpp:104-345) without its page: what the reference does with two
// std::map<pair<CellId, CellId>, float>, a std::map<float, size_t> and a std::set_intersection, as a sort-and-join.
//   edgeKeysKernel       per graph: the two cell ids of an edge, smaller first, as key = cellA << b | cellB (b: the bits of the
//                        largest cell id of both vertex lists); a vertex index is tested before an address is formed with it;
//   a stable radix sort of (key, similarity) over the 2 b bits of the key, headFlagsKernel, an inclusive scan and
//   distinctKernel: the head of every run of equal keys is what map::insert kept (the first in edge order);
//   joinKernel           one lane per distinct key of graph 0, a binary search in graph 1's distinct keys; the three counters
//                        are per-lane sums, added over the wave and sent with one atomic per wave; the bin of a common edge,
//                        0.01f * roundf((s1 - s0) / 0.01f) in float operations, is counted in a private 32-bit table per
//                        workgroup in LDS where |r| <= 2048 (added to a 64-bit table in memory with integer atomics), and is
//                        appended to a list otherwise (r can be +-inf); the list is sorted and its runs are the other bins;
//   the zero bin's sign  is the sign of the product of the first common edge (in key order) that falls into it -- the key a
//                        std::map<float, ...> keeps is the one inserted first --: an atomic minimum over rank << 1 | sign;
//   intersectionKernel   both vertex lists sorted; at the head of every run of list 0 the smaller of the two run lengths.
// Integer sums and minima only: nothing depends on the order in which the lanes arrive.
//
// CellGraph::assignColorsToGroups (src/CellGraph.cpp:794-862): groupIdsKernel writes (group[v0], group[v1]) per edge,
// em2_dev_contingency (em2_contingency.hip) makes the sparse table of those pairs, and the host folds it over its diagonal
// and colours the groups (em2_graph_compare_host.h).

#include "em2_adjacency.h"
#include "em2_entry.h"
#include "em2_graph_compare_host.h"
#include "em2_primitives.h"
#include "em2_runs.h"
#include "em2_scratch.h"
#include "em2_wave.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

namespace em2 {

constexpr int kComparePathTable = 0;               // the LDS table, the list for what it does not hold
constexpr int kComparePathList = 1;                // every common edge through the list

struct GraphCompareResult {
    uint64_t commonVertexCount = 0;
    uint64_t edgeCount0 = 0, edgeCount1 = 0;       // distinct unordered cell pairs: the sizes of the reference's two maps
    uint64_t commonEdgeCount = 0, commonIdenticalEdgeCount = 0;
    std::vector<float> binDelta;
    std::vector<uint64_t> binCount;
    int path = 0;
};

// What stops a comparison, for the entry point to put into words.
struct GraphCompareError {
    enum Kind { none, vertexIndex, selfLoop, notANumber } kind = none;
    int graph = 0;                                 // vertexIndex, selfLoop: the graph
    uint64_t edge = 0;                             // ... and its first edge that has it
    uint32_t cellA = 0, cellB = 0;                 // selfLoop (cellA), notANumber: the cells of the edge
};

namespace {

typedef unsigned long long u64;

constexpr uint32_t kCompareMaxBlocks = 1024;       // of every grid here: four workgroups for each of the 256 CUs

// Blocks of 256 threads for n items, at least 1 and at most kCompareMaxBlocks (the kernels stride over the grid).
inline uint32_t compareGrid(uint64_t n)
{
    const uint64_t blocks = (n + 255u) / 256u;
    return uint32_t(blocks > kCompareMaxBlocks ? kCompareMaxBlocks : (blocks ? blocks : 1u));
}

// The bits that hold every value up to `largest`, at least 1.
inline uint32_t bitWidth(uint32_t largest)
{
    uint32_t bits = 1;
    while (bits < 32u && (largest >> bits) != 0u) bits++;
    return bits;
}

__device__ __forceinline__ u64 waveSumU64(u64 value)
{
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) value += __shfl_xor(value, step, 64);
    return value;
}

__device__ __forceinline__ u64 waveMinU64(u64 value)
{
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        const u64 other = __shfl_xor(value, step, 64);
        value = other < value ? other : value;
    }
    return value;
}

// The words a comparison keeps in device memory.  (u64: the type of HIP's 64-bit atomics.)
struct CompareWords {
    u64 error[2];              // per graph: bit 0 a vertex index out of range, bit 1 an edge between a cell and itself
    u64 firstBadIndex[2];      // per graph: the first edge with the one ...
    u64 firstSelfLoop[2];      // ... and with the other (minima; ~0 for none)
    u64 commonVertices;
    u64 commonEdges, identicalEdges;
    u64 zeroFirst;             // min of rank << 1 | sign over the common edges of the zero bin (~0 for none)
    u64 nanFirst;              // min of the rank of a common edge whose difference is not a number (~0 for none)
    u64 listCount;             // products in the list
};

// keys[e] = cellA << bits | cellB with cellA < cellB the cells of edge e's two vertices; sims[e] = similarity[e].  An edge with a
// vertex index that is not below vertexCount (tested before the cell id is loaded) or with twice the same cell writes nothing
// and raises the graph's error word.
__global__ void __launch_bounds__(256)
edgeKeysKernel(const uint32_t* __restrict__ cells, uint32_t vertexCount, const uint32_t* __restrict__ v0, const uint32_t* __restrict__ v1,
               const float* __restrict__ similarity, uint64_t edgeCount, uint32_t bits, int graph, uint64_t* __restrict__ keys,
               float* __restrict__ sims, CompareWords* __restrict__ words)
{
    for (uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < edgeCount; e += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t a = v0[e], b = v1[e];
        if (a >= vertexCount || b >= vertexCount) {
            atomicOr(&words->error[graph], u64(1));
            atomicMin(&words->firstBadIndex[graph], u64(e));
            continue;
        }
        const uint32_t cellA = cells[a], cellB = cells[b];
        if (cellA == cellB) {
            atomicOr(&words->error[graph], u64(2));
            atomicMin(&words->firstSelfLoop[graph], u64(e));
            continue;
        }
        const uint32_t low = cellA < cellB ? cellA : cellB, high = cellA < cellB ? cellB : cellA;
        keys[e] = uint64_t(low) << bits | high;
        sims[e] = similarity[e];
    }
}

// The head of run r = rank[i] - 1 of the sorted keys: its key and the similarity that came first in edge order.
__global__ void __launch_bounds__(256)
distinctKernel(const uint64_t* __restrict__ keys, const float* __restrict__ sims, const uint32_t* __restrict__ flags,
               const uint32_t* __restrict__ rank, uint64_t n, uint64_t* __restrict__ distinctKeys, float* __restrict__ distinctSims)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (!flags[i]) continue;
        const uint32_t r = rank[i] - 1u;                         // (rank[i] in [1, i + 1]: r <= i < n, the arrays' size)
        distinctKeys[r] = keys[i];
        distinctSims[r] = sims[i];
    }
}

__global__ void __launch_bounds__(256)
widenKernel(const uint32_t* __restrict__ in, uint64_t n, uint64_t* __restrict__ out)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) out[i] = in[i];
}

// std::set_intersection of the two ascending lists, counted: an id that a[] holds x times and b[] y times counts min(x, y).
__global__ void __launch_bounds__(256)
intersectionKernel(const uint64_t* __restrict__ a, uint64_t na, const uint64_t* __restrict__ b, uint64_t nb, CompareWords* __restrict__ words)
{
    u64 mine = 0;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < na; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t id = a[i];
        if (i != 0 && a[i - 1] == id) continue;
        const uint64_t first = lowerBound(b, nb, id);
        if (first == nb || b[first] != id) continue;
        const uint64_t inA = lowerBound(a, na, id + 1u) - i;     // (ids are below 2^32: id + 1 does not wrap)
        const uint64_t inB = lowerBound(b, nb, id + 1u) - first;
        mine += inA < inB ? inA : inB;
    }
    mine = waveSumU64(mine);
    if ((threadIdx.x & 63u) == 0u && mine) atomicAdd(&words->commonVertices, mine);
}

// A float as a 32-bit key that ascends with it (-inf lowest, +inf highest; no NaN comes here).
__device__ __forceinline__ uint32_t ascendingBits(float x)
{
    const uint32_t bits = __float_as_uint(x);
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// One lane per distinct key of graph 0.  UseTable: the bins with |r| <= kCompareTableRadius are counted in LDS and added to
// table[kCompareTableBins]; every other product (all of them without UseTable) goes to list[] as ascendingBits of it, the two
// zeros as +0, at a position from words->listCount (one atomic per wave and trip).  list has room for n0 entries.
template <bool UseTable>
__global__ void __launch_bounds__(256)
joinKernel(const uint64_t* __restrict__ keys0, const float* __restrict__ sims0, uint64_t n0, const uint64_t* __restrict__ keys1,
           const float* __restrict__ sims1, uint64_t n1, u64* __restrict__ table, uint64_t* __restrict__ list,
           CompareWords* __restrict__ words)
{
    __shared__ uint32_t counters[UseTable ? kCompareTableBins : 1u];
    if (UseTable) {
        for (uint32_t c = threadIdx.x; c < kCompareTableBins; c += 256u) counters[c] = 0u;
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u;
    u64 common = 0, identical = 0, zeroFirst = ~u64(0), nanFirst = ~u64(0);
    // (every lane of the block makes the same number of trips: the ballot below is of whole waves)
    for (uint64_t base = uint64_t(blockIdx.x) * 256u; base < n0; base += uint64_t(gridDim.x) * 256u) {
        const uint64_t i = base + threadIdx.x;
        bool toList = false;
        float product = 0.0f;
        if (i < n0) {
            const uint64_t key = keys0[i];
            const uint64_t at = lowerBound(keys1, n1, key);
            if (at < n1 && keys1[at] == key) {
                const float s0 = sims0[i], s1 = sims1[at];
                common++;
                if (s0 == s1) identical++;
                const float delta = s1 - s0;
                if (delta != delta) {
                    nanFirst = i < nanFirst ? i : nanFirst;
                } else {
                    const float r = roundf(delta / 0.01f);
                    product = 0.01f * r;
                    if (r == 0.0f) {
                        const u64 mark = u64(i) << 1 | (__float_as_uint(product) >> 31);
                        zeroFirst = mark < zeroFirst ? mark : zeroFirst;
                        product = 0.0f;
                    }
                    if (UseTable && fabsf(r) <= float(kCompareTableRadius)) atomicAdd(&counters[int(r) + kCompareTableRadius], 1u);
                    else toList = true;
                }
            }
        }
        const uint64_t mask = __ballot(toList);
        if (mask) {
            const int leader = __ffsll((long long)mask) - 1;
            uint32_t first = 0;
            if (int(lane) == leader) first = uint32_t(atomicAdd(&words->listCount, u64(__popcll(mask))));   // (below n0 < 2^32)
            first = uint32_t(__shfl(int(first), leader, 64));
            if (toList) list[first + lanesBelow(mask)] = ascendingBits(product);
        }
    }
    common = waveSumU64(common);
    identical = waveSumU64(identical);
    zeroFirst = waveMinU64(zeroFirst);
    nanFirst = waveMinU64(nanFirst);
    if (lane == 0u) {
        if (common) atomicAdd(&words->commonEdges, common);
        if (identical) atomicAdd(&words->identicalEdges, identical);
        if (zeroFirst != ~u64(0)) atomicMin(&words->zeroFirst, zeroFirst);
        if (nanFirst != ~u64(0)) atomicMin(&words->nanFirst, nanFirst);
    }
    if (UseTable) {
        __syncthreads();
        for (uint32_t c = threadIdx.x; c < kCompareTableBins; c += 256u) {
            const uint32_t v = counters[c];
            if (v) atomicAdd(&table[c], u64(v));
        }
    }
}

// The head of run r of the sorted list: its key and where it begins.
__global__ void __launch_bounds__(256)
listRunsKernel(const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ rank, uint64_t n,
               uint32_t* __restrict__ runKey, uint32_t* __restrict__ runStart)
{
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += uint64_t(gridDim.x) * blockDim.x) {
        if (!flags[i]) continue;
        const uint32_t r = rank[i] - 1u;                         // (r <= i < n, the arrays' size)
        runKey[r] = uint32_t(sorted[i]);
        runStart[r] = uint32_t(i);
    }
}

// id0[e] = group[v0[e]], id1[e] = group[v1[e]]; an edge with a vertex index that is not below vertexCount writes nothing and
// raises *error.
__global__ void __launch_bounds__(256)
groupIdsKernel(const uint32_t* __restrict__ group, uint32_t vertexCount, const uint32_t* __restrict__ v0, const uint32_t* __restrict__ v1,
               uint64_t edgeCount, uint32_t* __restrict__ id0, uint32_t* __restrict__ id1, uint32_t* __restrict__ error)
{
    bool bad = false;
    for (uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < edgeCount; e += uint64_t(gridDim.x) * blockDim.x) {
        const uint32_t a = v0[e], b = v1[e];
        if (a < vertexCount && b < vertexCount) {
            id0[e] = group[a];
            id1[e] = group[b];
        } else bad = true;
    }
    if (bad) atomicOr(error, 1u);
}

template <class T> hipError_t toHost(std::vector<T>& to, const void* from, size_t count, hipStream_t stream)
{
    to.resize(count);
    if (count == 0) return hipSuccess;
    return hipMemcpyAsync(to.data(), from, count * sizeof(T), hipMemcpyDeviceToHost, stream);
}

struct CompareGraph {
    const uint32_t* vertexCellIds;     // host
    uint32_t vertexCount;
    const uint32_t* d_v0;              // device
    const uint32_t* d_v1;
    const float* d_similarity;
    uint64_t edgeCount;                // below 2^32
};

}  // namespace

// The comparison of two graphs whose edge arrays are in device memory (the caller has checked the pointers and that both edge
// counts are below 2^32).  path: kComparePathTable or kComparePathList.  Where `error.kind` is set, `out` holds nothing.
// Takes its scratch from the cache of em2_scratch.h; synchronises the stream.
static hipError_t runGraphCompare(const CompareGraph (&graphs)[2], int path, GraphCompareResult& out, GraphCompareError& error,
                                  hipStream_t stream)
{
    out = GraphCompareResult();
    out.path = path;
    error = GraphCompareError();
    StageTimer timer("compareCellGraphs");
    const dim3 threads(256);

    uint32_t largestCell = 0;
    for (const CompareGraph& g : graphs) {
        for (uint32_t v = 0; v < g.vertexCount; v++) largestCell = std::max(largestCell, g.vertexCellIds[v]);
    }
    const uint32_t bits = bitWidth(largestCell);
    const uint64_t mostEdges = std::max(graphs[0].edgeCount, graphs[1].edgeCount);
    const uint64_t listCapacity = graphs[0].edgeCount;

    ArenaPlan plan;
    const size_t offWords = plan.take(sizeof(CompareWords));
    const size_t offTable = plan.takeFor<u64>(kCompareTableBins);
    size_t offCells[2], offWide[2][2], offDistinctKeys[2], offDistinctSims[2];
    for (int g = 0; g < 2; g++) {
        offCells[g] = plan.takeFor<uint32_t>(graphs[g].vertexCount);
        offWide[g][0] = plan.takeFor<uint64_t>(graphs[g].vertexCount);
        offWide[g][1] = plan.takeFor<uint64_t>(graphs[g].vertexCount);
        offDistinctKeys[g] = plan.takeFor<uint64_t>(graphs[g].edgeCount);
        offDistinctSims[g] = plan.takeFor<float>(graphs[g].edgeCount);
    }
    const size_t offKeysA = plan.takeFor<uint64_t>(mostEdges);
    const size_t offKeysB = plan.takeFor<uint64_t>(mostEdges);
    const size_t offSimsA = plan.takeFor<float>(mostEdges);
    const size_t offSimsB = plan.takeFor<float>(mostEdges);
    const size_t offFlags = plan.takeFor<uint32_t>(mostEdges);
    const size_t offRank = plan.takeFor<uint32_t>(mostEdges);
    const size_t offListA = plan.takeFor<uint64_t>(listCapacity);
    const size_t offListB = plan.takeFor<uint64_t>(listCapacity);
    const size_t offRunKey = plan.takeFor<uint32_t>(listCapacity);
    const size_t offRunStart = plan.takeFor<uint32_t>(listCapacity);
    size_t tempBytes = 0;
    {
        size_t bytes = 0;
        for (int g = 0; g < 2; g++) {
            if (graphs[g].edgeCount) {
                EM2_TRY(sortPairsU64F32BufferBytes(size_t(graphs[g].edgeCount), 0u, 2u * bits, bytes));
                tempBytes = std::max(tempBytes, bytes);
                EM2_TRY(inclusiveScanBytes(size_t(graphs[g].edgeCount), bytes));
                tempBytes = std::max(tempBytes, bytes);
            }
            if (graphs[g].vertexCount) {
                EM2_TRY(sortKeysBufferBytes(size_t(graphs[g].vertexCount), 0u, bits, bytes));
                tempBytes = std::max(tempBytes, bytes);
            }
        }
        if (listCapacity) {
            EM2_TRY(sortKeysBufferBytes(size_t(listCapacity), 0u, 32u, bytes));
            tempBytes = std::max(tempBytes, bytes);
        }
    }
    const size_t offTemp = plan.take(tempBytes);

    CachedBuffer arena;
    EM2_TRY(arena.allocate(plan.bytes));
    char* base = arena.as<char>();
    CompareWords* words = arenaAt<CompareWords>(base, offWords);
    u64* table = arenaAt<u64>(base, offTable);
    uint32_t* flags = arenaAt<uint32_t>(base, offFlags);
    uint32_t* rank = arenaAt<uint32_t>(base, offRank);
    void* temp = base + offTemp;

    CompareWords host = CompareWords();
    host.firstBadIndex[0] = host.firstBadIndex[1] = host.firstSelfLoop[0] = host.firstSelfLoop[1] = ~u64(0);
    host.zeroFirst = host.nanFirst = ~u64(0);
    EM2_TRY(hipMemcpyAsync(words, &host, sizeof(host), hipMemcpyHostToDevice, stream));
    EM2_TRY(hipMemsetAsync(table, 0, kCompareTableBins * sizeof(u64), stream));
    for (int g = 0; g < 2; g++) {
        if (!graphs[g].vertexCount) continue;
        EM2_TRY(hipMemcpyAsync(base + offCells[g], graphs[g].vertexCellIds, size_t(graphs[g].vertexCount) * sizeof(uint32_t),
                               hipMemcpyHostToDevice, stream));
    }

    // ---- per graph: keys, the stable sort, the distinct keys ----
    const uint64_t* distinctKeys[2];
    const float* distinctSims[2];
    uint64_t distinctCount[2] = {0, 0};
    for (int g = 0; g < 2; g++) {
        const CompareGraph& graph = graphs[g];
        const uint64_t n = graph.edgeCount;
        uint64_t* dKeys = arenaAt<uint64_t>(base, offDistinctKeys[g]);
        float* dSims = arenaAt<float>(base, offDistinctSims[g]);
        distinctKeys[g] = dKeys;
        distinctSims[g] = dSims;
        if (n == 0) continue;
        DoubleBuffer<uint64_t> keys{arenaAt<uint64_t>(base, offKeysA), arenaAt<uint64_t>(base, offKeysB)};
        DoubleBuffer<float> sims{arenaAt<float>(base, offSimsA), arenaAt<float>(base, offSimsB)};
        edgeKeysKernel<<<dim3(compareGrid(n)), threads, 0, stream>>>(arenaAt<uint32_t>(base, offCells[g]), graph.vertexCount, graph.d_v0,
                                                                     graph.d_v1, graph.d_similarity, n, bits, g, keys.current(),
                                                                     sims.current(), words);
        EM2_TRY(hipGetLastError());
        // an edge that failed wrote no key: nothing below may use what the kernel left
        EM2_TRY(hipMemcpyAsync(&host, words, sizeof(host), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        if (host.error[g]) {
            arena.idle = true;
            error.graph = g;
            if (host.error[g] & 1u) {
                error.kind = GraphCompareError::vertexIndex;
                error.edge = host.firstBadIndex[g];
            } else {
                error.kind = GraphCompareError::selfLoop;
                error.edge = host.firstSelfLoop[g];
                uint32_t v = 0;
                EM2_TRY(hipMemcpy(&v, graph.d_v0 + error.edge, sizeof(v), hipMemcpyDeviceToHost));
                error.cellA = error.cellB = graph.vertexCellIds[v];          // (v passed the kernel's test)
            }
            return hipSuccess;
        }
        EM2_TRY(timer.stage("keys", stream));
        EM2_TRY(sortPairs(temp, tempBytes, keys, sims, size_t(n), 0u, 2u * bits, stream));
        EM2_TRY(timer.stage("sort", stream));
        headFlagsKernel<<<dim3(compareGrid(n)), threads, 0, stream>>>(keys.current(), n, flags);
        EM2_TRY(hipGetLastError());
        EM2_TRY(inclusiveScan(temp, tempBytes, flags, rank, size_t(n), stream));
        distinctKernel<<<dim3(compareGrid(n)), threads, 0, stream>>>(keys.current(), sims.current(), flags, rank, n, dKeys, dSims);
        EM2_TRY(hipGetLastError());
        uint32_t runs = 0;
        EM2_TRY(hipMemcpyAsync(&runs, rank + (n - 1u), sizeof(runs), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        if (runs == 0u || runs > n) {
            arena.idle = true;
            return hipErrorUnknown;
        }
        distinctCount[g] = runs;
        EM2_TRY(timer.stage("distinct keys", stream));
    }
    out.edgeCount0 = distinctCount[0];
    out.edgeCount1 = distinctCount[1];

    // ---- the common vertices ----
    if (graphs[0].vertexCount && graphs[1].vertexCount) {
        DoubleBuffer<uint64_t> ids[2] = {{arenaAt<uint64_t>(base, offWide[0][0]), arenaAt<uint64_t>(base, offWide[0][1])},
                                         {arenaAt<uint64_t>(base, offWide[1][0]), arenaAt<uint64_t>(base, offWide[1][1])}};
        for (int g = 0; g < 2; g++) {
            const uint64_t n = graphs[g].vertexCount;
            widenKernel<<<dim3(compareGrid(n)), threads, 0, stream>>>(arenaAt<uint32_t>(base, offCells[g]), n, ids[g].current());
            EM2_TRY(hipGetLastError());
            EM2_TRY(sortKeys(temp, tempBytes, ids[g], size_t(n), 0u, bits, stream));
        }
        intersectionKernel<<<dim3(compareGrid(graphs[0].vertexCount)), threads, 0, stream>>>(ids[0].current(), graphs[0].vertexCount,
                                                                                            ids[1].current(), graphs[1].vertexCount, words);
        EM2_TRY(hipGetLastError());
        EM2_TRY(timer.stage("common vertices", stream));
    }

    // ---- the join and the histogram ----
    DoubleBuffer<uint64_t> list{arenaAt<uint64_t>(base, offListA), arenaAt<uint64_t>(base, offListB)};
    if (distinctCount[0] && distinctCount[1]) {
        const dim3 grid(compareGrid(distinctCount[0]));
        if (path == kComparePathTable) {
            joinKernel<true><<<grid, threads, 0, stream>>>(distinctKeys[0], distinctSims[0], distinctCount[0], distinctKeys[1], distinctSims[1],
                                                           distinctCount[1], table, list.current(), words);
        } else {
            joinKernel<false><<<grid, threads, 0, stream>>>(distinctKeys[0], distinctSims[0], distinctCount[0], distinctKeys[1], distinctSims[1],
                                                            distinctCount[1], table, list.current(), words);
        }
        EM2_TRY(hipGetLastError());
    }
    EM2_TRY(hipMemcpyAsync(&host, words, sizeof(host), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(timer.stage("join and histogram", stream));
    if (host.nanFirst != ~u64(0)) {
        uint64_t key = 0;
        if (host.nanFirst >= distinctCount[0]) {
            arena.idle = true;
            return hipErrorUnknown;
        }
        EM2_TRY(hipMemcpy(&key, distinctKeys[0] + host.nanFirst, sizeof(key), hipMemcpyDeviceToHost));
        arena.idle = true;
        error.kind = GraphCompareError::notANumber;
        error.cellA = uint32_t(key >> bits);
        error.cellB = uint32_t(bits == 32u ? key & 0xffffffffull : key & ((uint64_t(1) << bits) - 1u));
        return hipSuccess;
    }
    if (host.listCount > listCapacity) {
        arena.idle = true;
        return hipErrorUnknown;
    }

    // ---- the list's bins ----
    std::vector<float> listDelta;
    std::vector<uint64_t> listBinCount;
    if (host.listCount) {
        const uint64_t n = host.listCount;
        uint32_t* runKey = arenaAt<uint32_t>(base, offRunKey);
        uint32_t* runStart = arenaAt<uint32_t>(base, offRunStart);
        EM2_TRY(sortKeys(temp, tempBytes, list, size_t(n), 0u, 32u, stream));
        headFlagsKernel<<<dim3(compareGrid(n)), threads, 0, stream>>>(list.current(), n, flags);     // (n <= edgeCount0 <= mostEdges)
        EM2_TRY(hipGetLastError());
        EM2_TRY(inclusiveScan(temp, tempBytes, flags, rank, size_t(n), stream));
        listRunsKernel<<<dim3(compareGrid(n)), threads, 0, stream>>>(list.current(), flags, rank, n, runKey, runStart);
        EM2_TRY(hipGetLastError());
        uint32_t runs = 0;
        EM2_TRY(hipMemcpyAsync(&runs, rank + (n - 1u), sizeof(runs), hipMemcpyDeviceToHost, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        if (runs == 0u || runs > n) {
            arena.idle = true;
            return hipErrorUnknown;
        }
        std::vector<uint32_t> keys, starts;
        EM2_TRY(toHost(keys, runKey, runs, stream));
        EM2_TRY(toHost(starts, runStart, runs, stream));
        EM2_TRY(hipStreamSynchronize(stream));
        for (uint32_t r = 0; r < runs; r++) {
            const uint32_t key = keys[r];
            listDelta.push_back(floatOfBits((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key));       // ascendingBits backwards
            listBinCount.push_back((r + 1u < runs ? uint64_t(starts[r + 1u]) : n) - starts[r]);
        }
        EM2_TRY(timer.stage("list bins", stream));
    }
    std::vector<u64> hostTable;
    if (path == kComparePathTable) {
        EM2_TRY(toHost(hostTable, table, kCompareTableBins, stream));
        EM2_TRY(hipStreamSynchronize(stream));
    }
    arena.idle = true;                                                      // (everything that used the block has been waited for)

    static_assert(sizeof(u64) == sizeof(uint64_t), "the table is read as uint64_t");
    mergeCompareBins(hostTable.empty() ? nullptr : reinterpret_cast<const uint64_t*>(hostTable.data()), listDelta, listBinCount,
                     host.zeroFirst != ~u64(0) && (host.zeroFirst & 1u), out.binDelta, out.binCount);
    out.commonVertexCount = host.commonVertices;
    out.commonEdgeCount = host.commonEdges;
    out.commonIdenticalEdgeCount = host.identicalEdges;
    return hipSuccess;
}

struct GroupColorsResult {
    uint32_t groupCount = 0;
    int contingencyPath = 0;                       // of em2_dev_contingency: 1 or 2; 0 where it did not run (no edges or no groups)
    std::vector<uint32_t> pair0, pair1;            // the group graph: g0 < g1, ascending
    std::vector<uint64_t> pairEdges;               // the cell-graph edges between the two groups
    std::vector<uint32_t> colorTable;
};

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

struct em2_graph_comparison {
    em2::GraphCompareResult result;
};

static int graphCompareCreate(const char* who, bool edgesOnDevice, const uint32_t* const* vertexCellIds, const uint32_t* vertexCount,
                              const uint32_t* const* v0, const uint32_t* const* v1, const float* const* similarity,
                              const uint64_t* edgeCount, int path, em2_graph_comparison** out)
{
    if (!out) return failNull(who);
    *out = nullptr;
    for (int g = 0; g < 2; g++) {
        if (vertexCount[g] && !vertexCellIds[g]) return failNull(who);
        if (edgeCount[g] && (!v0[g] || !v1[g] || !similarity[g])) return failNull(who);
    }
    if (path != em2::kComparePathTable && path != em2::kComparePathList) {
        return failArgument(who, "path must be 0 (the LDS table, the list for the rest) or 1 (every common edge through the list)");
    }
    // (a run's first element and a key's rank are kept in 32 bits)
    if (edgeCount[0] > 0xffffffffull || edgeCount[1] > 0xffffffffull) {
        return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 1 edges in a graph are not supported");
    }
    if (!haveDevice()) return failNoDevice(who);
    DeviceBuffer uploaded[2][3];
    em2::CompareGraph graphs[2];
    for (int g = 0; g < 2; g++) {
        graphs[g] = em2::CompareGraph{vertexCellIds[g], vertexCount[g], v0[g], v1[g], similarity[g], edgeCount[g]};
        if (!edgesOnDevice && edgeCount[g]) {
            EM2_HIP(uploaded[g][0].upload(v0[g], size_t(edgeCount[g])));
            EM2_HIP(uploaded[g][1].upload(v1[g], size_t(edgeCount[g])));
            EM2_HIP(uploaded[g][2].upload(similarity[g], size_t(edgeCount[g])));
            graphs[g].d_v0 = uploaded[g][0].as<uint32_t>();
            graphs[g].d_v1 = uploaded[g][1].as<uint32_t>();
            graphs[g].d_similarity = uploaded[g][2].as<float>();
        }
    }
    std::unique_ptr<em2_graph_comparison> c(new em2_graph_comparison);
    em2::GraphCompareError error;
    EM2_HIP_FOR(who, em2::runGraphCompare(graphs, path, c->result, error, nullptr));
    const std::string where = std::string(who) + ": graph " + std::to_string(error.graph) + ", edge " + std::to_string(error.edge);
    switch (error.kind) {
    case em2::GraphCompareError::vertexIndex:
        return fail(EM2_ERROR_INVALID_ARGUMENT, where + ": a vertex index is not below the vertex count");
    case em2::GraphCompareError::selfLoop:
        return fail(EM2_ERROR_RUNTIME, where + ": cellIdA != cellIdB (both ends are cell " + std::to_string(error.cellA) + ")");
    case em2::GraphCompareError::notANumber:
        return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": the similarity difference of the common edge between cells " +
                                               std::to_string(error.cellA) + " and " + std::to_string(error.cellB) +
                                               " is not a number (it cannot key the reference's histogram)");
    case em2::GraphCompareError::none:
        break;
    }
    *out = c.release();
    return EM2_OK;
}

int em2_cell_graph_compare(const uint32_t* vertexCellIds0, uint32_t vertexCount0, const uint32_t* edgeVertex0_0, const uint32_t* edgeVertex1_0,
                           const float* edgeSimilarity0, uint64_t edgeCount0, const uint32_t* vertexCellIds1, uint32_t vertexCount1,
                           const uint32_t* edgeVertex0_1, const uint32_t* edgeVertex1_1, const float* edgeSimilarity1, uint64_t edgeCount1,
                           int path, em2_graph_comparison** comparison)
{
    const uint32_t* cells[2] = {vertexCellIds0, vertexCellIds1};
    const uint32_t counts[2] = {vertexCount0, vertexCount1};
    const uint32_t* v0[2] = {edgeVertex0_0, edgeVertex0_1};
    const uint32_t* v1[2] = {edgeVertex1_0, edgeVertex1_1};
    const float* similarity[2] = {edgeSimilarity0, edgeSimilarity1};
    const uint64_t edges[2] = {edgeCount0, edgeCount1};
    return graphCompareCreate("em2_cell_graph_compare", false, cells, counts, v0, v1, similarity, edges, path, comparison);
}

int em2_dev_cell_graph_compare(const uint32_t* vertexCellIds0, uint32_t vertexCount0, const uint32_t* d_edgeVertex0_0,
                               const uint32_t* d_edgeVertex1_0, const float* d_edgeSimilarity0, uint64_t edgeCount0,
                               const uint32_t* vertexCellIds1, uint32_t vertexCount1, const uint32_t* d_edgeVertex0_1,
                               const uint32_t* d_edgeVertex1_1, const float* d_edgeSimilarity1, uint64_t edgeCount1, int path,
                               em2_graph_comparison** comparison)
{
    const uint32_t* cells[2] = {vertexCellIds0, vertexCellIds1};
    const uint32_t counts[2] = {vertexCount0, vertexCount1};
    const uint32_t* v0[2] = {d_edgeVertex0_0, d_edgeVertex0_1};
    const uint32_t* v1[2] = {d_edgeVertex1_0, d_edgeVertex1_1};
    const float* similarity[2] = {d_edgeSimilarity0, d_edgeSimilarity1};
    const uint64_t edges[2] = {edgeCount0, edgeCount1};
    return graphCompareCreate("em2_dev_cell_graph_compare", true, cells, counts, v0, v1, similarity, edges, path, comparison);
}

int em2_graph_comparison_sizes(const em2_graph_comparison* comparison, uint64_t* commonVertexCount, uint64_t* edgeCount0,
                               uint64_t* edgeCount1, uint64_t* commonEdgeCount, uint64_t* commonIdenticalEdgeCount, uint64_t* binCount,
                               int* path)
{
    if (!comparison) return failNull("em2_graph_comparison_sizes");
    const em2::GraphCompareResult& r = comparison->result;
    if (commonVertexCount) *commonVertexCount = r.commonVertexCount;
    if (edgeCount0) *edgeCount0 = r.edgeCount0;
    if (edgeCount1) *edgeCount1 = r.edgeCount1;
    if (commonEdgeCount) *commonEdgeCount = r.commonEdgeCount;
    if (commonIdenticalEdgeCount) *commonIdenticalEdgeCount = r.commonIdenticalEdgeCount;
    if (binCount) *binCount = r.binDelta.size();
    if (path) *path = r.path;
    return EM2_OK;
}

int em2_graph_comparison_get(const em2_graph_comparison* comparison, float* binDelta, uint64_t* binCount)
{
    if (!comparison) return failNull("em2_graph_comparison_get");
    const em2::GraphCompareResult& r = comparison->result;
    if (binDelta) std::copy(r.binDelta.begin(), r.binDelta.end(), binDelta);
    if (binCount) std::copy(r.binCount.begin(), r.binCount.end(), binCount);
    return EM2_OK;
}

void em2_graph_comparison_free(em2_graph_comparison* comparison) { delete comparison; }


struct em2_group_colors {
    em2::GroupColorsResult result;
};

static int groupColorsCreate(const char* who, bool edgesOnDevice, const uint32_t* vertexGroup, uint32_t vertexCount, const uint32_t* v0,
                             const uint32_t* v1, uint64_t edgeCount, int path, em2_group_colors** out)
{
    if (!out) return failNull(who);
    *out = nullptr;
    if ((vertexCount && !vertexGroup) || (edgeCount && (!v0 || !v1))) return failNull(who);
    if (path < 0 || path > 2) return failArgument(who, "path must be 0 (automatic), 1 (LDS) or 2 (sort)");
    if (edgeCount > 0xffffffffull) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": more than 2^32 - 1 edges are not supported");
    uint32_t largest = 0;
    for (uint32_t v = 0; v < vertexCount; v++) largest = std::max(largest, vertexGroup[v]);
    if (vertexCount && largest == 0xffffffffu) return failArgument(who, "a group id of 2^32 - 1 leaves no room for the group count");
    const uint32_t groupCount = vertexCount ? largest + 1u : 0u;
    if (!haveDevice()) return failNoDevice(who);
    std::unique_ptr<em2_group_colors> c(new em2_group_colors);
    em2::GroupColorsResult& r = c->result;
    r.groupCount = groupCount;
    if (edgeCount && !vertexCount) return failArgument(who, "a vertex index is not below the vertex count");
    if (edgeCount) {
        DeviceBuffer d0, d1, group, ids, error;
        if (!edgesOnDevice) {
            EM2_HIP(d0.upload(v0, size_t(edgeCount)));
            EM2_HIP(d1.upload(v1, size_t(edgeCount)));
            v0 = d0.as<uint32_t>();
            v1 = d1.as<uint32_t>();
        }
        EM2_HIP(group.upload(vertexGroup, size_t(vertexCount)));
        EM2_HIP(ids.allocateFor<uint32_t>(2u * size_t(edgeCount)));
        uint32_t bad = 0;
        EM2_HIP(error.upload(&bad, 1));
        uint32_t* id0 = ids.as<uint32_t>();
        uint32_t* id1 = id0 + edgeCount;
        em2::groupIdsKernel<<<dim3(em2::compareGrid(edgeCount)), dim3(256), 0, nullptr>>>(group.as<uint32_t>(), vertexCount, v0, v1, edgeCount,
                                                                                          id0, id1, error.as<uint32_t>());
        EM2_HIP(hipGetLastError());
        EM2_HIP(error.download(&bad, 1));                       // (waits for the kernel)
        if (bad) return failArgument(who, "a vertex index is not below the vertex count");
        // the sparse table of the (group, group) pairs: em2_contingency.hip, with its two paths
        em2_contingency* table = nullptr;
        const int status = em2_dev_contingency(id0, id1, edgeCount, groupCount, groupCount, path, &table);
        if (status != EM2_OK) return status;                    // (in em2_dev_contingency's words)
        std::unique_ptr<em2_contingency, void (*)(em2_contingency*)> owner(table, em2_contingency_free);
        uint64_t nonZero = 0;
        if (em2_contingency_sizes(table, nullptr, nullptr, nullptr, &nonZero, &r.contingencyPath) != EM2_OK) return EM2_ERROR_RUNTIME;
        std::vector<uint32_t> i0(nonZero), i1(nonZero);
        std::vector<uint64_t> count(nonZero);
        if (em2_contingency_get(table, nullptr, nullptr, i0.data(), i1.data(), count.data(), nullptr) != EM2_OK) return EM2_ERROR_RUNTIME;
        em2::foldGroupPairs(i0, i1, count, r.pair0, r.pair1, r.pairEdges);
    }
    em2::assignGroupColors(groupCount, r.pair0, r.pair1, r.colorTable);
    *out = c.release();
    return EM2_OK;
}

int em2_graph_group_colors(const uint32_t* vertexGroup, uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1,
                           uint64_t edgeCount, int path, em2_group_colors** colors)
{
    return groupColorsCreate("em2_graph_group_colors", false, vertexGroup, vertexCount, edgeVertex0, edgeVertex1, edgeCount, path, colors);
}

int em2_dev_graph_group_colors(const uint32_t* vertexGroup, uint32_t vertexCount, const uint32_t* d_edgeVertex0,
                               const uint32_t* d_edgeVertex1, uint64_t edgeCount, int path, em2_group_colors** colors)
{
    return groupColorsCreate("em2_dev_graph_group_colors", true, vertexGroup, vertexCount, d_edgeVertex0, d_edgeVertex1, edgeCount, path,
                             colors);
}

int em2_group_colors_sizes(const em2_group_colors* colors, uint32_t* groupCount, uint64_t* pairCount, int* path)
{
    if (!colors) return failNull("em2_group_colors_sizes");
    if (groupCount) *groupCount = colors->result.groupCount;
    if (pairCount) *pairCount = colors->result.pair0.size();
    if (path) *path = colors->result.contingencyPath;
    return EM2_OK;
}

int em2_group_colors_get(const em2_group_colors* colors, uint32_t* pairGroup0, uint32_t* pairGroup1, uint64_t* pairEdgeCount,
                         uint32_t* colorTable)
{
    if (!colors) return failNull("em2_group_colors_get");
    const em2::GroupColorsResult& r = colors->result;
    if (pairGroup0) std::copy(r.pair0.begin(), r.pair0.end(), pairGroup0);
    if (pairGroup1) std::copy(r.pair1.begin(), r.pair1.end(), pairGroup1);
    if (pairEdgeCount) std::copy(r.pairEdges.begin(), r.pairEdges.end(), pairEdgeCount);
    if (colorTable) std::copy(r.colorTable.begin(), r.colorTable.end(), colorTable);
    return EM2_OK;
}

void em2_group_colors_free(em2_group_colors* colors) { delete colors; }

}  // extern "C"
