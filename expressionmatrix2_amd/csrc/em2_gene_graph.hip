// em2_gene_graph.hip -- the GeneGraph constructor (src/GeneGraph.cpp:22-104) behind ExpressionMatrix::createGeneGraph
// (src/ExpressionMatrixGeneGraph.cpp:44-89) and GeneGraph::getConnectivity (src/GeneGraph.cpp:108-143) on a SimilarGenePairs
// object in device memory.  Integer / index work only, nothing is computed from a similarity: every output is
// bit-exact.
//
// The reference adds a vertex per gene of the graph's gene set S, walks every gene's stored list (add_edge into a boost::setS
// container: an edge that exists is not added again but still counts towards maxConnectivity), removes the vertices without an
// edge and, for getConnectivity, iterates every vertex's out-edge set.  Here:
//   * checkStoredPairsKernel    every stored pair of the SimilarGenePairs object names another gene of its gene set P, every
//                               usedCount is at most k -- nothing below reads a list before this has passed;
//   * runCellGraphEdges (em2_graph.hip)   the selection rule and the duplicate filter are the cell graph's: sel(v) = the first
//                               <= maxConnectivity stored pairs at or above the threshold whose partner is in S; the edges in
//                               insertion order are, for v0 ascending and v1 in sel(v0): (v0, v1) unless it is already in
//                               sel(v0) or (v1 < v0 and v0 in sel(v1)).  Both id maps (S -> P for the row, P -> global -> S for
//                               the partner) and their `consecutive` shortcut are that code's;
//   * edgeRecordsKernel         two directed records per edge: key = vertex << 32 | neighbour, value = the similarity's bits;
//   * rocPRIM's radix sort of the records by key.  An undirected edge exists once, so the keys are unique and the order is a
//     function of the input alone: per vertex, the neighbours ascending;
//   * connectivityOffsetsKernel the lower bound of v << 32 among the sorted keys for every v in [0, |S|]: the offsets of the
//                               lists; a gene is alive where its list is not empty.  No degree is counted with atomics;
//   * an exclusive scan of the alive flags, then geneGraphCompactKernel: the surviving genes in ascending order, and the
//     neighbour half of every sorted key.

#include "em2_device.h"
#include "em2_adjacency.h"
#include "em2_entry.h"
#include "em2_primitives.h"
#include "em2_scratch.h"

#include <algorithm>
#include <memory>
#include <vector>

// What the device code and the C entry points at the end of this file share.
namespace em2 {

// What the GeneGraph constructor (src/GeneGraph.cpp:22-104) leaves in the graph and what GeneGraph::getConnectivity
// (:108-143) reads from it, in host memory.  Every id is local to the graph's gene set S.
//   vertices                  the genes that keep a vertex (degree > 0), ascending;
//   edge0 / edge1 / edgeSimilarity   the edges in the order add_edge created them; the similarity is that of the first insertion;
//   connectivityOffsets       [|S| + 1]; the neighbours of gene v are connectivityGenes / connectivitySimilarities
//                             [offsets[v], offsets[v + 1]), none for a removed gene.  ORDER WITHIN A LIST: ascending neighbour id.
//                             The reference iterates a std::set of listS vertex descriptors -- heap pointers: its order is
//                             whatever malloc gave, i.e. undefined; this is the project's definition.
struct GeneGraphResult {
    uint32_t geneCount = 0;                        // |S|
    std::vector<uint32_t> vertices;
    std::vector<uint32_t> edge0, edge1;
    std::vector<float> edgeSimilarity;
    std::vector<uint64_t> connectivityOffsets;
    std::vector<uint32_t> connectivityGenes;
    std::vector<float> connectivitySimilarities;
};

// Bits of *inputError (nothing was computed where it is not 0).
constexpr uint32_t kGeneGraphSelfPair = 1u;        // a stored pair names its own gene
constexpr uint32_t kGeneGraphPartnerRange = 2u;    // a stored pair names a local id >= pairsGeneCount
constexpr uint32_t kGeneGraphUsedCount = 4u;       // a usedCount above k

// d_pairs [pairsGeneCount][k] and d_usedCount [pairsGeneCount] in device memory: the SimilarGenePairs object over the gene set
// P.  d_pairsGeneSet / d_graphGeneSet: the ascending global ids of P and of S in device memory, or NULL for a set of
// consecutive ids (then *Consecutive is true and *First is its first id).  graphGeneCount > 0.  maxConnectivity is the
// effective one: 0 (nothing is selected: k == 0) .. k.  Every stored pair of P is checked, also those of genes outside S.
// Takes its scratch from the cache of em2_scratch.h; synchronises the stream.
static hipError_t runGeneGraph(const PairOut* d_pairs, const uint32_t* d_usedCount, uint32_t pairsGeneCount, uint32_t k,
                               const uint32_t* d_pairsGeneSet, bool pairsConsecutive, uint32_t pairsFirst, const uint32_t* d_graphGeneSet,
                               bool graphConsecutive, uint32_t graphFirst, uint32_t graphGeneCount, double similarityThreshold,
                               uint32_t maxConnectivity, GeneGraphResult& out, uint32_t* inputError, hipStream_t stream);

namespace {

// Slot i = g * k + j of the pairs, for j < usedCount[g]: the partner is a local id of P other than g (findSimilarGenePairs0
// writes nothing else; the walk would index P's id table with it).  Gene g: usedCount[g] <= k.
__global__ void __launch_bounds__(256)
checkStoredPairsKernel(const PairOut* __restrict__ pairs, const uint32_t* __restrict__ usedCount, uint32_t geneCount, uint32_t k,
                       uint32_t* __restrict__ error)
{
    uint32_t bad = 0u;
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    const uint64_t first = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    for (uint64_t g = first; g < geneCount; g += stride) {
        if (usedCount[g] > k) bad |= kGeneGraphUsedCount;
    }
    const uint64_t slots = uint64_t(geneCount) * k;
    for (uint64_t i = first; i < slots; i += stride) {
        const uint32_t g = uint32_t(i / k);
        const uint32_t j = uint32_t(i - uint64_t(g) * k);
        if (j >= usedCount[g]) continue;
        const uint32_t partner = pairs[i].cell;
        if (partner >= geneCount) bad |= kGeneGraphPartnerRange;
        else if (partner == g) bad |= kGeneGraphSelfPair;
    }
    if (bad) atomicOr(error, bad);
}

__global__ void __launch_bounds__(256)
edgeRecordsKernel(const uint32_t* __restrict__ edge0, const uint32_t* __restrict__ edge1, const float* __restrict__ edgeSimilarity,
                  uint64_t edgeCount, uint64_t* __restrict__ keys, uint32_t* __restrict__ values)
{
    for (uint64_t e = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; e < edgeCount; e += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t v0 = edge0[e], v1 = edge1[e];
        const uint32_t bits = __float_as_uint(edgeSimilarity[e]);
        keys[2u * e] = v0 << 32 | v1;
        keys[2u * e + 1u] = v1 << 32 | v0;
        values[2u * e] = bits;
        values[2u * e + 1u] = bits;
    }
}

// offsets[v] = where the records of vertex v begin, v in [0, geneCount]; alive[v] = 1 where v has one, alive[geneCount] = 0
// (the scan's last input: its output there is the number of vertices that stay).
__global__ void __launch_bounds__(256)
connectivityOffsetsKernel(const uint64_t* __restrict__ keys, uint64_t recordCount, uint32_t geneCount, uint64_t* __restrict__ offsets,
                          uint32_t* __restrict__ alive)
{
    for (uint64_t v = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; v <= geneCount; v += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t begin = lowerBound(keys, recordCount, v << 32);
        offsets[v] = begin;
        alive[v] = v < geneCount && begin < recordCount && (keys[begin] >> 32) == v ? 1u : 0u;
    }
}

// vertices[rank[v]] = v for the genes that are alive (rank: the exclusive scan of alive); neighbours[i] = the low half of the
// i-th sorted key.
__global__ void __launch_bounds__(256)
geneGraphCompactKernel(const uint32_t* __restrict__ alive, const uint64_t* __restrict__ rank, uint32_t geneCount,
                       const uint64_t* __restrict__ keys, uint64_t recordCount, uint32_t* __restrict__ vertices,
                       uint32_t* __restrict__ neighbours)
{
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    const uint64_t first = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    for (uint64_t v = first; v < geneCount; v += stride) {
        if (alive[v]) vertices[rank[v]] = uint32_t(v);
    }
    for (uint64_t i = first; i < recordCount; i += stride) neighbours[i] = uint32_t(keys[i]);
}

template <class T> hipError_t toHost(std::vector<T>& to, const void* from, size_t count, hipStream_t stream)
{
    to.resize(count);
    if (count == 0) return hipSuccess;
    return hipMemcpyAsync(to.data(), from, count * sizeof(T), hipMemcpyDeviceToHost, stream);
}

}  // namespace

hipError_t runGeneGraph(const PairOut* d_pairs, const uint32_t* d_usedCount, uint32_t pairsGeneCount, uint32_t k,
                        const uint32_t* d_pairsGeneSet, bool pairsConsecutive, uint32_t pairsFirst, const uint32_t* d_graphGeneSet,
                        bool graphConsecutive, uint32_t graphFirst, uint32_t graphGeneCount, double similarityThreshold,
                        uint32_t maxConnectivity, GeneGraphResult& out, uint32_t* inputError, hipStream_t stream)
{
    *inputError = 0;
    out = GeneGraphResult();
    out.geneCount = graphGeneCount;
    StageTimer timer("geneGraph");
    const dim3 threads(256);
    ArenaPlan plan;

    // the stored pairs, then the edges in insertion order
    const size_t slots = size_t(graphGeneCount) * maxConnectivity;
    const size_t n1 = size_t(graphGeneCount) + 1u;
    const size_t offError = plan.take(256);
    const size_t offEdge0 = plan.takeFor<uint32_t>(slots);
    const size_t offEdge1 = plan.takeFor<uint32_t>(slots);
    const size_t offEdgeSimilarity = plan.takeFor<float>(slots);
    const size_t offOffsets = plan.takeFor<uint64_t>(n1);
    const size_t offAlive = plan.takeFor<uint32_t>(n1);
    const size_t offRank = plan.takeFor<uint64_t>(n1);
    const size_t offVertices = plan.takeFor<uint32_t>(graphGeneCount);
    size_t scanBytes = 0;
    EM2_TRY(exclusiveScanU32ToU64Bytes(n1, scanBytes));
    const size_t offScanTemp = plan.take(scanBytes);
    CachedBuffer arena, recordArena;
    EM2_TRY(arena.allocate(plan.bytes));
    char* base = arena.as<char>();
    uint32_t* error = arenaAt<uint32_t>(base, offError);
    uint32_t* edge0 = arenaAt<uint32_t>(base, offEdge0);
    uint32_t* edge1 = arenaAt<uint32_t>(base, offEdge1);
    float* edgeSimilarity = arenaAt<float>(base, offEdgeSimilarity);
    uint64_t* offsets = arenaAt<uint64_t>(base, offOffsets);
    uint32_t* alive = arenaAt<uint32_t>(base, offAlive);
    uint64_t* rank = arenaAt<uint64_t>(base, offRank);
    uint32_t* vertices = arenaAt<uint32_t>(base, offVertices);

    EM2_TRY(hipMemsetAsync(error, 0, 256, stream));
    checkStoredPairsKernel<<<dim3(gridFor(uint64_t(pairsGeneCount) * (k ? k : 1u))), threads, 0, stream>>>(d_pairs, d_usedCount, pairsGeneCount,
                                                                                                         k, error);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipMemcpyAsync(inputError, error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    if (*inputError) {
        arena.idle = true;
        return hipSuccess;
    }
    EM2_TRY(timer.stage("check", stream));

    // S is ascending: a gene's vertex is its position, the sorted ids are the set itself
    uint64_t edgeCount = 0;
    EM2_TRY(runCellGraphEdges(d_pairs, d_usedCount, pairsGeneCount, k, d_pairsGeneSet, d_graphGeneSet, d_graphGeneSet, nullptr,
                              graphGeneCount, similarityThreshold, maxConnectivity, edge0, edge1, edgeSimilarity, &edgeCount, stream,
                              pairsConsecutive, pairsFirst, graphConsecutive, graphFirst));
    EM2_TRY(timer.stage("selection and edges", stream));
    if (edgeCount > slots) {
        arena.idle = true;
        return hipErrorUnknown;
    }

    // the adjacency: 2 E directed records in (vertex, neighbour) order
    const uint64_t recordCount = 2u * edgeCount;
    const uint64_t* sortedKeys = nullptr;
    const uint32_t* sortedValues = nullptr;
    uint32_t* neighbours = nullptr;
    if (recordCount) {
        ArenaPlan records;
        const size_t offKeysA = records.takeFor<uint64_t>(recordCount);
        const size_t offKeysB = records.takeFor<uint64_t>(recordCount);
        const size_t offValuesA = records.takeFor<uint32_t>(recordCount);
        const size_t offValuesB = records.takeFor<uint32_t>(recordCount);
        const size_t offNeighbours = records.takeFor<uint32_t>(recordCount);
        size_t sortBytes = 0;
        EM2_TRY(sortPairsU64U32BufferBytes(size_t(recordCount), 0u, 64u, sortBytes));
        const size_t offSortTemp = records.take(sortBytes);
        EM2_TRY(recordArena.allocate(records.bytes));
        char* recordBase = recordArena.as<char>();
        DoubleBuffer<uint64_t> keys{arenaAt<uint64_t>(recordBase, offKeysA), arenaAt<uint64_t>(recordBase, offKeysB)};
        DoubleBuffer<uint32_t> values{arenaAt<uint32_t>(recordBase, offValuesA), arenaAt<uint32_t>(recordBase, offValuesB)};
        neighbours = arenaAt<uint32_t>(recordBase, offNeighbours);
        edgeRecordsKernel<<<dim3(gridFor(edgeCount)), threads, 0, stream>>>(edge0, edge1, edgeSimilarity, edgeCount, keys.current(),
                                                                           values.current());
        EM2_TRY(hipGetLastError());
        EM2_TRY(sortPairs(recordBase + offSortTemp, sortBytes, keys, values, size_t(recordCount), 0u, 64u, stream));
        sortedKeys = keys.current();
        sortedValues = values.current();
        EM2_TRY(timer.stage("records and sort", stream));
    }

    // (with no record the searches find nothing and read nothing: every offset 0, nobody alive)
    connectivityOffsetsKernel<<<dim3(gridFor(n1)), threads, 0, stream>>>(sortedKeys, recordCount, graphGeneCount, offsets, alive);
    EM2_TRY(hipGetLastError());
    EM2_TRY(exclusiveScan(base + offScanTemp, scanBytes, alive, rank, n1, stream));
    geneGraphCompactKernel<<<dim3(gridFor(recordCount > graphGeneCount ? recordCount : graphGeneCount)), threads, 0, stream>>>(
        alive, rank, graphGeneCount, sortedKeys, recordCount, vertices, neighbours);
    EM2_TRY(hipGetLastError());
    uint64_t vertexCount = 0;
    EM2_TRY(hipMemcpyAsync(&vertexCount, rank + graphGeneCount, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(timer.stage("offsets and vertices", stream));
    if (vertexCount > graphGeneCount) {
        arena.idle = recordArena.idle = true;
        return hipErrorUnknown;
    }

    EM2_TRY(toHost(out.vertices, vertices, size_t(vertexCount), stream));
    EM2_TRY(toHost(out.edge0, edge0, size_t(edgeCount), stream));
    EM2_TRY(toHost(out.edge1, edge1, size_t(edgeCount), stream));
    EM2_TRY(toHost(out.edgeSimilarity, edgeSimilarity, size_t(edgeCount), stream));
    EM2_TRY(toHost(out.connectivityOffsets, offsets, n1, stream));
    EM2_TRY(toHost(out.connectivityGenes, neighbours, size_t(recordCount), stream));
    EM2_TRY(toHost(out.connectivitySimilarities, sortedValues, size_t(recordCount), stream));
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(timer.stage("results to the host", stream));
    arena.idle = recordArena.idle = true;                       // (everything that used the blocks has been waited for)
    return hipSuccess;
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

struct em2_gene_graph {
    em2::GeneGraphResult result;
};

// Strictly ascending: what a stored GeneSet is once sorted (src/GeneSet.cpp), and what both id look-ups rely on.
static bool strictlyAscending(const uint32_t* ids, uint32_t count)
{
    for (uint32_t i = 1; i < count; i++) {
        if (ids[i - 1] >= ids[i]) return false;
    }
    return true;
}

static int geneGraphCreate(const char* who, bool pairsOnDevice, const em2_pair* pairs, const uint32_t* usedCount, uint32_t pairsGeneCount,
                           uint32_t k, const uint32_t* pairsGeneSet, const uint32_t* graphGeneSet, uint32_t graphGeneCount,
                           double similarityThreshold, uint64_t maxConnectivity, em2_gene_graph** graph)
{
    if (!graph) return failNull(who);
    *graph = nullptr;
    if (graphGeneCount == 0) return failArgument(who, "graphGeneCount must be positive");
    if (!graphGeneSet || (pairsGeneCount && (!pairsGeneSet || !usedCount || (!pairs && k)))) return failNull(who);
    if (!strictlyAscending(pairsGeneSet, pairsGeneCount) || !strictlyAscending(graphGeneSet, graphGeneCount)) {
        return failArgument(who, "a gene set is not in strictly ascending order");
    }
    if (!haveDevice()) return failNoDevice(who);
    // src/GeneGraph.cpp:80-83 increments and then tests for equality, so 0 -- and a negative Python int, converted to size_t --
    // never matches: no limit.  A gene never selects more than its k stored pairs either way.
    const uint32_t effective = (maxConnectivity == 0 || maxConnectivity > k) ? k : uint32_t(maxConnectivity);
    // (sets of consecutive ids need no search on the device and are not sent there)
    const bool pairsConsecutive = pairsGeneCount && pairsGeneSet[pairsGeneCount - 1] - pairsGeneSet[0] == pairsGeneCount - 1;
    const bool graphConsecutive = graphGeneSet[graphGeneCount - 1] - graphGeneSet[0] == graphGeneCount - 1;
    DeviceBuffer dPairs, dUsed, dPairsSet, dGraphSet;
    if (!pairsOnDevice) {
        EM2_HIP(dPairs.upload(pairs, size_t(pairsGeneCount) * k));
        EM2_HIP(dUsed.upload(usedCount, pairsGeneCount));
    }
    if (!pairsConsecutive) EM2_HIP(dPairsSet.upload(pairsGeneSet, pairsGeneCount));
    if (!graphConsecutive) EM2_HIP(dGraphSet.upload(graphGeneSet, graphGeneCount));
    std::unique_ptr<em2_gene_graph> g(new em2_gene_graph);
    uint32_t inputError = 0;
    const hipError_t status = em2::runGeneGraph(
        pairsOnDevice ? reinterpret_cast<const em2::PairOut*>(pairs) : dPairs.as<em2::PairOut>(), pairsOnDevice ? usedCount : dUsed.as<uint32_t>(),
        pairsGeneCount, k, pairsConsecutive ? nullptr : dPairsSet.as<uint32_t>(), pairsConsecutive, pairsGeneCount ? pairsGeneSet[0] : 0u,
        graphConsecutive ? nullptr : dGraphSet.as<uint32_t>(), graphConsecutive, graphGeneSet[0], graphGeneCount, similarityThreshold,
        effective, g->result, &inputError, nullptr);
    if (status != hipSuccess || inputError) {
        EM2_HIP(status);
        if (inputError & em2::kGeneGraphUsedCount) return failArgument(who, "a usedCount is above k");
        if (inputError & em2::kGeneGraphPartnerRange) return failArgument(who, "a stored pair names a gene outside the pairs' gene set");
        return failArgument(who, "a stored pair names its own gene");
    }
    *graph = g.release();
    return EM2_OK;
}

int em2_gene_graph_create(const em2_pair* pairs, const uint32_t* usedCount, uint32_t pairsGeneCount, uint32_t k,
                          const uint32_t* pairsGeneSet, const uint32_t* graphGeneSet, uint32_t graphGeneCount,
                          double similarityThreshold, uint64_t maxConnectivity, em2_gene_graph** graph)
{
    return geneGraphCreate("em2_gene_graph_create", false, pairs, usedCount, pairsGeneCount, k, pairsGeneSet, graphGeneSet, graphGeneCount,
                           similarityThreshold, maxConnectivity, graph);
}

int em2_dev_gene_graph_create(const em2_pair* d_pairs, const uint32_t* d_usedCount, uint32_t pairsGeneCount, uint32_t k,
                              const uint32_t* pairsGeneSet, const uint32_t* graphGeneSet, uint32_t graphGeneCount,
                              double similarityThreshold, uint64_t maxConnectivity, em2_gene_graph** graph)
{
    return geneGraphCreate("em2_dev_gene_graph_create", true, d_pairs, d_usedCount, pairsGeneCount, k, pairsGeneSet, graphGeneSet,
                           graphGeneCount, similarityThreshold, maxConnectivity, graph);
}

int em2_gene_graph_sizes(const em2_gene_graph* graph, uint32_t* vertexCount, uint64_t* edgeCount, uint32_t* removedCount)
{
    if (!graph) return failNull("em2_gene_graph_sizes");
    const em2::GeneGraphResult& r = graph->result;
    if (vertexCount) *vertexCount = uint32_t(r.vertices.size());
    if (edgeCount) *edgeCount = r.edge0.size();
    if (removedCount) *removedCount = r.geneCount - uint32_t(r.vertices.size());
    return EM2_OK;
}

int em2_gene_graph_get(const em2_gene_graph* graph, uint32_t* vertices, uint32_t* edgeGene0, uint32_t* edgeGene1, float* edgeSimilarity,
                       uint64_t* connectivityOffsets, uint32_t* connectivityGenes, float* connectivitySimilarities)
{
    if (!graph) return failNull("em2_gene_graph_get");
    const em2::GeneGraphResult& r = graph->result;
    if (vertices) std::copy(r.vertices.begin(), r.vertices.end(), vertices);
    if (edgeGene0) std::copy(r.edge0.begin(), r.edge0.end(), edgeGene0);
    if (edgeGene1) std::copy(r.edge1.begin(), r.edge1.end(), edgeGene1);
    if (edgeSimilarity) std::copy(r.edgeSimilarity.begin(), r.edgeSimilarity.end(), edgeSimilarity);
    if (connectivityOffsets) std::copy(r.connectivityOffsets.begin(), r.connectivityOffsets.end(), connectivityOffsets);
    if (connectivityGenes) std::copy(r.connectivityGenes.begin(), r.connectivityGenes.end(), connectivityGenes);
    if (connectivitySimilarities) std::copy(r.connectivitySimilarities.begin(), r.connectivitySimilarities.end(), connectivitySimilarities);
    return EM2_OK;
}

void em2_gene_graph_free(em2_gene_graph* graph) { delete graph; }

}  // extern "C"
