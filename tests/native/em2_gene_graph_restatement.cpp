// em2_gene_graph_restatement.cpp -- the GeneGraph constructor (reference src/GeneGraph.cpp:22-104) and
// GeneGraph::getConnectivity (:108-143) restated with standard containers in place of boost::adjacency_list<setS, listS,
// undirectedS>: a std::map vertex table (global gene id -> vertex), a std::set of out-edges per vertex keyed on the
// neighbour, a std::list of edges in creation order, and the removal of the vertices without an edge.  One thread, no GPU:
// the yardstick of tests/test_gpu_gene_graph.py; tests/test_gene_graph_cpu.py holds it against the closed form in Python.
//
// Every id the graph returns is local to the graph's gene set S.  Within a connectivity list the neighbours ascend by local
// id: the reference iterates a std::set of listS vertex descriptors (heap pointers), whose order is undefined; the project
// defines it (include/em2_lsh.h).
//
// Precondition, as for the library: every stored pair names a local id < pairsGeneCount other than its own gene.
#include <stdint.h>

#include <chrono>
#include <cstddef>
#include <list>
#include <map>
#include <set>
#include <vector>

namespace {

struct Pair {
    uint32_t gene;
    float similarity;
};

struct Edge {
    uint32_t v0, v1;
    float similarity;
};

struct OutEdge {
    uint32_t target;
    std::list<Edge>::const_iterator edge;
    bool operator<(const OutEdge& that) const { return target < that.target; }      // setS: one edge per neighbour
};

struct Vertex {
    uint32_t globalGeneId;
    std::set<OutEdge> outEdges;
};

struct Graph {
    std::vector<uint32_t> geneSet;                 // S
    std::vector<Vertex> vertices;                  // one per gene of S; the removed ones are no longer in the table
    std::map<uint32_t, uint32_t> vertexTable;      // global gene id -> vertex
    std::list<Edge> edges;
    uint64_t removed = 0;

    // boost::add_edge on setS: nothing happens where the edge exists
    void addEdge(uint32_t v0, uint32_t v1, float similarity)
    {
        OutEdge probe{v1, edges.end()};
        if (vertices[v0].outEdges.count(probe)) return;
        edges.push_back(Edge{v0, v1, similarity});
        const std::list<Edge>::const_iterator it = --edges.end();
        vertices[v0].outEdges.insert(OutEdge{v1, it});
        vertices[v1].outEdges.insert(OutEdge{v0, it});
    }
};

// GeneSet::getLocalGeneId on a sorted set (src/GeneSet.cpp): the position, or the invalid id
const uint32_t invalidGeneId = 0xffffffffu;
uint32_t localGeneId(const uint32_t* set, uint32_t count, uint32_t globalGeneId)
{
    uint32_t low = 0, high = count;
    while (low < high) {
        const uint32_t middle = low + (high - low) / 2;
        if (set[middle] < globalGeneId) low = middle + 1;
        else high = middle;
    }
    return low < count && set[low] == globalGeneId ? low : invalidGeneId;
}

}  // namespace

extern "C" {

void* em2r_gene_graph_create(const Pair* pairs, const uint32_t* usedCount, uint32_t pairsGeneCount, uint32_t k,
                             const uint32_t* pairsGeneSet, const uint32_t* graphGeneSet, uint32_t graphGeneCount,
                             double similarityThreshold, uint64_t maxConnectivity, double* seconds)
{
    const auto begin = std::chrono::steady_clock::now();
    Graph* graph = new Graph;
    graph->geneSet.assign(graphGeneSet, graphGeneSet + graphGeneCount);

    // :40-43
    for (const uint32_t globalGeneId : graph->geneSet) {
        graph->vertexTable.insert(std::make_pair(globalGeneId, uint32_t(graph->vertices.size())));
        graph->vertices.push_back(Vertex{globalGeneId, {}});
    }

    // :53-86
    for (const uint32_t globalGeneId0 : graph->geneSet) {
        const uint32_t v0 = graph->vertexTable[globalGeneId0];
        const uint32_t localGeneId0 = localGeneId(pairsGeneSet, pairsGeneCount, globalGeneId0);
        if (localGeneId0 == invalidGeneId) continue;
        uint64_t connectivity = 0;
        const Pair* list = pairs + size_t(localGeneId0) * k;
        for (uint32_t j = 0; j < usedCount[localGeneId0]; j++) {
            const float similarity = list[j].similarity;
            if (similarity < similarityThreshold) break;
            const uint32_t globalGeneId1 = pairsGeneSet[list[j].gene];
            const auto it1 = graph->vertexTable.find(globalGeneId1);
            if (it1 != graph->vertexTable.end()) {
                graph->addEdge(v0, it1->second, similarity);
                ++connectivity;
                if (connectivity == maxConnectivity) break;
            }
        }
    }

    // :88-99
    for (const Vertex& vertex : graph->vertices) {
        if (vertex.outEdges.empty()) {
            graph->vertexTable.erase(vertex.globalGeneId);
            ++graph->removed;
        }
    }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();
    return graph;
}

void em2r_gene_graph_sizes(const void* handle, uint64_t* vertexCount, uint64_t* edgeCount, uint64_t* removedCount)
{
    const Graph* graph = static_cast<const Graph*>(handle);
    *vertexCount = graph->vertexTable.size();
    *edgeCount = graph->edges.size();
    *removedCount = graph->removed;
}

// vertices [vertexCount]: local ids in S, ascending; the edges in creation order; the connectivity of getConnectivity
// (:108-143) as offsets [|S| + 1] into (neighbour, similarity) lists.
void em2r_gene_graph_get(const void* handle, uint32_t* vertices, uint32_t* edgeGene0, uint32_t* edgeGene1, float* edgeSimilarity,
                         uint64_t* connectivityOffsets, uint32_t* connectivityGenes, float* connectivitySimilarities)
{
    const Graph* graph = static_cast<const Graph*>(handle);
    const uint32_t geneCount = uint32_t(graph->geneSet.size());
    for (const auto& entry : graph->vertexTable) *vertices++ = entry.second;       // (S ascends, so does the vertex)
    for (const Edge& edge : graph->edges) {
        *edgeGene0++ = edge.v0;
        *edgeGene1++ = edge.v1;
        *edgeSimilarity++ = edge.similarity;
    }
    uint64_t at = 0;
    for (uint32_t localGeneId0 = 0; localGeneId0 != geneCount; localGeneId0++) {
        connectivityOffsets[localGeneId0] = at;
        const uint32_t globalGeneId0 = graph->geneSet[localGeneId0];
        const auto it0 = graph->vertexTable.find(globalGeneId0);
        if (it0 == graph->vertexTable.end()) continue;
        for (const OutEdge& out : graph->vertices[it0->second].outEdges) {
            const uint32_t globalGeneId1 = graph->vertices[out.target].globalGeneId;
            connectivityGenes[at] = localGeneId(graph->geneSet.data(), geneCount, globalGeneId1);
            connectivitySimilarities[at] = out.edge->similarity;
            ++at;
        }
    }
    connectivityOffsets[geneCount] = at;
}

void em2r_gene_graph_free(void* handle) { delete static_cast<Graph*>(handle); }

}  // extern "C"
