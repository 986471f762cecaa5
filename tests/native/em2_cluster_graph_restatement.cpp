// em2_cluster_graph_restatement.cpp -- test infrastructure: a single-thread C++ restatement of what
// ExpressionMatrix::createClusterGraph does after the label propagation (src/ExpressionMatrix.cpp:2153-2181):
// ClusterGraph (src/ClusterGraph.cpp:59-386), ExpressionMatrix::computeAverageExpression and computeExpressionVector with L2
// normalization (src/ExpressionMatrix.cpp:1179-1296) and regressionCoefficient (src/regressionCoefficient.cpp:10-42).
// Plain loops, std::map, std::sort; compiled with g++ -O2 -msse4.2 -ffp-contract=off by tests/cluster_graph_binding.py.
// The device code (csrc/em2_cluster_graph.hip) must reproduce every bit of it.
//
// Two places the reference does not pin: makeKnn orders edges of equal similarity by their Boost
// descriptors -- here the edge created later ranks higher, and knnTie reports whether that rule decided anything; a NaN
// similarity at makeKnn makes the sort undefined -- em2r_cluster_graph_create returns 1.

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace {

struct Count {
    uint32_t gene;
    float count;
};

// computeExpressionVector (:1253-1296), L2: the counts of one cell, normalized
void expressionVector(const uint64_t* toc, const Count* data, uint32_t cell, std::vector<std::pair<uint32_t, float>>& v)
{
    v.clear();
    for (uint64_t p = toc[cell]; p < toc[cell + 1]; ++p) v.push_back(std::make_pair(data[p].gene, data[p].count));
    double sum = 0.;
    for (const auto& p : v) sum += p.second * p.second;
    const float factor = float(1. / std::sqrt(sum));
    for (auto& p : v) p.second *= factor;
}

// computeAverageExpression (:1179-1245), L2
void averageExpression(const uint64_t* toc, const Count* data, uint32_t geneCount, const uint32_t* cells, uint64_t cellCount,
                       double* average)
{
    std::vector<std::pair<uint32_t, float>> v;
    for (uint32_t g = 0; g < geneCount; ++g) average[g] = 0.;
    for (uint64_t i = 0; i < cellCount; ++i) {
        expressionVector(toc, data, cells[i], v);
        for (const auto& p : v) average[p.first] += p.second;
    }
    const double factor = 1. / double(cellCount);
    for (uint32_t g = 0; g < geneCount; ++g) average[g] *= factor;
    double sum = 0.;
    for (uint32_t g = 0; g < geneCount; ++g) sum += average[g] * average[g];
    const double factor2 = 1. / std::sqrt(sum);
    for (uint32_t g = 0; g < geneCount; ++g) average[g] *= factor2;
}

// regressionCoefficient (src/regressionCoefficient.cpp:10-42)
double regressionCoefficient(const double* X, const double* Y, size_t n)
{
    double sx = 0., sy = 0., sxx = 0., syy = 0., sxy = 0.;
    for (size_t i = 0; i < n; ++i) {
        const double x = X[i], y = Y[i];
        sx += x;
        sy += y;
        sxx += x * x;
        syy += y * y;
        sxy += x * y;
    }
    const double nDouble = double(n);
    const double numerator = nDouble * sxy - sx * sy;
    const double denominator = std::sqrt((nDouble * sxx - sx * sx) * (nDouble * syy - sy * sy));
    return numerator / denominator;
}

struct Vertex {
    uint32_t clusterId;
    std::vector<uint32_t> cells;
    std::vector<double> average;
    bool removed;
};

struct Edge {
    size_t v0, v1;
    double similarity;
    bool removed;
};

struct Graph {
    uint32_t geneCount = 0;
    std::vector<Vertex> vertices;               // in add_vertex order; removed ones stay as tombstones
    std::vector<Edge> edges;                    // in add_edge order
    std::vector<uint32_t> unclusteredCells;
    int knnTie = 0;
};

void computeAll(Graph& g, const uint64_t* toc, const Count* data, const uint32_t* vertexRows)
{
    std::vector<uint32_t> rows;
    for (Vertex& v : g.vertices) {
        if (v.removed) continue;
        rows.clear();
        for (const uint32_t cell : v.cells) rows.push_back(vertexRows ? vertexRows[cell] : cell);
        v.average.resize(g.geneCount);
        averageExpression(toc, data, g.geneCount, rows.data(), rows.size(), v.average.data());
    }
    for (Edge& e : g.edges) {
        if (e.removed) continue;
        e.similarity = regressionCoefficient(g.vertices[e.v0].average.data(), g.vertices[e.v1].average.data(), g.geneCount);
    }
}

void removeVertex(Graph& g, size_t v)
{
    g.vertices[v].removed = true;
    for (Edge& e : g.edges) {
        if (e.v0 == v || e.v1 == v) e.removed = true;
    }
}

}  // namespace

extern "C" {

void em2r_cluster_average_expression(const uint64_t* toc, const Count* data, uint32_t geneCount, const uint32_t* clusterCells,
                                     const uint64_t* clusterOffsets, uint32_t clusterCount, double* averages)
{
    for (uint32_t c = 0; c < clusterCount; ++c) {
        averageExpression(toc, data, geneCount, clusterCells + clusterOffsets[c], clusterOffsets[c + 1] - clusterOffsets[c],
                          averages + size_t(c) * geneCount);
    }
}

void em2r_cluster_similarities(const double* averages, uint32_t geneCount, const uint32_t* edge0, const uint32_t* edge1,
                               uint64_t edgeCount, double* similarity)
{
    for (uint64_t e = 0; e < edgeCount; ++e) {
        similarity[e] = regressionCoefficient(averages + size_t(edge0[e]) * geneCount, averages + size_t(edge1[e]) * geneCount, geneCount);
    }
}

// 0: done; 1: a NaN similarity when makeKnn starts (*graph is not set).  stopAfter (tests): 0 all steps, 1 stop after the
// constructor's averages and similarities, 2 after the merge, 3 after removeSmallVertices and the second similarities
int em2r_cluster_graph_create(const uint64_t* toc, const Count* data, uint32_t geneCount, const uint32_t* vertexRows,
                              uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                              const uint32_t* labels, uint64_t minClusterSize, uint64_t k, double similarityThreshold,
                              double similarityThresholdForMerge, int stopAfter, void** graph)
{
    Graph* gp = new Graph;
    Graph& g = *gp;
    g.geneCount = geneCount;

    // ClusterGraph::ClusterGraph (:61-120)
    std::map<uint32_t, size_t> vertexMap;
    std::vector<size_t> vertexOfCell(vertexCount);
    for (uint32_t cv = 0; cv < vertexCount; ++cv) {
        const auto it = vertexMap.find(labels[cv]);
        if (it == vertexMap.end()) {
            vertexMap.insert(std::make_pair(labels[cv], g.vertices.size()));
            vertexOfCell[cv] = g.vertices.size();
            Vertex v;
            v.clusterId = labels[cv];
            v.removed = false;
            v.cells.push_back(cv);
            g.vertices.push_back(v);
        } else {
            g.vertices[it->second].cells.push_back(cv);
            vertexOfCell[cv] = it->second;
        }
    }
    std::set<std::pair<size_t, size_t>> edgeSet;            // setS: no parallel edges, undirected
    for (uint64_t ce = 0; ce < edgeCount; ++ce) {
        const size_t v0 = vertexOfCell[edgeVertex0[ce]], v1 = vertexOfCell[edgeVertex1[ce]];
        if (v0 == v1) continue;
        if (!edgeSet.insert(std::make_pair(std::min(v0, v1), std::max(v0, v1))).second) continue;
        Edge e;
        e.v0 = v0;
        e.v1 = v1;
        e.similarity = 0.;
        e.removed = false;
        g.edges.push_back(e);
    }

    // mergeVertices (:174-270)
    computeAll(g, toc, data, vertexRows);
    if (stopAfter == 1) {
        *graph = gp;
        return 0;
    }
    {
        // connected components over the high similarity edges, by a search from every vertex in vertex order
        const size_t n = g.vertices.size();
        std::vector<std::vector<size_t>> neighbours(n);
        for (const Edge& e : g.edges) {
            if (e.similarity > similarityThresholdForMerge) {
                neighbours[e.v0].push_back(e.v1);
                neighbours[e.v1].push_back(e.v0);
            }
        }
        std::vector<int> component(n, -1);
        int componentCount = 0;
        for (size_t start = 0; start < n; ++start) {
            if (component[start] >= 0) continue;
            std::vector<size_t> stack(1, start);
            component[start] = componentCount;
            while (!stack.empty()) {
                const size_t v = stack.back();
                stack.pop_back();
                for (const size_t w : neighbours[v]) {
                    if (component[w] < 0) {
                        component[w] = componentCount;
                        stack.push_back(w);
                    }
                }
            }
            ++componentCount;
        }
        std::vector<std::vector<size_t>> componentVertices(componentCount);
        for (size_t v = 0; v < n; ++v) componentVertices[component[v]].push_back(v);
        for (const std::vector<size_t>& verticesToMerge : componentVertices) {
            if (verticesToMerge.size() < 2) continue;
            Vertex& vertex0 = g.vertices[verticesToMerge.front()];
            for (size_t i = 1; i < verticesToMerge.size(); ++i) {
                Vertex& vertex1 = g.vertices[verticesToMerge[i]];
                std::copy(vertex1.cells.begin(), vertex1.cells.end(), std::back_inserter(vertex0.cells));
                vertexMap.erase(vertex1.clusterId);
                removeVertex(g, verticesToMerge[i]);
            }
        }
    }
    if (stopAfter == 2) {
        *graph = gp;
        return 0;
    }

    // removeSmallVertices (:304-319)
    {
        std::vector<size_t> verticesToBeRemoved;
        for (size_t v = 0; v < g.vertices.size(); ++v) {
            if (g.vertices[v].removed) continue;
            if (g.vertices[v].cells.size() < minClusterSize) {
                verticesToBeRemoved.push_back(v);
                std::copy(g.vertices[v].cells.begin(), g.vertices[v].cells.end(), std::back_inserter(g.unclusteredCells));
            }
        }
        for (const size_t v : verticesToBeRemoved) {
            vertexMap.erase(g.vertices[v].clusterId);
            removeVertex(g, v);
        }
    }

    computeAll(g, toc, data, vertexRows);
    if (stopAfter == 3) {
        *graph = gp;
        return 0;
    }

    // removeWeakEdges (:324-336)
    for (Edge& e : g.edges) {
        if (!e.removed && e.similarity < similarityThreshold) e.removed = true;
    }
    for (const Edge& e : g.edges) {
        if (!e.removed && std::isnan(e.similarity)) {
            delete gp;
            return 1;
        }
    }

    // makeKnn (:342-386)
    {
        std::vector<size_t> edgesToBeKept;
        std::vector<std::pair<double, size_t>> vertexEdges;
        for (size_t v = 0; v < g.vertices.size(); ++v) {
            if (g.vertices[v].removed) continue;
            vertexEdges.clear();
            for (size_t e = 0; e < g.edges.size(); ++e) {
                if (!g.edges[e].removed && (g.edges[e].v0 == v || g.edges[e].v1 == v)) {
                    vertexEdges.push_back(std::make_pair(g.edges[e].similarity, e));
                }
            }
            // equal similarities: the later edge first -- which is what std::greater on (similarity, creation index) says
            std::sort(vertexEdges.begin(), vertexEdges.end(), std::greater<std::pair<double, size_t>>());
            if (vertexEdges.size() > k) {
                if (k > 0 && vertexEdges[k - 1].first == vertexEdges[k].first) g.knnTie = 1;
                vertexEdges.resize(k);
            }
            for (const auto& p : vertexEdges) edgesToBeKept.push_back(p.second);
        }
        std::sort(edgesToBeKept.begin(), edgesToBeKept.end());
        for (size_t e = 0; e < g.edges.size(); ++e) {
            if (!g.edges[e].removed && !std::binary_search(edgesToBeKept.begin(), edgesToBeKept.end(), e)) g.edges[e].removed = true;
        }
    }

    // renumberClusters (:276-299)
    {
        std::vector<std::pair<const Vertex*, uint32_t>> vertexTable;
        for (const Vertex& v : g.vertices) {
            if (!v.removed) vertexTable.push_back(std::make_pair(&v, uint32_t(v.cells.size())));
        }
        std::sort(vertexTable.begin(), vertexTable.end(),
                  [](const std::pair<const Vertex*, uint32_t>& x, const std::pair<const Vertex*, uint32_t>& y) { return x.second > y.second; });
        for (uint32_t clusterId = 0; clusterId < uint32_t(vertexTable.size()); ++clusterId) {
            const_cast<Vertex*>(vertexTable[clusterId].first)->clusterId = clusterId;
        }
    }
    *graph = gp;
    return 0;
}

void em2r_cluster_graph_sizes(const void* graph, uint32_t* clusterCount, uint64_t* clusteredCellCount, uint64_t* unclusteredCellCount,
                              uint64_t* edgeCount, int* knnTie)
{
    const Graph& g = *static_cast<const Graph*>(graph);
    *clusterCount = 0;
    *clusteredCellCount = 0;
    *edgeCount = 0;
    for (const Vertex& v : g.vertices) {
        if (v.removed) continue;
        ++*clusterCount;
        *clusteredCellCount += v.cells.size();
    }
    for (const Edge& e : g.edges) {
        if (!e.removed) ++*edgeCount;
    }
    *unclusteredCellCount = g.unclusteredCells.size();
    *knnTie = g.knnTie;
}

// edge0 / edge1: the clusterIds of the edge's vertices as they stand (final ids after all steps)
void em2r_cluster_graph_get(const void* graph, uint32_t* clusterIds, uint64_t* cellOffsets, uint32_t* cells, uint32_t* unclusteredCells,
                            double* averages, uint32_t* edge0, uint32_t* edge1, double* edgeSimilarity)
{
    const Graph& g = *static_cast<const Graph*>(graph);
    size_t c = 0, at = 0;
    cellOffsets[0] = 0;
    for (const Vertex& v : g.vertices) {
        if (v.removed) continue;
        clusterIds[c] = v.clusterId;
        for (const uint32_t cell : v.cells) cells[at++] = cell;
        cellOffsets[c + 1] = at;
        for (uint32_t gene = 0; gene < g.geneCount; ++gene) averages[c * g.geneCount + gene] = v.average[gene];
        ++c;
    }
    for (size_t i = 0; i < g.unclusteredCells.size(); ++i) unclusteredCells[i] = g.unclusteredCells[i];
    size_t e = 0;
    for (const Edge& edge : g.edges) {
        if (edge.removed) continue;
        edge0[e] = g.vertices[edge.v0].clusterId;
        edge1[e] = g.vertices[edge.v1].clusterId;
        edgeSimilarity[e] = edge.similarity;
        ++e;
    }
}

void em2r_cluster_graph_free(void* graph) { delete static_cast<Graph*>(graph); }

// std::sort and std::stable_sort of (position, size) by size descending -> the positions in sorted order (tests: the
// renumbering is std::sort's arrangement, which is not the stable one)
void em2r_sort_by_size(const uint32_t* sizes, uint32_t count, int stable, uint32_t* order)
{
    std::vector<std::pair<uint64_t, uint32_t>> table;
    for (uint32_t i = 0; i < count; ++i) table.push_back(std::make_pair(uint64_t(i), sizes[i]));
    const auto greaterSize = [](const std::pair<uint64_t, uint32_t>& x, const std::pair<uint64_t, uint32_t>& y) { return x.second > y.second; };
    if (stable) std::stable_sort(table.begin(), table.end(), greaterSize);
    else std::sort(table.begin(), table.end(), greaterSize);
    for (uint32_t i = 0; i < count; ++i) order[i] = uint32_t(table[i].first);
}

}  // extern "C"
