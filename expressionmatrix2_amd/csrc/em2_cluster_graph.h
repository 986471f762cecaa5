// em2_cluster_graph.h -- internal interface of em2_cluster_graph.hip for the C ABI glue (em2_capi.hip).
#ifndef EM2_CLUSTER_GRAPH_H
#define EM2_CLUSTER_GRAPH_H

#include "em2_device.h"

#include <string>
#include <vector>

namespace em2 {

struct ClusterStatus {
    int code;                   // EM2_OK or an EM2_ERROR_* of include/em2_lsh.h
    std::string message;
};

// The device side of ClusterGraph::computeAverageGeneExpression / computeSimilarities (src/ClusterGraph.cpp:125-169):
// holds the expression counts and the table of averages [cluster][gene] in device memory between the calls.
class ClusterDevice {
public:
    ClusterDevice();
    ~ClusterDevice();
    ClusterDevice(const ClusterDevice&) = delete;
    ClusterDevice& operator=(const ClusterDevice&) = delete;
    ClusterStatus upload(const char* who, const uint64_t* toc, const CountIn* data, uint32_t rowCount, uint32_t geneCount);
    ClusterStatus setAverages(const double* averages, uint32_t clusterCount, uint32_t geneCount);
    ClusterStatus averages(const char* who, const uint32_t* cellRows, const uint64_t* offsets, uint32_t clusterCount, double* hostAverages);
    ClusterStatus similarities(const char* who, const uint32_t* edge0, const uint32_t* edge1, uint64_t edgeCount, double* similarity);

private:
    struct State;
    State* state;
};

// What ExpressionMatrix::createClusterGraph (src/ExpressionMatrix.cpp:2153-2181) leaves in the ClusterGraph.  Clusters in
// vertex order; cells and unclusteredCells are cell-graph vertex indices; edges in the order of their creation.
struct ClusterGraphResult {
    uint32_t geneCount = 0;
    std::vector<uint32_t> clusterIds;
    std::vector<uint64_t> cellOffsets;
    std::vector<uint32_t> cells, unclusteredCells;
    std::vector<double> averages;
    std::vector<uint32_t> edgeCluster0, edgeCluster1;
    std::vector<double> edgeSimilarity;
    uint32_t initialClusterCount = 0;       // vertices and edges of the constructor, before the merge
    uint64_t initialEdgeCount = 0;
    double averagesSeconds = 0., similaritiesSeconds = 0., totalSeconds = 0.;
};

ClusterStatus createClusterGraph(const uint64_t* toc, const CountIn* data, uint32_t rowCount, uint32_t geneCount,
                                 const uint32_t* vertexRows, uint32_t vertexCount, const uint32_t* edgeVertex0,
                                 const uint32_t* edgeVertex1, uint64_t edgeCount, const uint32_t* labels, uint64_t minClusterSize,
                                 uint64_t k, double similarityThreshold, double similarityThresholdForMerge, ClusterGraphResult& out);

}  // namespace em2

#endif
