// em2_gene_graph.h -- internal interface of em2_gene_graph.hip for the C ABI glue (em2_capi.hip).
#ifndef EM2_GENE_GRAPH_H
#define EM2_GENE_GRAPH_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

#include "em2_device.h"

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
hipError_t runGeneGraph(const PairOut* d_pairs, const uint32_t* d_usedCount, uint32_t pairsGeneCount, uint32_t k,
                        const uint32_t* d_pairsGeneSet, bool pairsConsecutive, uint32_t pairsFirst, const uint32_t* d_graphGeneSet,
                        bool graphConsecutive, uint32_t graphFirst, uint32_t graphGeneCount, double similarityThreshold,
                        uint32_t maxConnectivity, GeneGraphResult& out, uint32_t* inputError, hipStream_t stream);

}  // namespace em2

#endif
