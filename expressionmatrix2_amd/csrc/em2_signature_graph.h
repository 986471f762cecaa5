// em2_signature_graph.h -- internal interface of em2_signature_graph.hip for the C ABI glue (em2_capi.hip).
#ifndef EM2_SIGNATURE_GRAPH_H
#define EM2_SIGNATURE_GRAPH_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include <vector>

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
hipError_t runSignatureGraph(const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount, uint64_t minCellCount, bool withEdges,
                             SignatureGraphResult& out, uint32_t* inputError, hipStream_t stream);

// Lsh::writeSignatureStatistics (src/Lsh.cpp:279-303) without its text: d_setCount[i] = the cells with bit i set, i < lshCount.
// d_setCount is zeroed here.  Asynchronous on the stream.
hipError_t launchSignatureStatistics(const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount,
                                     unsigned long long* d_setCount, hipStream_t stream);

}  // namespace em2

#endif
