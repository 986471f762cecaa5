// em2_layout.h -- internal interface of em2_layout.hip for the C ABI glue (em2_capi.hip): the single-level spring-electrical
// layout of a graph.
#ifndef EM2_LAYOUT_H
#define EM2_LAYOUT_H

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace em2 {

// The constants of the model (Hu 2005) and of the summation shapes.  The shapes are part of the contract: they are functions
// of the vertex count alone, never of the device or the grid.
constexpr float kLayoutC = 0.2f;                    // C * K^2, with the natural length K = 1
constexpr float kLayoutFloor = 1e-30f;              // delta: d^2 is raised to it, so j = i and coincident vertices add an exact 0
constexpr double kLayoutT = 0.9;                    // the step is multiplied by t when the energy did not fall
constexpr uint32_t kLayoutProgress = 5;             // ... and divided by t after this many falls in a row
constexpr uint32_t kLayoutSliceCount = 16;          // slices of the j range of a repulsion sum: ceil(N / 16) consecutive vertices each
constexpr uint32_t kLayoutTile = 128;               // j positions staged in LDS at a time (no effect on any sum)
constexpr uint32_t kLayoutBlockVertices = 256;      // vertices of a workgroup, and the leaves of one chunk of the energy tree
constexpr uint32_t kLayoutMaxVertexCount = 1u << 30;

struct LayoutParameters {
    uint32_t seed;
    uint32_t maxIterationCount;
    double tolerance;
    double gravity;
    double initialStep;
};

struct LayoutResult {
    uint32_t iterationCount = 0;
    double step = 0.;
    double energy = 0.;
};

// Bit of *inputError (nothing was computed where it is not 0).
constexpr uint32_t kLayoutEdgeRange = 1u;           // an edge end >= vertexCount

// The layout of the graph of vertexCount > 0 vertices and the edges (d_edge0[e], d_edge1[e]) in device memory: initial
// positions from (seed, vertex), then Hu's adaptive iteration until maxIterationCount or step < tolerance.  d_x / d_y
// [vertexCount] in device memory receive the positions.  Every edge end is checked before anything indexes with it.
// Takes its scratch from the cache of em2_scratch.h; synchronises the stream.
hipError_t runGraphLayout(uint32_t vertexCount, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount,
                          const LayoutParameters& parameters, float* d_x, float* d_y, LayoutResult& result, uint32_t* inputError,
                          hipStream_t stream);

// One evaluation of the forces at the positions d_x / d_y, no move: d_fx / d_fy [vertexCount], *energy = the sum of |f|^2.
hipError_t runGraphLayoutForces(uint32_t vertexCount, const uint32_t* d_edge0, const uint32_t* d_edge1, uint64_t edgeCount, double gravity,
                                const float* d_x, const float* d_y, float* d_fx, float* d_fy, double* energy, uint32_t* inputError,
                                hipStream_t stream);

}  // namespace em2

#endif
