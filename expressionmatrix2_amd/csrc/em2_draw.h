// em2_draw.h -- what the two rasters of a laid-out graph share (em2_draw.hip defines it, em2_pie.hip uses it): the view, the
// one conversion of the coordinates with its checks, and the edge layer.  The definitions are in include/em2_lsh.h.
#ifndef EM2_DRAW_H
#define EM2_DRAW_H

#include "em2_hip_util.h"

namespace em2 {

constexpr uint32_t kMaxSizePixels = 8192;

// the prepare kernel's error word
constexpr uint32_t kBadPosition = 1u;
constexpr uint32_t kBadEdge = 2u;

struct DrawView {
    double xMin, yMin, s256;
    int32_t size;
    int64_t radius;                // R, in 1/256 pixel (em2_graph_draw: one for all vertices)
};

// The checks of a view that need no device (EM2_OK, or the error reported under `who`), and xMin, yMin, s256 and size of the
// view.  The radius is the caller's.
int drawViewOf(const char* who, uint32_t vertexCount, uint64_t edgeCount, uint32_t sizePixels, double xViewBoxCenter, double yViewBoxCenter,
               double viewBoxHalfSize, DrawView& view);

size_t graphDrawWorkspaceBytes(uint32_t vertexCount, uint64_t edgeCount);

// Everything of a raster but its vertices: ux / uy and the checks (*inputError: the prepare kernel's word; the outputs are
// untouched where it is not zero, and nothing else has run), both layers cleared, the edge layer drawn unless hideEdges.
// *ux / *uy point into the workspace.  Synchronises the stream once, after the checks.
hipError_t runGraphDrawBase(uint32_t vertexCount, const double* d_x, const double* d_y, uint64_t edgeCount, const uint32_t* d_v0,
                            const uint32_t* d_v1, bool hideEdges, const DrawView& view, uint32_t* d_vertexTop, uint32_t* d_edgeHits,
                            void* workspace, uint32_t* inputError, const int32_t** ux, const int32_t** uy, StageTimer& timer,
                            hipStream_t stream);

}  // namespace em2

#endif
