// em2_pie.h -- the result object of the colour census, which em2_pie.hip fills on the device and em2_pie_host.cpp completes
// with the value table of a meta data field (the definitions are in include/em2_lsh.h).
#ifndef EM2_PIE_H
#define EM2_PIE_H

#include <stdint.h>

#include <string>
#include <vector>

namespace em2 {

// The slices of every vertex in host memory, a CSR over the vertices, and, from the em2_matrix_ form only, the values of the
// field in the order that gave them their colours.
struct PieCensusResult {
    uint32_t vertexCount = 0;
    uint32_t longVertexCount = 0;                  // the vertices a wave worked
    std::vector<uint64_t> sliceOffsets;            // [vertexCount + 1]
    std::vector<uint8_t> sliceColor;
    std::vector<uint32_t> sliceCells;
    std::vector<double> sliceFraction;
    std::vector<std::string> values;               // sorted as the reference sorts them: rank r has colour index min(r, 12)
    std::vector<uint64_t> valueCells;
};

}  // namespace em2

struct em2_pie_census {
    em2::PieCensusResult result;
};

#endif
