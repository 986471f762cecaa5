// em2_graph_compare_host.h -- the host ends of em2_graph_compare.hip (no HIP, header only, so that a stand-alone program
// can run them under a sanitizer): the merge of the two lists of histogram bins of compareCellGraphs, the fold of a group
// contingency table over its diagonal, and the greedy colouring of CellGraph::assignColorsToGroups (src/CellGraph.cpp:794-862).
#ifndef EM2_GRAPH_COMPARE_HOST_H
#define EM2_GRAPH_COMPARE_HOST_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace em2 {

constexpr int kCompareTableRadius = 2048;                       // the LDS table holds the bins r in [-2048, 2048]
constexpr uint32_t kCompareTableBins = 2u * kCompareTableRadius + 1u;

inline uint32_t floatBits(float x)
{
    uint32_t bits;
    memcpy(&bits, &x, sizeof(bits));
    return bits;
}

inline float floatOfBits(uint32_t bits)
{
    float x;
    memcpy(&x, &bits, sizeof(x));
    return x;
}

// The bins of the similarity difference, ascending by delta, from
//   table [kCompareTableBins]     the number of common edges with std::round(delta / 0.01f) == i - kCompareTableRadius;
//   listDelta / listCount         the bins of the products that went through the sorted list, ascending, no NaN, the two zeros
//                                 as +0 (this function gives the zero bin its sign back);
//   zeroNegative                  the first common edge of the zero bin, in key order, has the product -0.
// A table bin's delta is 0.01f * float(r), the product the kernel's edges formed (one float multiplication: correctly rounded,
// whoever forms it).  Equal deltas from the two lists are one bin.
inline void mergeCompareBins(const uint64_t* table, const std::vector<float>& listDelta, const std::vector<uint64_t>& listCount,
                             bool zeroNegative, std::vector<float>& binDelta, std::vector<uint64_t>& binCount)
{
    binDelta.clear();
    binCount.clear();
    const auto push = [&](float delta, uint64_t count) {
        if (!binDelta.empty() && binDelta.back() == delta) binCount.back() += count;
        else {
            binDelta.push_back(delta);
            binCount.push_back(count);
        }
    };
    size_t at = 0;                                               // of the list
    for (uint32_t i = 0; i < kCompareTableBins; i++) {
        if (!table || table[i] == 0u) continue;
        const float delta = 0.01f * float(int(i) - kCompareTableRadius);
        for (; at < listDelta.size() && listDelta[at] < delta; at++) push(listDelta[at], listCount[at]);
        push(delta, table[i]);
    }
    for (; at < listDelta.size(); at++) push(listDelta[at], listCount[at]);
    for (float& delta : binDelta) {
        if (delta == 0.0f) delta = floatOfBits(zeroNegative ? 0x80000000u : 0u);
    }
}

// The group graph from the sparse contingency table of (group of vertex 0, group of vertex 1) over the edges -- cells
// (i0, i1, count) ascending by (i0, i1) --: the cells off the diagonal folded over it, as pairs g0 < g1 ascending by
// (g0, g1), with the number of edges between the two groups.
inline void foldGroupPairs(const std::vector<uint32_t>& i0, const std::vector<uint32_t>& i1, const std::vector<uint64_t>& count,
                           std::vector<uint32_t>& pair0, std::vector<uint32_t>& pair1, std::vector<uint64_t>& pairEdges)
{
    struct Cell {
        uint32_t low, high;
        uint64_t count;
    };
    std::vector<Cell> cells;
    for (size_t c = 0; c < count.size(); c++) {
        if (i0[c] == i1[c]) continue;
        cells.push_back(Cell{std::min(i0[c], i1[c]), std::max(i0[c], i1[c]), count[c]});
    }
    std::sort(cells.begin(), cells.end(), [](const Cell& a, const Cell& b) { return a.low != b.low ? a.low < b.low : a.high < b.high; });
    pair0.clear();
    pair1.clear();
    pairEdges.clear();
    for (const Cell& cell : cells) {
        if (!pair0.empty() && pair0.back() == cell.low && pair1.back() == cell.high) pairEdges.back() += cell.count;
        else {
            pair0.push_back(cell.low);
            pair1.push_back(cell.high);
            pairEdges.push_back(cell.count);
        }
    }
}

// CellGraph::assignColorsToGroups (src/CellGraph.cpp:830-861) over the group graph's pairs (g0 < g1 < groupCount, distinct):
// the groups ascending; the colours of the adjacent groups with a smaller number, sorted and made unique; the first index c
// with adjacentColors[c] != c, else their number.
inline void assignGroupColors(uint32_t groupCount, const std::vector<uint32_t>& pair0, const std::vector<uint32_t>& pair1,
                              std::vector<uint32_t>& colorTable)
{
    // CSR by the pair's larger group: the smaller neighbours of every group
    std::vector<uint64_t> begin(size_t(groupCount) + 1u, 0u);
    for (size_t p = 0; p < pair1.size(); p++) begin[size_t(pair1[p]) + 1u]++;
    for (size_t g = 0; g < groupCount; g++) begin[g + 1u] += begin[g];
    std::vector<uint32_t> lower(pair0.size());
    std::vector<uint64_t> fill(begin.begin(), begin.end() - 1);
    for (size_t p = 0; p < pair0.size(); p++) lower[fill[pair1[p]]++] = pair0[p];

    colorTable.assign(groupCount, 0u);
    std::vector<uint32_t> adjacentColors;
    for (uint32_t g = 0; g < groupCount; g++) {
        adjacentColors.clear();
        for (uint64_t at = begin[g]; at < begin[g + 1u]; at++) adjacentColors.push_back(colorTable[lower[at]]);
        std::sort(adjacentColors.begin(), adjacentColors.end());
        adjacentColors.erase(std::unique(adjacentColors.begin(), adjacentColors.end()), adjacentColors.end());
        uint32_t color = uint32_t(adjacentColors.size());
        for (uint32_t c = 0; c < adjacentColors.size(); c++) {
            if (adjacentColors[c] != c) {
                color = c;
                break;
            }
        }
        colorTable[g] = color;
    }
}

}  // namespace em2

#endif
