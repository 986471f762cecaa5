// The behaviour of ExpressionMatrix::compareCellGraphs (two edge maps keyed by ordered cell pairs, a histogram map keyed by a
// float, set_intersection of the sorted vertex lists) and of CellGraph::assignColorsToGroups (a group graph with set
// adjacency, a greedy colouring in group order), written out with the standard containers on one thread.  Test
// infrastructure only: the tests hold the library's results against this, word for word.
//   g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <iterator>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace {

typedef std::map<std::pair<uint32_t, uint32_t>, float> EdgeMap;

// 0, or 1: a vertex index out of range, 2: an edge from a cell to itself.
int fillEdgeMap(const uint32_t* cells, uint32_t vertexCount, const uint32_t* v0, const uint32_t* v1, const float* similarity,
                uint64_t edgeCount, EdgeMap& edges)
{
    for (uint64_t e = 0; e < edgeCount; e++) {
        if (v0[e] >= vertexCount || v1[e] >= vertexCount) return 1;
    }
    for (uint64_t e = 0; e < edgeCount; e++) {
        uint32_t cellA = cells[v0[e]];
        uint32_t cellB = cells[v1[e]];
        if (cellA == cellB) return 2;
        if (cellB < cellA) std::swap(cellA, cellB);
        edges.insert(std::make_pair(std::make_pair(cellA, cellB), similarity[e]));      // (the first one stays)
    }
    return 0;
}

}  // namespace

extern "C" {

// counts[5]: common vertices, edges of map 0, edges of map 1, common edges, identical common edges.  binDelta / binCount need
// room for min(edgeCount0, edgeCount1) bins; *bins receives their number.  Returns 0, or 1 (a vertex index out of range),
// 2 (an edge from a cell to itself), 3 (the difference of a common edge is not a number: it cannot key the histogram map).
int em2r_gc_compare(const uint32_t* cells0, uint32_t vertexCount0, const uint32_t* v0_0, const uint32_t* v1_0, const float* similarity0,
                    uint64_t edgeCount0, const uint32_t* cells1, uint32_t vertexCount1, const uint32_t* v0_1, const uint32_t* v1_1,
                    const float* similarity1, uint64_t edgeCount1, uint64_t* counts, float* binDelta, uint64_t* binCount, uint64_t* bins)
{
    std::vector<uint32_t> sorted0(cells0, cells0 + vertexCount0), sorted1(cells1, cells1 + vertexCount1);
    std::sort(sorted0.begin(), sorted0.end());
    std::sort(sorted1.begin(), sorted1.end());
    std::vector<uint32_t> commonCells;
    std::set_intersection(sorted0.begin(), sorted0.end(), sorted1.begin(), sorted1.end(), std::back_inserter(commonCells));

    EdgeMap edgeMap0, edgeMap1;
    int status = fillEdgeMap(cells0, vertexCount0, v0_0, v1_0, similarity0, edgeCount0, edgeMap0);
    if (status) return status;
    status = fillEdgeMap(cells1, vertexCount1, v0_1, v1_1, similarity1, edgeCount1, edgeMap1);
    if (status) return status;

    uint64_t commonEdgeCount = 0, commonIdenticalEdgeCount = 0;
    std::map<float, uint64_t> histogram;
    const float binWidth = 0.01f;
    for (const auto& p0 : edgeMap0) {
        const auto it1 = edgeMap1.find(p0.first);
        if (it1 == edgeMap1.end()) continue;
        ++commonEdgeCount;
        const float s0 = p0.second;
        const float s1 = it1->second;
        if (s0 == s1) ++commonIdenticalEdgeCount;
        const float delta = s1 - s0;
        if (delta != delta) return 3;
        const float roundedDelta = binWidth * std::round(delta / binWidth);
        const auto it = histogram.find(roundedDelta);
        if (it == histogram.end()) histogram.insert(std::make_pair(roundedDelta, uint64_t(1)));
        else ++(it->second);
    }
    counts[0] = commonCells.size();
    counts[1] = edgeMap0.size();
    counts[2] = edgeMap1.size();
    counts[3] = commonEdgeCount;
    counts[4] = commonIdenticalEdgeCount;
    uint64_t at = 0;
    for (const auto& p : histogram) {
        binDelta[at] = p.first;
        binCount[at] = p.second;
        at++;
    }
    *bins = at;
    return 0;
}

// colorTable needs room for (largest group + 1) entries, the three pair arrays for edgeCount.  Returns 0, or 1 (a vertex
// index out of range).
int em2r_gc_group_colors(const uint32_t* group, uint32_t vertexCount, const uint32_t* v0, const uint32_t* v1, uint64_t edgeCount,
                         uint32_t* groupCountOut, uint32_t* pair0, uint32_t* pair1, uint64_t* pairEdges, uint64_t* pairCount,
                         uint32_t* colorTableOut)
{
    for (uint64_t e = 0; e < edgeCount; e++) {
        if (v0[e] >= vertexCount || v1[e] >= vertexCount) return 1;
    }
    size_t groupCount = 0;
    for (uint32_t v = 0; v < vertexCount; v++) groupCount = std::max(groupCount, size_t(group[v]) + 1);

    std::vector<std::set<uint32_t> > adjacency(groupCount);
    std::map<std::pair<uint32_t, uint32_t>, uint64_t> edgesBetween;
    for (uint64_t e = 0; e < edgeCount; e++) {
        const uint32_t group0 = group[v0[e]];
        const uint32_t group1 = group[v1[e]];
        if (group0 == group1) continue;
        adjacency[group0].insert(group1);
        adjacency[group1].insert(group0);
        ++edgesBetween[std::make_pair(std::min(group0, group1), std::max(group0, group1))];
    }

    std::vector<uint32_t> colorTable;
    std::vector<uint32_t> adjacentColors;
    for (uint32_t group0 = 0; group0 < groupCount; group0++) {
        adjacentColors.clear();
        for (const uint32_t group1 : adjacency[group0]) {
            if (group1 < group0) adjacentColors.push_back(colorTable[group1]);
        }
        std::sort(adjacentColors.begin(), adjacentColors.end());
        adjacentColors.resize(std::unique(adjacentColors.begin(), adjacentColors.end()) - adjacentColors.begin());
        for (uint32_t color = 0; color < adjacentColors.size(); color++) {
            if (adjacentColors[color] != color) {
                colorTable.push_back(color);
                break;
            }
        }
        if (colorTable.size() == group0) colorTable.push_back(uint32_t(adjacentColors.size()));
    }

    *groupCountOut = uint32_t(groupCount);
    std::copy(colorTable.begin(), colorTable.end(), colorTableOut);
    uint64_t at = 0;
    for (const auto& p : edgesBetween) {
        pair0[at] = p.first.first;
        pair1[at] = p.first.second;
        pairEdges[at] = p.second;
        at++;
    }
    *pairCount = at;
    return 0;
}

}  // extern "C"
