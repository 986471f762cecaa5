// A one-thread restatement of the signature graph's colourings and pictures (include/em2_lsh.h, "Colouring and drawing the
// signature graph"): std::map<string, CellId>, std::sort, <random>, ostream formatting and plain loops over vertices, cells and
// pixels.  It shares no code with the library.  Test infrastructure only; tests/signature_draw_binding.py compiles and loads it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

namespace {

typedef uint32_t CellId;

template <class Pair> class OrderPairsBySecondGreater {
public:
    bool operator()(const Pair& x, const Pair& y) const { return x.second > y.second; }
};

const double pi = 3.141592653589793238462643383279502884;

int64_t floorDiv(int64_t a, int64_t b)
{
    int64_t q = a / b;
    if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
    return q;
}

__int128 cross(int64_t px, int64_t py, int64_t qx, int64_t qy) { return __int128(px) * qy - __int128(py) * qx; }

std::vector<std::string> unpack(const char* packed, uint64_t count)
{
    std::vector<std::string> out;
    const char* at = packed;
    for (uint64_t i = 0; i < count; ++i) {
        out.emplace_back(at);
        at += out.back().size() + 1;
    }
    return out;
}

}  // namespace

extern "C" {

// The vertex's colours as the reference keeps them: a vector of (colour, count as a double) in order of first occurrence, std::sort,
// the sum, the factor.  The outputs have room for 13 slices per vertex.  1: an id out of range, nothing written.
int em2r_census(uint32_t vertexCount, const uint64_t* cellOffsets, const uint32_t* cells, uint64_t cellCount, const uint32_t* idOfCell,
                uint32_t cellSetSize, const uint8_t* colorOfValue, uint32_t valueCount, uint64_t* sliceOffsets, uint8_t* sliceColor,
                uint32_t* sliceCells, double* sliceFraction)
{
    for (uint32_t v = 0; v < vertexCount; ++v) {
        if (cellOffsets[v] > cellOffsets[v + 1] || cellOffsets[v + 1] > cellCount) return 1;
        for (uint64_t i = cellOffsets[v]; i < cellOffsets[v + 1]; ++i) {
            if (cells[i] >= cellSetSize || idOfCell[cells[i]] >= valueCount || colorOfValue[idOfCell[cells[i]]] > 12) return 1;
        }
    }
    uint64_t at = 0;
    for (uint32_t v = 0; v < vertexCount; ++v) {
        sliceOffsets[v] = at;
        std::vector<std::pair<int, double>> colors;
        for (uint64_t i = cellOffsets[v]; i < cellOffsets[v + 1]; ++i) {
            const int color = colorOfValue[idOfCell[cells[i]]];
            bool done = false;
            for (auto& p : colors) {
                if (p.first == color) {
                    ++(p.second);
                    done = true;
                    break;
                }
            }
            if (!done) colors.push_back(std::make_pair(color, 1.));
        }
        std::sort(colors.begin(), colors.end(), OrderPairsBySecondGreater<std::pair<int, double>>());
        double sum = 0;
        for (const auto& p : colors) sum += p.second;
        const double factor = 1. / sum;
        for (auto& p : colors) {
            sliceColor[at] = uint8_t(p.first);
            sliceCells[at] = uint32_t(p.second);
            p.second *= factor;
            sliceFraction[at] = p.second;
            ++at;
        }
    }
    sliceOffsets[vertexCount] = at;
    return 0;
}

// values: one string per cell, each followed by a 0 byte.  The table of the distinct values as the reference makes it: a
// std::map<string, CellId>, copied into a vector, std::sort.  tableOrder[rank] = the value's position in the map (string
// ascending), tableCells[rank] its cells, rankOfCell[i] the rank of cell i's value.  Returns the number of values.
uint64_t em2r_value_table(const char* values, uint64_t cellCount, uint32_t* tableOrder, uint64_t* tableCells, uint32_t* rankOfCell)
{
    const std::vector<std::string> perCell = unpack(values, cellCount);
    std::map<std::string, CellId> metaDataValuesTable;
    for (const std::string& metaDataValue : perCell) {
        const auto it = metaDataValuesTable.find(metaDataValue);
        if (it == metaDataValuesTable.end()) {
            metaDataValuesTable.insert(std::make_pair(metaDataValue, 1));
        } else {
            ++(it->second);
        }
    }
    std::map<std::string, uint32_t> positionInMap;
    for (const auto& p : metaDataValuesTable) {
        const uint32_t position = uint32_t(positionInMap.size());
        positionInMap[p.first] = position;
    }
    std::vector<std::pair<std::string, CellId>> metaDataValues(metaDataValuesTable.begin(), metaDataValuesTable.end());
    std::sort(metaDataValues.begin(), metaDataValues.end(), OrderPairsBySecondGreater<std::pair<std::string, CellId>>());
    std::map<std::string, uint32_t> rankOf;
    for (size_t rank = 0; rank < metaDataValues.size(); ++rank) {
        tableOrder[rank] = positionInMap[metaDataValues[rank].first];
        tableCells[rank] = metaDataValues[rank].second;
        rankOf[metaDataValues[rank].first] = uint32_t(rank);
    }
    for (uint64_t i = 0; i < cellCount; ++i) rankOfCell[i] = rankOf[perCell[i]];
    return metaDataValues.size();
}

void em2r_order_by_count(const uint64_t* counts, uint64_t count, uint32_t* order)
{
    std::vector<std::pair<uint64_t, CellId>> sortedVertices;               // (vertex_descriptor, CellId)
    for (uint64_t v = 0; v < count; ++v) sortedVertices.push_back(std::make_pair(v, CellId(counts[v])));
    std::sort(sortedVertices.begin(), sortedVertices.end(), OrderPairsBySecondGreater<std::pair<uint64_t, CellId>>());
    for (uint64_t i = 0; i < count; ++i) order[i] = uint32_t(sortedVertices[i].first);
}

// draws[3 * vertexCount]: what the distribution gave, for the test of the generator itself.
void em2r_random_colors(uint32_t vertexCount, uint32_t* rgb, double* draws)
{
    std::mt19937 randomGenerator(231);
    std::uniform_real_distribution<double> distribution(0, 1.);
    for (uint32_t v = 0; v < vertexCount; ++v) {
        double c[3];
        for (int k = 0; k < 3; ++k) {
            c[k] = distribution(randomGenerator);
            draws[3 * v + k] = c[k];
            c[k] = std::max(0., std::min(c[k], 1.));
        }
        rgb[v] = (uint32_t(int(c[0] * 255)) << 16) | (uint32_t(int(c[1] * 255)) << 8) | uint32_t(int(c[2] * 255));
    }
}

void em2r_pie_boundaries(uint32_t vertexCount, const uint64_t* sliceOffsets, const double* sliceFraction, int32_t* boundaryX,
                         int32_t* boundaryY, uint8_t* largeArc)
{
    for (uint32_t v = 0; v < vertexCount; ++v) {
        double totalAngle = 0.;
        for (uint64_t k = sliceOffsets[v]; k < sliceOffsets[v + 1]; ++k) {
            const double angle = sliceFraction[k] * 2. * pi;
            boundaryX[k] = int32_t(std::llround(std::cos(totalAngle) * 1048576.));
            boundaryY[k] = int32_t(std::llround(std::sin(totalAngle) * 1048576.));
            largeArc[k] = angle > pi;
            totalAngle = totalAngle + angle;
        }
    }
}

// 1: an argument error, nothing written.
int em2r_graph_draw_pies(uint32_t vertexCount, const double* x, const double* y, const double* radius, uint64_t edgeCount,
                         const uint32_t* v0, const uint32_t* v1, int hideEdges, uint32_t sizePixels, double xCenter, double yCenter,
                         double halfSize, const uint64_t* sliceOffsets, uint64_t sliceCount, const int32_t* boundaryX,
                         const int32_t* boundaryY, const uint8_t* largeArc, uint32_t* vertexTop, uint32_t* sliceTop, uint32_t* edgeHits)
{
    if (sizePixels < 1 || sizePixels > 8192 || !std::isfinite(halfSize) || halfSize <= 0.) return 1;
    const int64_t S = sizePixels;
    const double xMin = xCenter - halfSize, yMin = yCenter - halfSize;
    const double s256 = double(S) * 256. / (2. * halfSize);
    std::vector<int64_t> ux(vertexCount), uy(vertexCount), R(vertexCount);
    const double limit = 1073741824.;
    for (uint32_t v = 0; v < vertexCount; ++v) {
        if (!std::isfinite(x[v]) || !std::isfinite(y[v])) return 1;
        if (!(radius[v] * s256 >= 0.) || radius[v] * s256 > 8192. * 256.) return 1;
        if (!(sliceOffsets[v] < sliceOffsets[v + 1]) || sliceOffsets[v + 1] > sliceCount) return 1;
        ux[v] = int64_t(std::max(-limit, std::min(limit, std::floor((x[v] - xMin) * s256))));
        uy[v] = int64_t(std::max(-limit, std::min(limit, std::floor((y[v] - yMin) * s256))));
        R[v] = std::llround(radius[v] * s256);
    }
    if (vertexCount && (sliceOffsets[0] != 0 || sliceOffsets[vertexCount] != sliceCount)) return 1;
    for (uint64_t e = 0; e < edgeCount; ++e) {
        if (v0[e] >= vertexCount || v1[e] >= vertexCount) return 1;
    }
    for (int64_t p = 0; p < S * S; ++p) vertexTop[p] = sliceTop[p] = edgeHits[p] = 0;
    // the vertices in painter order: a later one paints over what is there
    for (uint32_t v = 0; v < vertexCount; ++v) {
        const int64_t ownI = floorDiv(ux[v], 256), ownJ = floorDiv(uy[v], 256);
        const int64_t reach = R[v] / 256 + 2;
        for (int64_t j = std::max<int64_t>(0, ownJ - reach); j <= std::min(S - 1, ownJ + reach); ++j) {
            for (int64_t i = std::max<int64_t>(0, ownI - reach); i <= std::min(S - 1, ownI + reach); ++i) {
                const int64_t dx = 256 * i + 128 - ux[v], dy = 256 * j + 128 - uy[v];
                if (dx * dx + dy * dy <= R[v] * R[v] || (i == ownI && j == ownJ)) vertexTop[j * S + i] = v + 1;
            }
        }
    }
    for (int64_t j = 0; j < S; ++j) {
        for (int64_t i = 0; i < S; ++i) {
            if (!vertexTop[j * S + i]) continue;
            const uint32_t v = vertexTop[j * S + i] - 1;
            const uint64_t first = sliceOffsets[v], m = sliceOffsets[v + 1] - first;
            const int64_t dx = 256 * i + 128 - ux[v], dy = 256 * j + 128 - uy[v];
            uint64_t slice = 0;
            if (m >= 2 && !(dx == 0 && dy == 0)) {
                slice = m - 1;
                for (uint64_t k = 0; k + 1 < m; ++k) {
                    const int64_t ax = boundaryX[first + k], ay = boundaryY[first + k];
                    const int64_t bx = boundaryX[first + k + 1], by = boundaryY[first + k + 1];
                    bool inside;
                    if (largeArc[first + k]) inside = !(cross(bx, by, dx, dy) >= 0 && cross(dx, dy, ax, ay) > 0);
                    else inside = cross(ax, ay, dx, dy) >= 0 && cross(dx, dy, bx, by) > 0;
                    if (inside) {
                        slice = k;
                        break;
                    }
                }
            }
            sliceTop[j * S + i] = uint32_t(first + slice + 1);
        }
    }
    for (uint64_t e = 0; !hideEdges && e < edgeCount; ++e) {
        const int64_t i0 = floorDiv(ux[v0[e]], 256), j0 = floorDiv(uy[v0[e]], 256);
        const int64_t i1 = floorDiv(ux[v1[e]], 256), j1 = floorDiv(uy[v1[e]], 256);
        const int64_t dx = i1 - i0, dy = j1 - j0;
        const bool majorIsX = std::llabs(dx) >= std::llabs(dy);
        const int64_t dM = majorIsX ? std::llabs(dx) : std::llabs(dy), dm = majorIsX ? std::llabs(dy) : std::llabs(dx);
        const int64_t signM = (majorIsX ? dx : dy) < 0 ? -1 : 1, signm = (majorIsX ? dy : dx) < 0 ? -1 : 1;
        for (int64_t k = 0; k <= dM; ++k) {
            const int64_t major = (majorIsX ? i0 : j0) + signM * k;
            const int64_t minor = (majorIsX ? j0 : i0) + (dM ? signm * floorDiv(2 * k * dm + dM, 2 * dM) : 0);
            const int64_t i = majorIsX ? major : minor, j = majorIsX ? minor : major;
            if (i >= 0 && i < S && j >= 0 && j < S) ++edgeHits[j * S + i];
        }
    }
    return 0;
}

// sliceColors: one string per slice, each followed by a 0 byte; sliceOffsets NULL: no vertex has a colour.
int em2r_signature_graph_svg(const char* fileName, uint32_t vertexCount, const double* x, const double* y, const uint64_t* cellCounts,
                             uint64_t edgeCount, const uint32_t* v0, const uint32_t* v1, int hideEdges, double svgSizePixels, double xShift,
                             double yShift, double zoomFactor, double vertexSizeFactor, double edgeThicknessFactor,
                             const uint64_t* sliceOffsets, const char* sliceColors, const double* sliceFraction, double* svgParameters)
{
    std::ofstream s(fileName);
    if (!s) return 1;
    // vertex.colors of every vertex
    std::vector<std::vector<std::pair<std::string, double>>> colors(vertexCount);
    if (sliceOffsets) {
        const std::vector<std::string> strings = unpack(sliceColors, sliceOffsets[vertexCount]);
        for (uint32_t v = 0; v < vertexCount; ++v) {
            for (uint64_t k = sliceOffsets[v]; k < sliceOffsets[v + 1]; ++k) colors[v].push_back(std::make_pair(strings[k], sliceFraction[k]));
        }
    }
    double xMin = std::numeric_limits<double>::max();
    double xMax = std::numeric_limits<double>::min();
    double yMin = xMin;
    double yMax = xMax;
    CellId maxCellCount = 0;
    for (uint32_t v = 0; v < vertexCount; ++v) {
        xMin = std::min(xMin, x[v]);
        xMax = std::max(xMax, x[v]);
        yMin = std::min(yMin, y[v]);
        yMax = std::max(yMax, y[v]);
        maxCellCount = std::max(maxCellCount, CellId(cellCounts[v]));
    }
    const double boundingBoxSize = std::max(xMax - xMin, yMax - yMin);
    const double xViewBoxCenter = (xMin + xMax) / 2. - xShift;
    const double yViewBoxCenter = (yMin + yMax) / 2. - yShift;
    const double viewBoxSize = 1.05 * boundingBoxSize / zoomFactor;
    svgParameters[0] = xViewBoxCenter;
    svgParameters[1] = yViewBoxCenter;
    svgParameters[2] = viewBoxSize / 2.;
    svgParameters[3] = viewBoxSize / svgSizePixels;

    std::vector<std::pair<uint64_t, CellId>> sortedVertices;
    for (uint32_t v = 0; v < vertexCount; ++v) sortedVertices.push_back(std::make_pair(uint64_t(v), CellId(cellCounts[v])));
    std::sort(sortedVertices.begin(), sortedVertices.end(), OrderPairsBySecondGreater<std::pair<uint64_t, CellId>>());

    s << "<svg id=svgObject style='border:solid DarkBlue;margin:2;' width='" << svgSizePixels << "' height='" << svgSizePixels
      << "' viewBox='" << xViewBoxCenter - viewBoxSize / 2. << " " << yViewBoxCenter - viewBoxSize / 2. << " " << viewBoxSize << " "
      << viewBoxSize << "'>";
    if (!hideEdges) {
        s << "<g id=edges>";
        const double unscaledEdgeThickness = 5.e-4 * boundingBoxSize;
        for (uint64_t e = 0; e < edgeCount; ++e) {
            s << "<line x1='" << x[v0[e]] << "' y1='" << y[v0[e]] << "' x2='" << x[v1[e]] << "' y2='" << y[v1[e]]
              << "' style='stroke:black;stroke-width:" << unscaledEdgeThickness * edgeThicknessFactor << "' />";
        }
        s << "</g>";
    }
    s << "<g id=vertices>";
    const double largestVertexUnscaledRadius = 0.03 * boundingBoxSize;
    for (const auto& p : sortedVertices) {
        const uint64_t v = p.first;
        const double vertexRadius = largestVertexUnscaledRadius * std::sqrt(double(cellCounts[v]) / double(maxCellCount));
        if (colors[v].size() < 2) {
            const std::string vertexColor = colors[v].empty() ? std::string("black") : colors[v].front().first;
            s << "<circle cx='0' cy='0' r='" << vertexRadius << "' stroke='none' fill='" << vertexColor << "' transform='translate(" << x[v]
              << " " << y[v] << ") scale(" << vertexSizeFactor << ")'></circle>";
        } else {
            double totalAngle = 0.;
            for (const auto& c : colors[v]) {
                const double angle = c.second * 2. * pi;
                const double angle0 = totalAngle;
                const double angle1 = angle0 + angle;
                s << "<path d='M 0 0 L " << vertexRadius * std::cos(angle0) << " " << vertexRadius * std::sin(angle0) << " A " << vertexRadius
                  << " " << vertexRadius << " 0 " << ((angle > pi) ? 1 : 0) << " 1 " << vertexRadius * std::cos(angle1) << " "
                  << vertexRadius * std::sin(angle1) << " Z' stroke='none' fill='" << c.first << "' transform='translate(" << x[v] << " "
                  << y[v] << ") scale(" << vertexSizeFactor << ")'></path>";
                totalAngle = angle1;
            }
        }
    }
    s << "</g></svg>";
    s.flush();
    return s ? 0 : 1;
}

}  // extern "C"
