// em2_pie_host.cpp -- the host half of the signature graph's picture: the order std::sort gives pairs under
// OrderPairsBySecondGreater, colorRandom through <random>, the value table of colorByMetaDataInterpretedAsCategory around the
// device's census (em2_pie.hip), the boundary vectors of the pie raster, and SignatureGraph::writeSvg
// (src/SignatureGraph.cpp:183-321) byte for byte through a C++ ostream.
#include "em2_host.h"
#include "em2_meta_data.h"
#include "em2_pie.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <limits>
#include <memory>
#include <new>
#include <random>
#include <string>
#include <utility>
#include <vector>

// Defined in em2_capi.hip.
extern "C" void em2_internal_set_last_error(const char* message);

namespace {

const double kPi = 3.141592653589793238462643383279502884;        // boost::math::constants::pi<double>()

int failWith(int code, const std::string& message)
{
    em2_internal_set_last_error(message.c_str());
    return code;
}

[[noreturn]] void fail(int code, const std::string& message)
{
    em2::host::Error e;
    e.code = code;
    e.message = message;
    throw e;
}

// src/orderPairs.hpp:56-62.
template <class Pair> class OrderPairsBySecondGreater {
public:
    bool operator()(const Pair& x, const Pair& y) const { return x.second > y.second; }
};

// The indices as std::sort leaves (index, counts[index]) under that comparator.
void orderByCount(const uint64_t* counts, uint64_t count, std::vector<uint32_t>& order)
{
    std::vector<std::pair<uint32_t, uint64_t>> pairs(static_cast<size_t>(count));
    for (size_t i = 0; i < pairs.size(); ++i) pairs[i] = std::make_pair(uint32_t(i), counts[i]);
    std::sort(pairs.begin(), pairs.end(), OrderPairsBySecondGreater<std::pair<uint32_t, uint64_t>>());
    order.resize(pairs.size());
    for (size_t i = 0; i < pairs.size(); ++i) order[i] = pairs[i].first;
}

// `count` strings, each followed by its NUL, in `bytes` bytes; false where they are not.
bool splitPacked(const char* packed, uint64_t bytes, uint64_t count, std::vector<std::string>& out)
{
    out.clear();
    uint64_t at = 0;
    while (at < bytes && out.size() < count) {
        const void* end = std::memchr(packed + at, 0, size_t(bytes - at));
        if (!end) return false;
        const uint64_t length = uint64_t(static_cast<const char*>(end) - (packed + at));
        out.emplace_back(packed + at, size_t(length));
        at += length + 1u;
    }
    return out.size() == count && at == bytes;
}

}  // namespace

namespace em2 {
namespace host {

void Matrix::pieCensus(uint32_t vertexCount, const uint64_t* cellOffsets, const uint32_t* cells, uint64_t cellCount,
                       const uint32_t* globalCellIds, uint32_t cellSetSize, const std::string& metaDataName, em2_pie_census** census) const
{
    const char* who = "em2_matrix_pie_census";
    *census = nullptr;
    for (uint32_t v = 0; v < vertexCount; ++v) {
        if (cellOffsets[v] > cellOffsets[v + 1u] || cellOffsets[v + 1u] > cellCount) {
            fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": the cell offsets do not ascend within cellCount");
        }
    }
    const uint64_t keptBegin = vertexCount ? cellOffsets[0] : 0u, keptEnd = vertexCount ? cellOffsets[vertexCount] : 0u;

    // One raw value id per cell of the cell set.  The reference hands out "" both for a cell without the field and for a stored
    // "", and for every cell where the store does not know the field's name (:204, getCellMetaData(CellId, StringId)): one id.
    const MetaDataStore& store = *metaData_;
    const uint32_t nameId = store.present ? store.names.find(metaDataName) : kInvalidStringId;
    const uint32_t storedEmpty = store.present ? store.values.find("") : kInvalidStringId;
    std::vector<uint32_t> raw(cellSetSize);
    for (uint32_t i = 0; i < cellSetSize; ++i) {
        checkCellId(who, globalCellIds[i]);
        uint32_t valueId = kInvalidStringId;
        if (nameId != kInvalidStringId) {
            const uint64_t node = store.firstNode(globalCellIds[i], nameId);
            if (node != MetaDataStore::kNoNode) valueId = store.nodes[size_t(node)].valueId;
        }
        if (valueId == kInvalidStringId) valueId = storedEmpty;
        else if (valueId >= store.values.size()) store.values.get(valueId);           // (throws: damaged)
        raw[i] = valueId;
    }
    // The distinct raw ids as strings, ascending: the order of the reference's std::map<string, CellId>.  The compact id of a
    // value is its position there.
    std::vector<uint32_t> distinct(raw);
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    std::vector<std::pair<std::string, uint32_t>> named(distinct.size());
    for (size_t d = 0; d < distinct.size(); ++d) {
        named[d] = std::make_pair(distinct[d] == kInvalidStringId ? std::string() : store.values.get(distinct[d]), distinct[d]);
    }
    std::sort(named.begin(), named.end());
    std::vector<uint32_t> position(distinct.size());
    for (size_t d = 0; d < named.size(); ++d) {
        position[size_t(std::lower_bound(distinct.begin(), distinct.end(), named[d].second) - distinct.begin())] = uint32_t(d);
    }
    std::vector<uint32_t> idOfCell(cellSetSize);
    for (uint32_t i = 0; i < cellSetSize; ++i) {
        idOfCell[i] = position[size_t(std::lower_bound(distinct.begin(), distinct.end(), raw[i]) - distinct.begin())];
    }
    const uint32_t valueCount = uint32_t(named.size());

    // The cells of each value over the cells of the vertices (:205-216), counted on the device: a table of one column.
    std::vector<uint64_t> cellsOfValue(valueCount, 0u);
    if (keptEnd > keptBegin) {
        std::vector<uint32_t> keptIds(size_t(keptEnd - keptBegin)), zeros(size_t(keptEnd - keptBegin), 0u);
        for (uint64_t i = keptBegin; i < keptEnd; ++i) {
            if (cells[i] >= cellSetSize) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": a vertex's cell is not below cellSetSize");
            keptIds[size_t(i - keptBegin)] = idOfCell[cells[i]];
        }
        em2_contingency* table = nullptr;
        const int status = em2_contingency_create(keptIds.data(), zeros.data(), keptIds.size(), valueCount, 1, 0, &table);
        if (status != EM2_OK) fail(status, em2_last_error());
        std::unique_ptr<em2_contingency, void (*)(em2_contingency*)> owner(table, em2_contingency_free);
        em2_contingency_get(table, cellsOfValue.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
    }

    // The values that occur, in map order, through std::sort (:219-220); rank r gets colour index min(r, 12) (:224-227).
    std::vector<uint32_t> occurring;
    std::vector<uint64_t> occurringCells;
    for (uint32_t id = 0; id < valueCount; ++id) {
        if (cellsOfValue[id]) {
            occurring.push_back(id);
            occurringCells.push_back(cellsOfValue[id]);
        }
    }
    std::vector<uint32_t> order;
    orderByCount(occurringCells.data(), occurringCells.size(), order);
    std::vector<uint8_t> colorOfValue(valueCount, uint8_t(0));                         // (a value no vertex holds is never looked up)
    for (size_t rank = 0; rank < order.size(); ++rank) colorOfValue[occurring[order[rank]]] = uint8_t(rank < 12u ? rank : 12u);

    em2_pie_census* made = nullptr;
    const int status = em2_pie_census_create(vertexCount, cellOffsets, cells, cellCount, idOfCell.data(), cellSetSize, colorOfValue.data(),
                                             valueCount, &made);
    if (status != EM2_OK) fail(status, em2_last_error());
    for (size_t rank = 0; rank < order.size(); ++rank) {
        made->result.values.push_back(named[occurring[order[rank]]].first);
        made->result.valueCells.push_back(occurringCells[order[rank]]);
    }
    *census = made;
}

}  // namespace host
}  // namespace em2

extern "C" {

int em2_pie_census_values_sizes(const em2_pie_census* census, uint64_t* valueCount, uint64_t* valueBytes)
{
    if (!census) return failWith(EM2_ERROR_INVALID_ARGUMENT, "em2_pie_census_values_sizes: null pointer");
    uint64_t bytes = 0;
    for (const std::string& value : census->result.values) bytes += value.size() + 1u;
    if (valueCount) *valueCount = census->result.values.size();
    if (valueBytes) *valueBytes = bytes;
    return EM2_OK;
}

int em2_pie_census_values_get(const em2_pie_census* census, char* values, uint64_t* valueCells)
{
    if (!census) return failWith(EM2_ERROR_INVALID_ARGUMENT, "em2_pie_census_values_get: null pointer");
    if (values) {
        char* at = values;
        for (const std::string& value : census->result.values) {
            std::memcpy(at, value.c_str(), value.size() + 1u);
            at += value.size() + 1u;
        }
    }
    if (valueCells) std::copy(census->result.valueCells.begin(), census->result.valueCells.end(), valueCells);
    return EM2_OK;
}

int em2_order_by_count(const uint64_t* counts, uint64_t count, uint32_t* order)
{
    if (count && (!counts || !order)) return failWith(EM2_ERROR_INVALID_ARGUMENT, "em2_order_by_count: null pointer");
    if (count > 0xffffffffull) return failWith(EM2_ERROR_INVALID_ARGUMENT, "em2_order_by_count: count must be below 2^32");
    try {
        std::vector<uint32_t> sorted;
        orderByCount(counts, count, sorted);
        std::copy(sorted.begin(), sorted.end(), order);
    } catch (const std::bad_alloc&) {
        return failWith(EM2_ERROR_RUNTIME, "out of host memory");
    }
    return EM2_OK;
}

int em2_signature_graph_random_colors(uint32_t vertexCount, uint32_t* rgb)
{
    if (vertexCount && !rgb) return failWith(EM2_ERROR_INVALID_ARGUMENT, "em2_signature_graph_random_colors: null pointer");
    const int seed = 231;                                              // :179-181
    std::mt19937 randomGenerator(seed);
    std::uniform_real_distribution<double> distribution(0, 1.);
    for (uint32_t v = 0; v < vertexCount; ++v) {
        double red = distribution(randomGenerator);
        double green = distribution(randomGenerator);
        double blue = distribution(randomGenerator);
        red = std::max(0., std::min(red, 1.));                         // color, src/color.cpp:16-23
        green = std::max(0., std::min(green, 1.));
        blue = std::max(0., std::min(blue, 1.));
        const int r = int(red * 255), g = int(green * 255), b = int(blue * 255);
        rgb[v] = (uint32_t(r) << 16) | (uint32_t(g) << 8) | uint32_t(b);
    }
    return EM2_OK;
}

int em2_pie_boundaries(uint32_t vertexCount, const uint64_t* sliceOffsets, const double* sliceFraction, int32_t* boundaryX,
                       int32_t* boundaryY, uint8_t* largeArc)
{
    const char* who = "em2_pie_boundaries";
    if (vertexCount && !sliceOffsets) return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    for (uint32_t v = 0; v < vertexCount; ++v) {
        if (sliceOffsets[v] > sliceOffsets[v + 1u]) return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": sliceOffsets do not ascend");
    }
    if (vertexCount && sliceOffsets[vertexCount] > sliceOffsets[0] && (!sliceFraction || !boundaryX || !boundaryY || !largeArc)) {
        return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    }
    for (uint32_t v = 0; v < vertexCount; ++v) {
        double totalAngle = 0.;
        for (uint64_t k = sliceOffsets[v]; k < sliceOffsets[v + 1u]; ++k) {
            const double angle = sliceFraction[k] * 2. * kPi;          // src/SignatureGraph.cpp:300-302
            const double angle0 = totalAngle;
            const double angle1 = angle0 + angle;
            // (a fraction that is not finite gives a cosine that is not: llround's result is then unspecified, 0 here)
            const double cx = std::cos(angle0) * 1048576., cy = std::sin(angle0) * 1048576.;
            boundaryX[k] = std::isfinite(cx) ? int32_t(std::llround(cx)) : 0;
            boundaryY[k] = std::isfinite(cy) ? int32_t(std::llround(cy)) : 0;
            largeArc[k] = angle > kPi ? 1 : 0;
            totalAngle = angle1;
        }
    }
    return EM2_OK;
}

int em2_signature_graph_write_svg(const char* fileName, uint32_t vertexCount, const double* x, const double* y, const uint64_t* cellCounts,
                                  uint64_t edgeCount, const uint32_t* v0, const uint32_t* v1, int hideEdges, double svgSizePixels,
                                  double xShift, double yShift, double zoomFactor, double vertexSizeFactor, double edgeThicknessFactor,
                                  const uint64_t* sliceOffsets, const char* sliceColors, uint64_t sliceColorsBytes,
                                  const double* sliceFraction, double* svgParameters)
{
    const char* who = "em2_signature_graph_write_svg";
    if (!fileName || !svgParameters || (vertexCount && (!x || !y || !cellCounts)) || (edgeCount && !hideEdges && (!v0 || !v1))) {
        return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    }
    std::vector<std::string> colors;
    if (sliceOffsets) {
        if (!vertexCount) return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": sliceOffsets without a vertex");
        for (uint32_t v = 0; v < vertexCount; ++v) {
            if (sliceOffsets[v] > sliceOffsets[v + 1u]) return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": sliceOffsets do not ascend");
        }
        const uint64_t sliceCount = sliceOffsets[vertexCount];
        if (sliceOffsets[0] != 0u || (sliceCount && (!sliceColors || !sliceFraction)) ||
            !splitPacked(sliceColors ? sliceColors : "", sliceColorsBytes, sliceCount, colors)) {
            return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": sliceColors does not hold one string per slice");
        }
    }
    for (uint64_t e = 0; !hideEdges && e < edgeCount; ++e) {
        if (v0[e] >= vertexCount || v1[e] >= vertexCount) {
            return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": an edge's vertex is not below vertexCount");
        }
    }

    using std::max;
    using std::min;
    double xMin = std::numeric_limits<double>::max();                  // :194-209
    double xMax = std::numeric_limits<double>::min();
    double yMin = xMin;
    double yMax = xMax;
    uint32_t maxCellCount = 0;                                         // CellId
    for (uint32_t v = 0; v < vertexCount; ++v) {
        xMin = min(xMin, x[v]);
        xMax = max(xMax, x[v]);
        yMin = min(yMin, y[v]);
        yMax = max(yMax, y[v]);
        maxCellCount = max(maxCellCount, uint32_t(cellCounts[v]));
    }
    const double xBoundingBoxCenter = (xMin + xMax) / 2.;              // :212-216
    const double yBoundingBoxCenter = (yMin + yMax) / 2.;
    const double xBoundingBoxSize = xMax - xMin;
    const double yBoundingBoxSize = yMax - yMin;
    const double boundingBoxSize = max(xBoundingBoxSize, yBoundingBoxSize);
    const double xViewBoxCenter = xBoundingBoxCenter - xShift;         // :219-223
    const double yViewBoxCenter = yBoundingBoxCenter - yShift;
    const double viewBoxSize = 1.05 * boundingBoxSize / zoomFactor;
    const double xMinViewBox = xViewBoxCenter - viewBoxSize / 2.;
    const double yMinViewBox = yViewBoxCenter - viewBoxSize / 2.;
    svgParameters[0] = xViewBoxCenter;                                 // :226-229
    svgParameters[1] = yViewBoxCenter;
    svgParameters[2] = viewBoxSize / 2.;
    svgParameters[3] = viewBoxSize / svgSizePixels;

    std::vector<uint32_t> sortedVertices;                              // :234-239
    try {
        orderByCount(cellCounts, vertexCount, sortedVertices);
    } catch (const std::bad_alloc&) {
        return failWith(EM2_ERROR_RUNTIME, "out of host memory");
    }

    std::ofstream s(fileName, std::ios::binary);
    if (!s) return failWith(EM2_ERROR_RUNTIME, std::string(who) + ": cannot open " + fileName + " for writing");
    s << "<svg id=svgObject "
         "style='border:solid DarkBlue;margin:2;' "
         "width='" << svgSizePixels << "' "
         "height='" << svgSizePixels << "' "
         "viewBox='" << xMinViewBox << " " << yMinViewBox << " " << viewBoxSize << " " << viewBoxSize << "'"
         ">";                                                          // :244-250

    if (!hideEdges) {                                                  // :253-268
        s << "<g id=edges>";
        const double unscaledEdgeThickness = 5.e-4 * boundingBoxSize;
        for (uint64_t e = 0; e < edgeCount; ++e) {
            s << "<line x1='" << x[v0[e]] << "' y1='" << y[v0[e]] << "'";
            s << " x2='" << x[v1[e]] << "' y2='" << y[v1[e]] << "'";
            s << " style='stroke:black;stroke-width:" << unscaledEdgeThickness * edgeThicknessFactor << "' />";
        }
        s << "</g>";
    }

    s << "<g id=vertices>";                                            // :274-315
    const double largestVertexUnscaledRadius = 0.03 * boundingBoxSize;
    for (const uint32_t v : sortedVertices) {
        const double vertexRadius = largestVertexUnscaledRadius * std::sqrt(double(cellCounts[v]) / double(maxCellCount));
        const uint64_t first = sliceOffsets ? sliceOffsets[v] : 0u, sliceCount = sliceOffsets ? sliceOffsets[v + 1u] - first : 0u;
        if (sliceCount < 2u) {
            const std::string vertexColor = sliceCount == 0u ? std::string("black") : colors[size_t(first)];
            s << "<circle cx='0' cy='0' r='" << vertexRadius << "' stroke='none' fill='" << vertexColor << "'"
                 " transform='translate(" << x[v] << " " << y[v] << ") scale(" << vertexSizeFactor << ")'"
                 "></circle>";
        } else {
            double totalAngle = 0.;
            for (uint64_t k = first; k < first + sliceCount; ++k) {
                const std::string& color = colors[size_t(k)];
                const double angle = sliceFraction[k] * 2. * kPi;
                const double angle0 = totalAngle;
                const double angle1 = angle0 + angle;
                s << "<path d='M 0 0 L " << vertexRadius * std::cos(angle0) << " " << vertexRadius * std::sin(angle0) << " A "
                  << vertexRadius << " " << vertexRadius << " 0 " << ((angle > kPi) ? 1 : 0) << " 1 "
                  << vertexRadius * std::cos(angle1) << " " << vertexRadius * std::sin(angle1)
                  << " Z' stroke='none' fill='" << color << "'"
                     " transform='translate(" << x[v] << " " << y[v] << ") scale(" << vertexSizeFactor << ")'"
                     "></path>";
                totalAngle = angle1;
            }
        }
    }
    s << "</g>";
    s << "</svg>";
    s.flush();
    if (!s) return failWith(EM2_ERROR_RUNTIME, std::string(who) + ": writing " + fileName + " failed");
    return EM2_OK;
}

}  // extern "C"
