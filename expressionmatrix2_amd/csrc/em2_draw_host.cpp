// em2_draw_host.cpp -- the host half of drawing a graph: CellGraph::writeSvg (src/CellGraph.cpp:301-439) byte
// for byte, through a C++ ostream so that the numbers are formatted by the library as the reference's are (precision 6, the
// default float field), and the number a meta data value stands for when the page colours by it
// (src/ExpressionMatrixHttpServerGraphs.cpp:949-964).
#include "../../include/em2_lsh.h"

#include <cerrno>
#include <cfloat>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

// Defined in em2_capi.hip.
extern "C" void em2_internal_set_last_error(const char* message);

namespace {

int failWith(int code, const std::string& message)
{
    em2_internal_set_last_error(message.c_str());
    return code;
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

extern "C" {

int em2_graph_write_svg(const char* fileName, uint32_t vertexCount, const double* x, const double* y, const uint32_t* cellIds,
                        uint64_t edgeCount, const uint32_t* v0, const uint32_t* v1, int hideEdges, double svgSizePixels,
                        double xViewBoxCenter, double yViewBoxCenter, double viewBoxHalfSize, double vertexRadius, double edgeThickness,
                        const char* vertexColors, uint64_t vertexColorsBytes, const uint32_t* vertexGroups, uint32_t groupColorCount,
                        const int32_t* groupColorGroups, const char* groupColors, uint64_t groupColorsBytes, const char* geneSetName)
{
    const char* who = "em2_graph_write_svg";
    if (!fileName || !geneSetName || (vertexCount && (!x || !y || !cellIds)) || (edgeCount && !hideEdges && (!v0 || !v1)) ||
        (groupColorCount && (!groupColorGroups || !groupColors || (vertexCount && !vertexGroups)))) {
        return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    }
    std::vector<std::string> colors, groupColorStrings;
    if (vertexColors && !splitPacked(vertexColors, vertexColorsBytes, vertexCount, colors)) {
        return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": vertexColors does not hold one string per vertex");
    }
    if (groupColorCount && !splitPacked(groupColors, groupColorsBytes, groupColorCount, groupColorStrings)) {
        return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": groupColors does not hold groupColorCount strings");
    }
    for (uint64_t e = 0; !hideEdges && e < edgeCount; ++e) {
        if (v0[e] >= vertexCount || v1[e] >= vertexCount) {
            return failWith(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": an edge's vertex is not below vertexCount");
        }
    }
    std::map<int, std::string> colorMap;                               // std::map<int, string> groupColors, :310
    for (uint32_t g = 0; g < groupColorCount; ++g) colorMap.insert(std::make_pair(int(groupColorGroups[g]), groupColorStrings[g]));

    std::ofstream s(fileName, std::ios::binary);
    if (!s) return failWith(EM2_ERROR_RUNTIME, std::string(who) + ": cannot open " + fileName + " for writing");

    s << "<p><svg id=graphSvg width='" << svgSizePixels << "' height='" << svgSizePixels << "' viewBox='"
      << xViewBoxCenter - viewBoxHalfSize << " " << yViewBoxCenter - viewBoxHalfSize << " " << 2. * viewBoxHalfSize << " "
      << 2. * viewBoxHalfSize << "'>";                                 // :319-324

    if (!hideEdges) {                                                  // :330-357; no edge has a colour of its own here
        s << "<g id=edges>";
        for (uint64_t e = 0; e < edgeCount; ++e) {
            s << "<line x1='" << x[v0[e]] << "' y1='" << y[v0[e]] << "'";
            s << " x2='" << x[v1[e]] << "' y2='" << y[v1[e]] << "'";
            s << " style='stroke:black;stroke-width:" << edgeThickness << "' />";
        }
        s << "</g>";
    }

    if (colorMap.empty()) {                                            // :365-384
        s << "<g id=vertices><g>";
        for (uint32_t v = 0; v < vertexCount; ++v) {
            s << "<a xlink:href='cell?cellId=" << cellIds[v] << "&geneSetName=" << geneSetName << "'>"
              << "<circle cx='" << x[v] << "' cy='" << y[v] << "' r='" << vertexRadius << "' stroke=none";
            if (vertexColors && !colors[v].empty()) s << " fill='" << colors[v] << "'";
            s << "><title>Cell " << cellIds[v] << "</title></circle></a>";
        }
        s << "</g></g>";
    } else {                                                           // :389-437
        std::vector<std::vector<uint32_t>> groups;
        for (uint32_t v = 0; v < vertexCount; ++v) {
            const size_t group = vertexGroups[v];
            if (groups.size() <= group) groups.resize(group + 1);
            groups[group].push_back(v);
        }
        s << "<g id=vertices>";
        for (int iGroup = 0; iGroup < int(groups.size()); iGroup++) {
            const auto it = colorMap.find(iGroup);
            const std::string groupColor = it == colorMap.end() ? "black" : it->second;
            s << "<g id=vertexGroup" << iGroup << " style='fill:" << groupColor << "'>";
            for (const uint32_t v : groups[iGroup]) {
                s << "<a xlink:href='cell?cellId=" << cellIds[v] << "&geneSetName=" << geneSetName << "'>"
                  << "<circle cx='" << x[v] << "' cy='" << y[v] << "' r='" << vertexRadius << "' stroke=none>"
                  << "<title>Cell " << cellIds[v] << "</title></circle></a>";
            }
            s << "</g>";
        }
        s << "</g>";
    }
    s.flush();
    if (!s) return failWith(EM2_ERROR_RUNTIME, std::string(who) + ": writing " + fileName + " failed");
    return EM2_OK;
}

int em2_meta_data_number(const char* value, uint64_t bytes, double* number)
{
    if (!number || (!value && bytes)) return failWith(EM2_ERROR_INVALID_ARGUMENT, "em2_meta_data_number: null pointer");
    *number = DBL_MAX;                                                 // "no value", :954
    const std::string text(value ? value : "", size_t(bytes));
    if (text.empty() || std::memchr(text.data(), 0, text.size())) return EM2_OK;
    const unsigned char first = static_cast<unsigned char>(text[0]);
    if (first == ' ' || (first >= '\t' && first <= '\r')) return EM2_OK;      // strtod would skip it
    char* end = nullptr;
    const double parsed = std::strtod(text.c_str(), &end);
    if (end != text.c_str() + text.size()) return EM2_OK;              // not the whole string
    *number = parsed;
    return EM2_OK;
}

}  // extern "C"
