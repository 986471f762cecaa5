// em2_draw_restatement.cpp -- one thread and plain loops for what csrc/em2_cell_values.hip, em2_draw.hip and em2_draw_host.cpp
// compute (include/em2_lsh.h, "Colouring and drawing a laid-out graph"): the two values per cell, the colours from numbers, the
// raster and its composition, and the SVG text.  Written from the definitions, with none of the library's code: the
// similarity is the merge loop, the raster tests every step of every edge against the image, the vertices every pixel of a
// clipped box.  Test infrastructure only; built with -ffp-contract=off.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstdint>
#include <fstream>
#include <map>
#include <string>
#include <vector>

namespace {

struct Count {
    uint32_t gene;
    float count;
};

const uint32_t kInvalid = 0xffffffffu;

uint32_t localOf(const uint32_t* localIds, uint32_t globalGeneCount, uint32_t gene)
{
    if (!localIds) return gene;
    return gene < globalGeneCount ? localIds[gene] : kInvalid;
}

int64_t floorDiv(int64_t a, int64_t b)
{
    int64_t q = a / b;
    if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
    return q;
}

}  // namespace

extern "C" {

void em2r_cell_similarities(const uint64_t* toc, const Count* data, const uint32_t* localIds, uint32_t globalGeneCount, uint32_t geneCount,
                            uint32_t cellId0, const uint32_t* cellIds, uint32_t count, double* out)
{
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t cellId1 = cellIds[i];
        const Count *begin0 = data + toc[cellId0], *end0 = data + toc[cellId0 + 1];
        const Count *begin1 = data + toc[cellId1], *end1 = data + toc[cellId1 + 1];
        double sum01 = 0.;
        const Count *it0 = begin0, *it1 = begin1;
        while (it0 != end0 && it1 != end1) {
            if (it0->gene < it1->gene) {
                ++it0;
            } else if (it1->gene < it0->gene) {
                ++it1;
            } else {
                if (localOf(localIds, globalGeneCount, it0->gene) != kInvalid) sum01 += it0->count * it1->count;
                ++it0;
                ++it1;
            }
        }
        double sum0 = 0., sum00 = 0., sum1 = 0., sum11 = 0.;
        for (const Count* it = begin0; it != end0; ++it) {
            if (localOf(localIds, globalGeneCount, it->gene) == kInvalid) continue;
            sum0 += it->count;
            sum00 += it->count * it->count;
        }
        for (const Count* it = begin1; it != end1; ++it) {
            if (localOf(localIds, globalGeneCount, it->gene) == kInvalid) continue;
            sum1 += it->count;
            sum11 += it->count * it->count;
        }
        const double n = double(geneCount);
        const double numerator = n * sum01 - sum0 * sum1;
        const double denominator = std::sqrt((n * sum00 - sum0 * sum0) * (n * sum11 - sum1 * sum1));
        out[i] = numerator / denominator;
    }
}

// 1: the gene is not in the gene set.
int em2r_gene_expression(const uint64_t* toc, const Count* data, const uint32_t* localIds, uint32_t globalGeneCount, uint32_t globalGeneId,
                         int method, const uint32_t* cellIds, uint32_t count, float* out)
{
    const uint32_t localGene = localOf(localIds, globalGeneCount, globalGeneId);
    if (localGene == kInvalid) return 1;
    std::vector<std::pair<uint32_t, float>> expressionVector;
    for (uint32_t i = 0; i < count; ++i) {
        expressionVector.clear();
        for (uint64_t p = toc[cellIds[i]]; p < toc[cellIds[i] + 1]; ++p) {
            const uint32_t local = localOf(localIds, globalGeneCount, data[p].gene);
            if (local != kInvalid) expressionVector.push_back(std::make_pair(local, data[p].count));
        }
        float factor = 1.f;
        double sum = 0.;
        if (method == 1) {
            for (const auto& p : expressionVector) sum += p.second;
            factor = float(1. / sum);
        } else if (method == 2) {
            for (const auto& p : expressionVector) sum += p.second * p.second;
            factor = float(1. / std::sqrt(sum));
        }
        for (auto& p : expressionVector) p.second *= factor;
        float value = 0.f;
        for (const auto& p : expressionVector) {
            if (p.first == localGene) {
                value = p.second;
                break;
            }
        }
        out[i] = value;
    }
    return 0;
}

void em2r_spectral_colors(const double* values, uint64_t count, double minColorValue, double maxColorValue, int haveMin, int haveMax,
                          uint32_t* rgb, double* range)
{
    double minValue = DBL_MAX, maxValue = -DBL_MAX;
    for (uint64_t i = 0; i < count; ++i) {
        const double value = values[i];
        if (value == DBL_MAX) continue;
        if (value < minValue) minValue = value;
        if (maxValue < value) maxValue = value;
    }
    if (!haveMin) minColorValue = minValue;
    if (!haveMax) maxColorValue = maxValue;
    range[0] = minValue;
    range[1] = maxValue;
    range[2] = minColorValue;
    range[3] = maxColorValue;
    if (minValue == maxValue || maxValue == -DBL_MAX) {
        for (uint64_t i = 0; i < count; ++i) rgb[i] = 0x40000000u;
        return;
    }
    const double scalingFactor = 1. / (maxColorValue - minColorValue);
    for (uint64_t i = 0; i < count; ++i) {
        if (values[i] == DBL_MAX) {
            rgb[i] = 0x80000000u;
            continue;
        }
        const double x = scalingFactor * (values[i] - minColorValue);
        double red, green;
        if (x <= 0.) {
            red = 1.;
            green = 0.;
        } else if (x <= 0.5) {
            red = 1.;
            green = 2. * x;
        } else if (x < 1.) {
            red = 2. * (1. - x);
            green = 1.;
        } else {
            red = 0.;
            green = 1.;
        }
        red = std::max(0., std::min(red, 1.));
        green = std::max(0., std::min(green, 1.));
        rgb[i] = (uint32_t(int(red * 255)) << 16) | (uint32_t(int(green * 255)) << 8);
    }
}

// 1: an argument error, nothing written.
int em2r_graph_draw(uint32_t vertexCount, const double* x, const double* y, uint64_t edgeCount, const uint32_t* v0, const uint32_t* v1,
                    int hideEdges, uint32_t sizePixels, double xCenter, double yCenter, double halfSize, double vertexRadius,
                    uint32_t* vertexTop, uint32_t* edgeHits)
{
    if (sizePixels < 1 || sizePixels > 8192 || !std::isfinite(halfSize) || halfSize <= 0.) return 1;
    const int64_t S = sizePixels;
    const double xMin = xCenter - halfSize, yMin = yCenter - halfSize;
    const double s256 = double(S) * 256. / (2. * halfSize);
    if (!(vertexRadius * s256 >= 0.) || vertexRadius * s256 > 256. * 256.) return 1;
    const int64_t R = std::llround(vertexRadius * s256);
    std::vector<int64_t> ux(vertexCount), uy(vertexCount);
    const double limit = 1073741824.;
    for (uint32_t v = 0; v < vertexCount; ++v) {
        if (!std::isfinite(x[v]) || !std::isfinite(y[v])) return 1;
        ux[v] = int64_t(std::max(-limit, std::min(limit, std::floor((x[v] - xMin) * s256))));
        uy[v] = int64_t(std::max(-limit, std::min(limit, std::floor((y[v] - yMin) * s256))));
    }
    for (uint64_t e = 0; e < edgeCount; ++e) {
        if (v0[e] >= vertexCount || v1[e] >= vertexCount) return 1;
    }
    for (int64_t p = 0; p < S * S; ++p) vertexTop[p] = edgeHits[p] = 0;
    for (uint32_t v = 0; v < vertexCount; ++v) {
        const int64_t ownI = floorDiv(ux[v], 256), ownJ = floorDiv(uy[v], 256);
        const int64_t reach = R / 256 + 2;
        for (int64_t j = std::max<int64_t>(0, ownJ - reach); j <= std::min(S - 1, ownJ + reach); ++j) {
            for (int64_t i = std::max<int64_t>(0, ownI - reach); i <= std::min(S - 1, ownI + reach); ++i) {
                const int64_t dx = 256 * i + 128 - ux[v], dy = 256 * j + 128 - uy[v];
                if (dx * dx + dy * dy <= R * R || (i == ownI && j == ownJ)) vertexTop[j * S + i] = std::max(vertexTop[j * S + i], v + 1u);
            }
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

void em2r_graph_compose(uint32_t sizePixels, const uint32_t* vertexTop, const uint32_t* edgeHits, const uint32_t* vertexRgb, uint32_t edgeShade,
                        uint8_t* rgba)
{
    for (uint64_t p = 0; p < uint64_t(sizePixels) * sizePixels; ++p) {
        uint8_t* pixel = rgba + 4 * p;
        pixel[0] = pixel[1] = pixel[2] = pixel[3] = 255;
        if (edgeHits[p] > 0) {
            const uint64_t shade = std::min<uint64_t>(255, uint64_t(edgeShade) * edgeHits[p]);
            pixel[0] = pixel[1] = pixel[2] = uint8_t(255 - shade);
        }
        if (vertexTop[p] > 0) {
            const uint32_t color = vertexRgb[vertexTop[p] - 1];
            pixel[0] = uint8_t(color >> 16);
            pixel[1] = uint8_t(color >> 8);
            pixel[2] = uint8_t(color);
        }
    }
}

// vertexColors: vertexCount strings, each followed by a 0 byte, or NULL.  groupColorCount == 0: no groups.
int em2r_graph_svg(const char* fileName, uint32_t vertexCount, const double* x, const double* y, const uint32_t* cellIds, uint64_t edgeCount,
                   const uint32_t* v0, const uint32_t* v1, int hideEdges, double svgSizePixels, double xCenter, double yCenter, double halfSize,
                   double vertexRadius, double edgeThickness, const char* vertexColors, const uint32_t* vertexGroups, uint32_t groupColorCount,
                   const int32_t* groupColorGroups, const char* groupColors, const char* geneSetName)
{
    std::ofstream s(fileName, std::ios::binary);
    if (!s) return 1;
    std::vector<std::string> colors;
    for (uint32_t v = 0; vertexColors && v < vertexCount; ++v) {
        colors.push_back(vertexColors);
        vertexColors += colors.back().size() + 1;
    }
    std::map<int, std::string> groupColor;
    for (uint32_t g = 0; g < groupColorCount; ++g) {
        groupColor[groupColorGroups[g]] = groupColors;
        groupColors += groupColor[groupColorGroups[g]].size() + 1;
    }
    s << "<p><svg id=graphSvg width='" << svgSizePixels << "' height='" << svgSizePixels << "' viewBox='" << xCenter - halfSize << " "
      << yCenter - halfSize << " " << 2. * halfSize << " " << 2. * halfSize << "'>";
    if (!hideEdges) {
        s << "<g id=edges>";
        for (uint64_t e = 0; e < edgeCount; ++e) {
            s << "<line x1='" << x[v0[e]] << "' y1='" << y[v0[e]] << "' x2='" << x[v1[e]] << "' y2='" << y[v1[e]]
              << "' style='stroke:black;stroke-width:" << edgeThickness << "' />";
        }
        s << "</g>";
    }
    const auto circle = [&](uint32_t v, const std::string& fill) {
        s << "<a xlink:href='cell?cellId=" << cellIds[v] << "&geneSetName=" << geneSetName << "'><circle cx='" << x[v] << "' cy='" << y[v]
          << "' r='" << vertexRadius << "' stroke=none";
        if (!fill.empty()) s << " fill='" << fill << "'";
        s << "><title>Cell " << cellIds[v] << "</title></circle></a>";
    };
    if (groupColor.empty()) {
        s << "<g id=vertices><g>";
        for (uint32_t v = 0; v < vertexCount; ++v) circle(v, colors.empty() ? std::string() : colors[v]);
        s << "</g></g>";
    } else {
        uint32_t groupCount = 0;
        for (uint32_t v = 0; v < vertexCount; ++v) groupCount = std::max(groupCount, vertexGroups[v] + 1);
        s << "<g id=vertices>";
        for (uint32_t group = 0; group < groupCount; ++group) {
            s << "<g id=vertexGroup" << group << " style='fill:" << (groupColor.count(int(group)) ? groupColor[int(group)] : "black") << "'>";
            for (uint32_t v = 0; v < vertexCount; ++v) {
                if (vertexGroups[v] == group) circle(v, std::string());
            }
            s << "</g>";
        }
        s << "</g>";
    }
    return s.good() ? 0 : 1;
}

}  // extern "C"
