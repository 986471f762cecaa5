// em2_pie_host_main.cpp -- a stand-alone program around the host-only code of the signature graph's picture (the order of
// std::sort under OrderPairsBySecondGreater, the random colours, the boundary vectors, the value table's accessors and the SVG
// writer), for a sanitizer build on the CPU (never loaded into Python, never run on a GPU):
//
//   cd expressionmatrix2_amd/csrc && g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o /tmp/em2_pie_host_main ../../tests/native/em2_pie_host_main.cpp em2_pie_host.cpp -Wl,--unresolved-symbols=ignore-all
//   /tmp/em2_pie_host_main OUTPUT.svg
//
// The census over a store (Matrix::pieCensus) needs the device and is left unresolved: this program never calls it.
#include "../../include/em2_lsh.h"
#include "../../expressionmatrix2_amd/csrc/em2_pie.h"

#include <cstdio>
#include <string>
#include <vector>

static std::string lastError;
extern "C" const char* em2_last_error(void) { return lastError.c_str(); }
extern "C" void em2_internal_set_last_error(const char* message) { lastError = message; }

#define EXPECT(condition)                                                     \
    do {                                                                      \
        if (!(condition)) {                                                   \
            std::printf("FAILED line %d: %s (%s)\n", __LINE__, #condition, lastError.c_str()); \
            return 1;                                                         \
        }                                                                     \
    } while (0)

int main(int argc, char** argv)
{
    if (argc != 2) {
        std::printf("usage: %s OUTPUT.svg\n", argv[0]);
        return 2;
    }
    // 1 000 vertices with few distinct cell counts: std::sort's introsort and its final insertion sort both run
    const uint32_t vertexCount = 1000;
    std::vector<uint64_t> cellCounts(vertexCount);
    std::vector<double> x(vertexCount), y(vertexCount);
    for (uint32_t v = 0; v < vertexCount; ++v) {
        cellCounts[v] = 1u + (v * 2654435761u >> 29);
        x[v] = double(v % 37) - 20.;
        y[v] = double(v / 37) * 0.5;
    }
    std::vector<uint32_t> order(vertexCount);
    EXPECT(em2_order_by_count(cellCounts.data(), vertexCount, order.data()) == EM2_OK);
    for (uint32_t i = 1; i < vertexCount; ++i) EXPECT(cellCounts[order[i - 1]] >= cellCounts[order[i]]);
    EXPECT(em2_order_by_count(nullptr, 0, nullptr) == EM2_OK);
    EXPECT(em2_order_by_count(nullptr, 3, order.data()) == EM2_ERROR_INVALID_ARGUMENT);

    std::vector<uint32_t> rgb(vertexCount);
    EXPECT(em2_signature_graph_random_colors(vertexCount, rgb.data()) == EM2_OK);
    EXPECT(rgb[0] == 0x9a3c22u);
    EXPECT(em2_signature_graph_random_colors(0, nullptr) == EM2_OK);

    // slices: vertex v has 1 + v % 13 slices of equal fractions
    std::vector<uint64_t> sliceOffsets(vertexCount + 1, 0u);
    std::vector<double> fraction;
    std::string colors;
    for (uint32_t v = 0; v < vertexCount; ++v) {
        const uint32_t m = 1u + v % 13u;
        for (uint32_t k = 0; k < m; ++k) {
            fraction.push_back(1. / double(m));
            colors += k % 2u ? "black" : "#00ff00";
            colors.push_back('\0');
        }
        sliceOffsets[v + 1] = sliceOffsets[v] + m;
    }
    std::vector<int32_t> bx(fraction.size()), by(fraction.size());
    std::vector<uint8_t> arc(fraction.size());
    EXPECT(em2_pie_boundaries(vertexCount, sliceOffsets.data(), fraction.data(), bx.data(), by.data(), arc.data()) == EM2_OK);
    EXPECT(bx[0] == 1048576 && by[0] == 0 && arc[0] == 1 && bx[2] == -1048576 && arc[1] == 0);
    fraction[5] = 1e308 * 10.;                                         // not finite: no conversion of such a cosine
    EXPECT(em2_pie_boundaries(vertexCount, sliceOffsets.data(), fraction.data(), bx.data(), by.data(), arc.data()) == EM2_OK);
    fraction[5] = 1. / 3.;
    EXPECT(em2_pie_boundaries(0, nullptr, nullptr, nullptr, nullptr, nullptr) == EM2_OK);

    std::vector<uint32_t> v0, v1;
    for (uint32_t v = 0; v + 1 < vertexCount; v += 3) {
        v0.push_back(v);
        v1.push_back(v + 1);
    }
    double parameters[4];
    EXPECT(em2_signature_graph_write_svg(argv[1], vertexCount, x.data(), y.data(), cellCounts.data(), v0.size(), v0.data(), v1.data(), 0, 500.,
                                         0.5, -0.5, 2., 1.5, 0.5, sliceOffsets.data(), colors.data(), colors.size(), fraction.data(),
                                         parameters) == EM2_OK);
    EXPECT(parameters[2] > 0.);
    EXPECT(em2_signature_graph_write_svg(argv[1], vertexCount, x.data(), y.data(), cellCounts.data(), v0.size(), v0.data(), v1.data(), 1, 500.,
                                         0., 0., 1., 1., 1., nullptr, nullptr, 0, nullptr, parameters) == EM2_OK);
    EXPECT(em2_signature_graph_write_svg(argv[1], 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, 500., 0., 0., 1., 1., 1., nullptr,
                                         nullptr, 0, nullptr, parameters) == EM2_OK);
    // one string short, an edge out of range
    EXPECT(em2_signature_graph_write_svg(argv[1], vertexCount, x.data(), y.data(), cellCounts.data(), 0, nullptr, nullptr, 0, 500., 0., 0., 1.,
                                         1., 1., sliceOffsets.data(), colors.data(), colors.size() - 6, fraction.data(),
                                         parameters) == EM2_ERROR_INVALID_ARGUMENT);
    v1[0] = vertexCount;
    EXPECT(em2_signature_graph_write_svg(argv[1], vertexCount, x.data(), y.data(), cellCounts.data(), v0.size(), v0.data(), v1.data(), 0, 500.,
                                         0., 0., 1., 1., 1., nullptr, nullptr, 0, nullptr, parameters) == EM2_ERROR_INVALID_ARGUMENT);

    em2_pie_census census;
    census.result.values = {"b", "", "a longer value"};
    census.result.valueCells = {5, 5, 1};
    uint64_t valueCount = 0, valueBytes = 0;
    EXPECT(em2_pie_census_values_sizes(&census, &valueCount, &valueBytes) == EM2_OK && valueCount == 3 && valueBytes == 2 + 1 + 15);
    std::vector<char> values(valueBytes);
    std::vector<uint64_t> cells(valueCount);
    EXPECT(em2_pie_census_values_get(&census, values.data(), cells.data()) == EM2_OK && values[0] == 'b' && values[2] == 0 && cells[2] == 1);
    std::printf("ok\n");
    return 0;
}
