// em2_gene_information_restatement.cpp -- ExpressionMatrix::computeGeneInformationContent restated for one thread, line by line:
//   src/ExpressionMatrix.cpp:241-263     addCell: sum1, sum2, norm1Inverse, norm2Inverse of a whole cell
//   src/ExpressionMatrix.cpp:1035-1046   getCellExpressionCount: the binary search per (gene, cell)
//   src/ExpressionMatrix.cpp:1968-2018   the float scaling, the sequential double sums, the host's log
//   src/ExpressionMatrixGeneSets.cpp:336-350   the cells expressing a gene (stored zeros included)
// The CSR is a subset's (local gene ids, ascending within a cell); the norm inverses are given per cell (those of the whole
// cell), NULL for NormalizationMethod::none.  Test infrastructure only.
// Build: g++ -std=c++17 -O2 -msse4.2 -ffp-contract=off -fPIC -shared (tests/gene_information_binding.py).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

struct Count {
    uint32_t gene;
    float count;
};

// getCellExpressionCount (:1035-1046): lower_bound on the gene id alone; 0 where the cell does not store the gene.
float cellExpressionCount(const uint64_t* toc, const Count* data, uint32_t cell, uint32_t gene)
{
    const Count* begin = data + toc[cell];
    const Count* end = data + toc[cell + 1];
    const Count* it = std::lower_bound(begin, end, gene, [](const Count& x, uint32_t g) { return x.gene < g; });
    if (it == end || it->gene != gene) return 0.f;
    return it->count;
}

}  // namespace

extern "C" {

// addCell (:241-263) over the stored order of every cell.
int em2r_cell_norm_inverses(const uint64_t* toc, const Count* data, uint32_t cellCount, double* norm1Inverse, double* norm2Inverse)
{
    for (uint32_t cell = 0; cell < cellCount; ++cell) {
        double sum1 = 0., sum2 = 0.;
        for (uint64_t p = toc[cell]; p < toc[cell + 1]; ++p) {
            const float value = data[p].count;
            sum1 += value;
            sum2 += value * value;
        }
        const double norm2 = std::sqrt(sum2);
        norm1Inverse[cell] = 1. / sum1;
        norm2Inverse[cell] = 1. / norm2;
    }
    return 0;
}

// The genes [geneBegin, geneEnd): informationContent, informationContentDouble, sum, expressingCellCount, positiveCount are
// indexed from geneBegin.  *seconds: the wall time of the loop.
int em2r_gene_information_content(const uint64_t* toc, const Count* data, uint32_t cellCount, uint32_t geneBegin, uint32_t geneEnd,
                                  const double* normInverse, float* informationContent, double* informationContentDouble, double* sums,
                                  uint32_t* expressingCellCount, uint32_t* positiveCount, double* seconds)
{
    const auto start = std::chrono::steady_clock::now();
    std::vector<float> count;
    for (uint32_t gene = geneBegin; gene < geneEnd; ++gene) {
        count.clear();
        count.reserve(cellCount);
        uint32_t expressing = 0, positive = 0;
        for (uint32_t cell = 0; cell < cellCount; ++cell) {
            float c = cellExpressionCount(toc, data, cell, gene);
            if (normInverse) c *= float(normInverse[cell]);               // :1983-1988
            count.push_back(c);
            const Count* begin = data + toc[cell];
            const Count* end = data + toc[cell + 1];
            const Count* it = std::lower_bound(begin, end, gene, [](const Count& x, uint32_t g) { return x.gene < g; });
            if (it != end && it->gene == gene) ++expressing;
            if (c > 0.) ++positive;
        }
        double sum = 0.;                                                    // :1998-2001
        for (const float c : count) sum += double(c);
        double information = std::log(double(cellCount));                   // :2004
        const double inverseSum = 1. / sum;
        for (const float c : count) {
            if (c > 0.) {
                const double p = c * inverseSum;
                information += p * std::log(p);
            }
        }
        information /= std::log(2.);                                        // :2015
        const uint32_t at = gene - geneBegin;
        informationContent[at] = float(information);
        informationContentDouble[at] = information;
        sums[at] = sum;
        expressingCellCount[at] = expressing;
        positiveCount[at] = positive;
    }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    return 0;
}

}  // extern "C"
