// em2_ingest_restatement.cpp -- the storing part of ExpressionMatrix::addCell (src/ExpressionMatrix.cpp:241-277) and the
// per-barcode loop of addCellsFromHdf5 (src/ExpressionMatrixHdf5.cpp:145-183), restated with the reference's types
// (std::vector<std::pair<uint32_t, float>>, std::sort on the pairs, double sums in input order) for the tests of the ingest
// kernels.  Test infrastructure only; compiled on demand with the oracle's flags (-O3 -msse4.2 -ffp-contract=off).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

namespace {

struct Cell {                           // src/Cell.hpp; the last two members are written as 0 by the code under test
    double sum1, sum2, norm2, norm1Inverse, norm2Inverse, sum1Large, sum2Large;
};

struct Negative {};
struct Duplicate {
    uint32_t gene;
};

// :241-277 with the gene ids already looked up.  `stored` is the cell's vector in cellExpressionCounts.
Cell storeCell(const std::vector<std::pair<uint32_t, float>>& expressionCounts, std::vector<std::pair<uint32_t, float>>& stored)
{
    Cell cell;
    std::memset(&cell, 0, sizeof(cell));
    cell.sum1 = 0.;
    cell.sum2 = 0.;
    stored.clear();
    for (const auto& p : expressionCounts) {
        const float value = p.second;
        if (value < 0.) throw Negative();
        if (value == 0.) continue;
        cell.sum1 += value;
        cell.sum2 += value * value;
        stored.push_back(std::make_pair(p.first, value));
    }
    cell.norm2 = std::sqrt(cell.sum2);
    cell.norm1Inverse = 1. / cell.sum1;
    cell.norm2Inverse = 1. / cell.norm2;
    std::sort(stored.begin(), stored.end());
    for (size_t i = 1; i < stored.size(); i++) {
        if (stored[i - 1].first == stored[i].first) throw Duplicate{stored[i].first};
    }
    return cell;
}

}  // namespace

extern "C" {

// Every barcode of a sparse matrix.  keptCount[i]: the values of the row that are not zero (whatever becomes of the cell);
// status 0 ok, 1 negative, 2 duplicate with its gene (0xffffffff otherwise); toc: the exclusive sums of keptCount; data at
// toc[i] and cells[i] are written for the rows that are stored, skipped rows and rows that throw leave theirs untouched.
void em2r_ingest_csr(const uint64_t* indptr, const uint32_t* indices, const float* values, const uint8_t* skip, uint32_t cellCount,
                     const uint32_t* geneIdOfIndex, uint32_t* keptCount, uint32_t* status, uint32_t* duplicateGene, uint64_t* toc,
                     uint64_t* data, Cell* cells)
{
    std::vector<std::pair<uint32_t, float>> expressionCounts, stored;
    toc[0] = 0;
    for (uint32_t i = 0; i < cellCount; i++) {
        keptCount[i] = 0;
        status[i] = 0;
        duplicateGene[i] = 0xffffffffu;
        toc[i + 1] = toc[i];
        if (skip && skip[i]) continue;                                        // :177-179
        expressionCounts.clear();
        for (uint64_t j = indptr[i]; j < indptr[i + 1]; j++) {                // :168-174
            expressionCounts.push_back(std::make_pair(geneIdOfIndex[indices[j]], values[j]));
            if (values[j] != 0.) keptCount[i]++;
        }
        toc[i + 1] = toc[i] + keptCount[i];
        try {
            const Cell cell = storeCell(expressionCounts, stored);
            static_assert(sizeof(std::pair<uint32_t, float>) == 8, "a stored entry is 8 bytes");
            if (!stored.empty()) std::memcpy(data + toc[i], stored.data(), stored.size() * 8u);
            cells[i] = cell;
        } catch (const Negative&) {
            status[i] = 1;
        } catch (const Duplicate& d) {
            status[i] = 2;
            duplicateGene[i] = d.gene;
        }
    }
}

}  // extern "C"
