// em2_analyze.hip -- ExpressionMatrix::analyzeLsh (src/ExpressionMatrixLsh.cpp:1244-1367): every unordered pair of
// cells of an expression matrix subset, its exact similarity (ExpressionMatrixSubset::computeCellSimilarity,
// src/ExpressionMatrixSubset.cpp:83-133) against its LSH similarity (Lsh::computeCellSimilarity, src/Lsh.cpp:254-265).
//
// The reference's loop is serial in two ways that define its output: the bins accumulate doubles in pair order
// (:1323-1325), and the csv is downsampled by one draw of a seeded mt19937 per pair, in pair order (:1329).  What is
// O(pairs x counts per cell) -- the sparse scalar product of each pair (:86-108) and the mismatch count of its two
// signatures -- is done here on the device, bit for bit as the reference does it: the products are float products, the
// sum a double sum in ascending gene order.  What is O(pairs) and order-defined -- correlation coefficient from the
// scalar product, bins, the random draw, the csv lines -- stays with the host (analyzeLshHost below), which walks the
// pairs in the reference's order over the device's output, chunk of rows by chunk of rows.
//
// Device layout: a block per row cell i (in the global-memory form the blocks stride over the rows).  The counts of cell i
// are scattered into em2_expression.h's dense row vector; thread t then takes the cells j = i + 1 + t, i + 1 + t + 256, ...
// and walks cell j's counts once: for the genes both cells have, in ascending gene order, scalarProduct += count_i *
// count_j -- the pairs the reference's two-pointer merge visits, in the same order.
//
// The host half of ExpressionMatrix::analyzeSimilarPairs (src/ExpressionMatrixLsh.cpp:55-150) is here too: the same bins.

#include "em2_device.h"
#include "em2_expression.h"

#include <cmath>
#include <cstdio>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "em2_tables.h"

namespace em2 {
namespace {

template <bool IN_LDS>
__global__ void __launch_bounds__(256)
analyzePairsKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint32_t cellCount, uint32_t geneCount,
                   const uint64_t* __restrict__ sig, uint32_t words, uint32_t rowBegin, uint32_t rowEnd,
                   double* __restrict__ scalarProducts, uint32_t* __restrict__ mismatches, char* rowScratch)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldsRaw[];
    const RowVector rowVector = rowVectorOf<IN_LDS>(ldsRaw, rowScratch, geneCount);
    const uint64_t belowBegin = uint64_t(rowBegin) * (uint64_t(rowBegin) + 1u) / 2u - uint64_t(rowBegin);
    for (uint32_t i = rowBegin + blockIdx.x; i < rowEnd; i += gridDim.x) {
        loadRow(rowVector, geneCount, toc, data, i);
        // pairs of row i start at this offset of the chunk's output: rows rowBegin .. i-1 have cellCount - 1 - r pairs each
        const uint64_t below = uint64_t(i) * (uint64_t(i) + 1u) / 2u - uint64_t(i);          // 0 + 1 + ... + (i - 1)
        const uint64_t offset = uint64_t(i - rowBegin) * uint64_t(cellCount - 1u) - (below - belowBegin);
        const uint64_t* sig0 = sig + size_t(i) * words;
        for (uint32_t j = i + 1u + threadIdx.x; j < cellCount; j += blockDim.x) {
            const double scalarProduct = scalarProductWithRow(rowVector, toc, data, j);
            const uint64_t* sig1 = sig + size_t(j) * words;
            uint32_t m = 0;
            for (uint32_t w = 0; w < words; ++w) m += uint32_t(__builtin_popcountll(sig0[w] ^ sig1[w]));
            const uint64_t at = offset + (j - i - 1u);
            scalarProducts[at] = scalarProduct;
            mismatches[at] = m;
        }
        __syncthreads();
    }
}

}  // namespace


uint64_t analyzePairCount(uint32_t cellCount, uint32_t rowBegin, uint32_t rowEnd)
{
    uint64_t n = 0;
    for (uint32_t r = rowBegin; r < rowEnd; ++r) n += uint64_t(cellCount - 1u - r);
    return n;
}

size_t analyzeScratchBytes(uint32_t geneCount, uint32_t rowCount)
{
    return rowFitsLds(geneCount) ? 0 : rowScratchBytes(geneCount, rowCount);
}

// Rows [rowBegin, rowEnd) against the cells above them; scalarProducts / mismatches hold analyzePairCount entries, row
// by row, within a row by ascending second cell.  scratch: analyzeScratchBytes(geneCount, rowEnd - rowBegin).
hipError_t launchAnalyzePairs(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount,
                              const uint64_t* signatures, uint32_t words, uint32_t rowBegin, uint32_t rowEnd, void* scratch,
                              double* scalarProducts, uint32_t* mismatches, hipStream_t stream)
{
    if (rowEnd <= rowBegin) return hipSuccess;
    return launchRowKernel(rowFitsLds(geneCount), &analyzePairsKernel<true>, &analyzePairsKernel<false>, rowEnd - rowBegin, 256u,
                           geneCount, 0u, scratch, stream, toc, data, cellCount, geneCount, signatures, words, rowBegin, rowEnd,
                           scalarProducts, mismatches);
}


// ---- The host halves: everything of ExpressionMatrixLsh.cpp:1286-1364 (analyzeLsh) and :73-148 (analyzeSimilarPairs)
// ---- that is defined by the order of the pairs.  Both keep the same 200 bins and draw from the same kind of engine.

struct AnalysisState {
    static constexpr size_t binCount = 200;                           // :1297, :76
    uint64_t sum0[binCount] = {};
    double sum1[binCount] = {}, sum2[binCount] = {};
    std::mt19937 randomSource;                                        // boost::mt19937 has std::mt19937's parameters
    std::ofstream csvOut;
    std::vector<double> similarityTable;                              // analyzeLsh only

    static double binWidth() { return 2. / double(binCount); }

    // False where the reference's CZI_ASSERT(bin < binCount) throws (:1322, :111).  The reference converts the floor to size_t
    // first, which is undefined for NaN, +-inf (a cell without variance) and negative values: here the assert fires for every
    // value that is not one of the bins, whatever a compiler makes of that conversion.
    bool add(double exactSimilarity, double delta)
    {
        const double binAsDouble = std::floor((exactSimilarity + 1.) / binWidth());
        if (!(binAsDouble >= 0. && binAsDouble < double(binCount))) return false;
        const size_t bin = size_t(binAsDouble);
        ++sum0[bin];
        sum1[bin] += delta;
        sum2[bin] += delta * delta;
        return true;
    }

    // One draw per pair, in pair order: whether the pair goes into the csv (:1329, :115).
    bool draw(double csvDownsample)
    {
        const double factor = 1.0 / (double(0xffffffffu) + 1.0);      // boost::uniform_01 over a 32-bit engine: eng() * 2^-32
        return double(randomSource()) * factor < csvDownsample;
    }
};

static AnalysisState* analysisBegin(uint32_t seed, const char* pairsCsvPath, const char* header)
{
    AnalysisState* s = new AnalysisState;
    s->randomSource.seed(seed);
    s->csvOut.open(pairsCsvPath);
    if (!s->csvOut) {
        delete s;
        return nullptr;
    }
    s->csvOut << header;
    return s;
}

AnalysisState* analyzeLshBegin(uint32_t lshCount, uint32_t seed, const char* pairsCsvPath)
{
    AnalysisState* s = analysisBegin(seed, pairsCsvPath, "LocalCellId0,LocalCellId1,GlobalCellId0,GlobalCellId1,ExactSimilarity,LshSimilarity\n");
    if (s) {
        s->similarityTable.resize(size_t(lshCount) + 1);
        computeSimilarityTable(lshCount, s->similarityTable.data());
    }
    return s;
}

AnalysisState* analyzeStoredBegin(const char* pairsCsvPath)
{
    return analysisBegin(231, pairsCsvPath, "GlobalCellId0,GlobalCellId1,ExactSimilarity,StoredSimilarity\n");      // :84, :73
}

// The pairs of rows [rowBegin, rowEnd), in order.  Returns false where the bin assert throws.
bool analyzeLshRows(AnalysisState* s, const double* sums, uint32_t cellCount, uint32_t geneCount, const uint32_t* globalCellIds,
                    uint32_t rowBegin, uint32_t rowEnd, const double* scalarProducts, const uint32_t* mismatches, double csvDownsample,
                    double* exactOut, double* lshOut)
{
    const double n = double(geneCount);
    size_t at = 0;
    for (uint32_t localCellId0 = rowBegin; localCellId0 < rowEnd; localCellId0++) {
        const double s10 = sums[2 * size_t(localCellId0)], s20 = sums[2 * size_t(localCellId0) + 1];
        for (uint32_t localCellId1 = localCellId0 + 1; localCellId1 < cellCount; localCellId1++, at++) {
            const double s11 = sums[2 * size_t(localCellId1)], s21 = sums[2 * size_t(localCellId1) + 1];
            const double numerator = n * scalarProducts[at] - s10 * s11;                                  // ExpressionMatrixSubset.cpp:118
            const double denominator = std::sqrt((n * s20 - s10 * s10) * (n * s21 - s11 * s11));
            const double exactSimilarity = numerator / denominator;
            const double lshSimilarity = s->similarityTable[mismatches[at]];
            if (!s->add(exactSimilarity, lshSimilarity - exactSimilarity)) return false;
            if (exactOut) exactOut[at] = exactSimilarity;
            if (lshOut) lshOut[at] = lshSimilarity;
            if (s->draw(csvDownsample)) {
                s->csvOut << localCellId0 << ",";
                s->csvOut << localCellId1 << ",";
                s->csvOut << globalCellIds[localCellId0] << ",";
                s->csvOut << globalCellIds[localCellId1] << ",";
                s->csvOut << exactSimilarity << ",";
                s->csvOut << lshSimilarity << ",\n";
            }
        }
    }
    return true;
}

// The stored pairs of rows [rowBegin, rowEnd), cell 0 ascending, in stored order (:95-125); exact[(row - rowBegin) * k + t]
// their exact similarities.  Returns false where the bin assert throws.
bool analyzeStoredRows(AnalysisState* s, const PairOut* pairs, const uint32_t* usedCount, uint32_t k, const uint32_t* globalCellIds,
                       uint32_t rowBegin, uint32_t rowEnd, const double* exact, double csvDownsample)
{
    for (uint32_t localCellId0 = rowBegin; localCellId0 < rowEnd; ++localCellId0) {
        for (uint32_t t = 0; t < usedCount[localCellId0]; ++t) {
            const PairOut& p = pairs[size_t(localCellId0) * k + t];
            const float storedSimilarity = p.similarity;
            const double exactSimilarity = exact[size_t(localCellId0 - rowBegin) * k + t];
            if (!s->add(exactSimilarity, storedSimilarity - exactSimilarity)) return false;
            if (s->draw(csvDownsample)) {
                s->csvOut << globalCellIds[localCellId0] << ",";
                s->csvOut << globalCellIds[p.cell] << ",";
                s->csvOut << exactSimilarity << ",";
                s->csvOut << storedSimilarity << "\n";
            }
        }
    }
    return true;
}

// The statistics csv (:1345-1364 with the RmsTheory column for lshCount > 0, :133-148 without it for lshCount == 0;
// statisticsCsvPath NULL: none) and the bins.  Returns false where the file cannot be opened.  Deletes the state.
bool analysisEnd(AnalysisState* s, uint32_t lshCount, const char* statisticsCsvPath, uint64_t* sum0, double* sum1, double* sum2)
{
    s->csvOut.close();
    bool ok = true;
    if (statisticsCsvPath) {
        std::ofstream statsOut(statisticsCsvPath);
        ok = bool(statsOut);
        statsOut << (lshCount ? "Similarity,Bias,Rms,RmsTheory\n" : "Similarity,Bias,Rms\n");
        for (size_t bin = 0; bin < AnalysisState::binCount; bin++) {
            if (s->sum0[bin] < 2) continue;
            const double similarity = (double(bin) + 0.5) * AnalysisState::binWidth() - 1.;
            const double s0 = double(s->sum0[bin]);
            const double average = s->sum1[bin] / s0;
            const double sigma = std::sqrt(s->sum2[bin] / s0);
            statsOut << similarity << ",";
            statsOut << average << ",";
            if (!lshCount) {
                statsOut << sigma << "\n";
                continue;
            }
            const double pi = 3.141592653589793238462643383279502884;      // boost::math::double_constants::pi
            const double sinTheta = std::sqrt(1. - similarity * similarity);
            const double theta = std::acos(similarity);
            const double p = 1. - theta / pi;
            const double theoreticalSigma = pi * sinTheta * std::sqrt(p * (1. - p) / double(lshCount));
            statsOut << sigma << ",";
            statsOut << theoreticalSigma << "\n";
        }
    }
    for (size_t bin = 0; bin < AnalysisState::binCount; bin++) {
        if (sum0) sum0[bin] = s->sum0[bin];
        if (sum1) sum1[bin] = s->sum1[bin];
        if (sum2) sum2[bin] = s->sum2[bin];
    }
    delete s;
    return ok;
}

}  // namespace em2
