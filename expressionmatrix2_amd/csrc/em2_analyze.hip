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
#include "em2_entry.h"
#include "em2_csr.h"

#include <cmath>
#include <cstdio>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include "em2_tables.h"

#include <algorithm>

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


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;
using em2::wordCountOf;

namespace {

// Ends an analysis that does not reach its end (an error return): closes the csv, frees the state.
struct AnalysisCloser {
    em2::AnalysisState*& state;
    ~AnalysisCloser() { if (state) em2::analysisEnd(state, 0, nullptr, nullptr, nullptr, nullptr); }
};

}  // namespace

extern "C" {

int em2_analyze_lsh(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount,
                    const uint64_t* signatures, uint32_t lshCount, const uint32_t* globalCellIds, uint32_t seed,
                    double csvDownsample, const char* pairsCsvPath, const char* statisticsCsvPath,
                    uint64_t* sum0, double* sum1, double* sum2, double* exactSimilarity, double* lshSimilarity)
{
    if (lshCount == 0 || geneCount == 0) return fail(EM2_ERROR_INVALID_ARGUMENT, "em2_analyze_lsh: lshCount and geneCount must be positive");
    if (cellCount == 0) return fail(EM2_ERROR_INVALID_ARGUMENT, "em2_analyze_lsh: the cell set is empty");
    if (!toc || !signatures || !globalCellIds || !pairsCsvPath) return failNull("em2_analyze_lsh");
    if (!haveDevice()) return failNoDevice("em2_analyze_lsh");
    const uint64_t nnz = toc[cellCount];
    if (nnz && !data) return fail(EM2_ERROR_INVALID_ARGUMENT, "em2_analyze_lsh: null data");
    for (uint64_t i = 0; i < nnz; ++i) {
        if (data[i].gene >= geneCount) return fail(EM2_ERROR_INVALID_ARGUMENT, "em2_analyze_lsh: a local gene id is not below geneCount");
    }
    const uint32_t words = wordCountOf(lshCount);

    // ExpressionMatrixSubset::computeSums (src/ExpressionMatrixSubset.cpp:47-58)
    std::vector<double> sums(2 * size_t(cellCount), 0.);
    for (uint32_t c = 0; c < cellCount; ++c) {
        double s1 = 0., s2 = 0.;
        for (uint64_t i = toc[c]; i < toc[c + 1]; ++i) {
            const float count = data[i].count;
            s1 += count;
            s2 += count * count;
        }
        sums[2 * size_t(c)] = s1;
        sums[2 * size_t(c) + 1] = s2;
    }

    em2::AnalysisState* state = em2::analyzeLshBegin(lshCount, seed, pairsCsvPath);
    if (!state) return fail(EM2_ERROR_RUNTIME, std::string("em2_analyze_lsh: cannot open ") + pairsCsvPath);
    AnalysisCloser closer{state};

    // rows in chunks of about 16M pairs: 192 MB of device output per chunk, walked by the host in order
    const uint64_t chunkPairs = 1ull << 24;
    const auto chunkEnd = [&](uint32_t begin, uint64_t& pairs) {
        uint32_t end = begin;
        for (pairs = 0; end + 1 < cellCount && (end == begin || pairs + (cellCount - 1 - end) <= chunkPairs);) pairs += cellCount - 1 - end++;
        return end;
    };
    uint32_t maxRows = 0;
    uint64_t maxPairs = 0, pairs = 0;
    for (uint32_t begin = 0; begin + 1 < cellCount;) {
        const uint32_t end = chunkEnd(begin, pairs);
        if (end - begin > maxRows) maxRows = end - begin;
        if (pairs > maxPairs) maxPairs = pairs;
        begin = end;
    }
    em2::UploadedCsr csr;
    (void)csr.check(toc, reinterpret_cast<const em2::CountIn*>(data), cellCount, false);      // (null data was refused above)
    EM2_HIP(csr.upload());
    DeviceBuffer dSig, dProducts, dMismatches, dScratch;
    EM2_HIP(dSig.upload(signatures, size_t(cellCount) * words));
    EM2_HIP(dProducts.allocateFor<double>(maxPairs));
    EM2_HIP(dMismatches.allocateFor<uint32_t>(maxPairs));
    EM2_HIP(dScratch.allocate(em2::analyzeScratchBytes(geneCount, maxRows)));
    std::vector<double> products(maxPairs);
    std::vector<uint32_t> mismatches(maxPairs);
    uint64_t done = 0;
    for (uint32_t begin = 0; begin + 1 < cellCount;) {
        const uint32_t end = chunkEnd(begin, pairs);
        EM2_HIP(em2::launchAnalyzePairs(csr.toc.as<uint64_t>(), csr.data.as<em2::CountIn>(), cellCount, geneCount, dSig.as<uint64_t>(), words,
                                        begin, end, dScratch.p, dProducts.as<double>(), dMismatches.as<uint32_t>(), nullptr));
        EM2_HIP(hipStreamSynchronize(nullptr));
        EM2_HIP(dProducts.download(products.data(), pairs));
        EM2_HIP(dMismatches.download(mismatches.data(), pairs));
        if (!em2::analyzeLshRows(state, sums.data(), cellCount, geneCount, globalCellIds, begin, end, products.data(), mismatches.data(),
                                 csvDownsample, exactSimilarity ? exactSimilarity + done : nullptr,
                                 lshSimilarity ? lshSimilarity + done : nullptr)) {
            return fail(EM2_ERROR_RUNTIME, "em2_analyze_lsh: Assertion failed: bin < binCount (a pair of cells with exact similarity 1, or a "
                                           "cell without variance; src/ExpressionMatrixLsh.cpp:1322)");
        }
        done += pairs;
        begin = end;
    }
    em2::AnalysisState* finished = state;
    state = nullptr;
    if (!em2::analysisEnd(finished, lshCount, statisticsCsvPath, sum0, sum1, sum2)) {
        return fail(EM2_ERROR_RUNTIME, std::string("em2_analyze_lsh: cannot write ") + (statisticsCsvPath ? statisticsCsvPath : ""));
    }
    return EM2_OK;
}


// ExpressionMatrix::analyzeSimilarPairs (src/ExpressionMatrixLsh.cpp:55-150) after its lookups: the exact similarity of every
// stored pair on the device, chunk of rows by chunk of rows; bins, the seeded draw and the csv lines on the host in the
// reference's order (cell 0 ascending, stored order).
int em2_analyze_similar_pairs(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount,
                              const em2_pair* pairs, const uint32_t* usedCount, uint32_t k, const uint32_t* globalCellIds,
                              double csvDownsample, const char* pairsCsvPath, const char* statisticsCsvPath,
                              uint64_t* sum0, double* sum1, double* sum2)
{
    const char* who = "em2_analyze_similar_pairs";
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (!toc || !usedCount || !globalCellIds || !pairsCsvPath || !statisticsCsvPath || (!pairs && k && cellCount)) return failNull(who);
    em2::UploadedCsr csr;
    if (const char* error = csr.check(toc, reinterpret_cast<const em2::CountIn*>(data), cellCount)) return failArgument(who, error);
    if (cellCount && toc[0] != 0) return failArgument(who, "toc must start at 0");
    uint64_t stored = 0;
    for (uint32_t c = 0; c < cellCount; ++c) {
        if (usedCount[c] > k) return failArgument(who, "a cell stores more than k pairs");
        for (uint32_t t = 0; t < usedCount[c]; ++t) {
            if (pairs[size_t(c) * k + t].cell >= cellCount) return failArgument(who, "a stored pair names a cell that does not exist");
        }
        stored += usedCount[c];
    }
    if (stored && !haveDevice()) return failNoDevice(who);

    em2::AnalysisState* state = em2::analyzeStoredBegin(pairsCsvPath);
    if (!state) return fail(EM2_ERROR_RUNTIME, std::string(who) + ": cannot open " + pairsCsvPath);
    AnalysisCloser closer{state};

    if (stored) {
        // rows in chunks of at most 2^24 slots (128 MB of doubles), one row at least
        const uint32_t chunkRows = std::max<uint32_t>(1u, uint32_t(std::min<uint64_t>(cellCount, (1ull << 24) / k)));
        const em2::PairOut* hostPairs = reinterpret_cast<const em2::PairOut*>(pairs);
        DeviceBuffer dPairs, dUsed, dWorkspace, dExact;
        EM2_HIP(csr.upload());
        EM2_HIP(dPairs.upload(pairs, size_t(cellCount) * k));
        EM2_HIP(dUsed.upload(usedCount, cellCount));
        EM2_HIP(dWorkspace.allocate(em2::storedPairsWorkspaceBytes(cellCount, chunkRows, geneCount)));
        EM2_HIP(dExact.allocateFor<double>(size_t(chunkRows) * k));
        uint32_t inputError = 0;
        EM2_HIP(em2::prepareStoredPairs(csr.toc.as<uint64_t>(), csr.data.as<em2::CountIn>(), cellCount, geneCount, dWorkspace.p, &inputError, nullptr));
        if (inputError) return failArgument(who, em2::inputErrorText(inputError));
        std::vector<double> exact(size_t(chunkRows) * k);
        for (uint32_t begin = 0; begin < cellCount; begin += chunkRows) {
            const uint32_t end = uint32_t(std::min<uint64_t>(cellCount, uint64_t(begin) + chunkRows));
            EM2_HIP(em2::launchStoredPairs(csr.toc.as<uint64_t>(), csr.data.as<em2::CountIn>(), cellCount, geneCount, begin, end,
                                           dPairs.as<em2::PairOut>(), dUsed.as<uint32_t>(), k, dWorkspace.p, dExact.as<double>(), nullptr));
            EM2_HIP(hipStreamSynchronize(nullptr));
            EM2_HIP(dExact.download(exact.data(), size_t(end - begin) * k));
            if (!em2::analyzeStoredRows(state, hostPairs, usedCount, k, globalCellIds, begin, end, exact.data(), csvDownsample)) {
                return fail(EM2_ERROR_RUNTIME, std::string(who) + ": Assertion failed: bin < binCount (a stored pair with exact "
                                               "similarity 1 or not finite; src/ExpressionMatrixLsh.cpp:111)");
            }
        }
    }
    em2::AnalysisState* finished = state;
    state = nullptr;
    if (!em2::analysisEnd(finished, 0, statisticsCsvPath, sum0, sum1, sum2)) {
        return fail(EM2_ERROR_RUNTIME, std::string(who) + ": cannot open " + statisticsCsvPath);
    }
    return EM2_OK;
}

}  // extern "C"
