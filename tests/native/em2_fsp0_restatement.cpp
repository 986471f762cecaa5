// em2_fsp0_restatement.cpp -- CPU restatement of ExpressionMatrix::findSimilarPairs0
// (src/ExpressionMatrixFindSimilarPairs.cpp:16-99) and ExpressionMatrix::analyzeSimilarPairs
// (src/ExpressionMatrixLsh.cpp:55-150) on the CSR of an expression matrix subset.  Test infrastructure only: the
// device results are compared with it bit for bit.  Written from the reference's lines cited below, in this
// project's words; compiled by tests/fsp0_binding.py with -ffp-contract=off so that no product and sum fuse.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <fstream>
#include <limits>
#include <random>
#include <utility>
#include <vector>

namespace {

struct Count {          // std::pair<GeneId, float> (src/ExpressionMatrixSubset.hpp:36)
    uint32_t gene;
    float count;
};

struct Sums {
    double sum1 = 0., sum2 = 0.;
};

// ExpressionMatrixSubset::computeSums (src/ExpressionMatrixSubset.cpp:47-58).
std::vector<Sums> computeSums(const uint64_t* toc, const Count* data, uint32_t cellCount)
{
    std::vector<Sums> sums(cellCount);
    for (uint32_t cell = 0; cell < cellCount; cell++) {
        for (uint64_t i = toc[cell]; i < toc[cell + 1]; i++) {
            const float& count = data[i].count;
            sums[cell].sum1 += count;                        // :54
            sums[cell].sum2 += count * count;                // :55, the product is a float
        }
    }
    return sums;
}

// ExpressionMatrixSubset::computeCellSimilarity (src/ExpressionMatrixSubset.cpp:83-133).
double cellSimilarity(const uint64_t* toc, const Count* data, uint32_t geneCount, const std::vector<Sums>& sums, uint32_t cell0,
                      uint32_t cell1)
{
    const Count* it0 = data + toc[cell0];
    const Count* const end0 = data + toc[cell0 + 1];
    const Count* it1 = data + toc[cell1];
    const Count* const end1 = data + toc[cell1 + 1];
    double scalarProduct = 0.;
    while (it0 != end0 && it1 != end1) {                     // :94-107
        if (it0->gene < it1->gene) {
            ++it0;
        } else if (it1->gene < it0->gene) {
            ++it1;
        } else {
            scalarProduct += it0->count * it1->count;        // :103, a float product added to a double
            ++it0;
            ++it1;
        }
    }
    const double n = double(geneCount);                      // :111
    const Sums& a = sums[cell0];
    const Sums& b = sums[cell1];
    const double numerator = n * scalarProduct - a.sum1 * b.sum1;                                        // :114
    const double denominator = std::sqrt((n * a.sum2 - a.sum1 * a.sum1) * (n * b.sum2 - b.sum1 * b.sum1));   // :115-118
    return numerator / denominator;                          // :132
}

typedef std::pair<uint32_t, float> Pair;                     // src/SimilarPairs.hpp:53-56

struct CellInfo {                                            // src/SimilarPairs.cpp:36-40
    uint32_t usedCount = 0;
    uint32_t lowestSimilarityIndex = std::numeric_limits<uint32_t>::max();
    float lowestSimilarity = std::numeric_limits<float>::max();
};

// SimilarPairs::add(CellId, Pair) (src/SimilarPairs.cpp:170-232).  Where the reference would write through
// lowestSimilarityIndex == 0xffffffff (undefined there) the candidate is dropped, as the product documents.
void add(std::vector<Pair>& slots, CellInfo& info, size_t k, Pair pair)
{
    const uint32_t n = info.usedCount;
    if (n < k) {
        for (uint32_t i = 0; i < n; i++) {                   // :179-183
            if (slots[i].first == pair.first) return;
        }
        if (pair.second < info.lowestSimilarity) {           // :185-188
            info.lowestSimilarityIndex = n;
            info.lowestSimilarity = pair.second;
        }
        slots.push_back(pair);                               // :191-192 (slot n)
        ++info.usedCount;
        return;
    }
    if (pair.second <= info.lowestSimilarity) return;        // :203
    for (uint32_t i = 0; i < n; i++) {                       // :209-214
        if (slots[i].first == pair.first) return;
    }
    if (info.lowestSimilarityIndex == std::numeric_limits<uint32_t>::max()) return;
    slots[info.lowestSimilarityIndex] = pair;                // :217
    info.lowestSimilarityIndex = std::numeric_limits<uint32_t>::max();   // :220-228
    info.lowestSimilarity = std::numeric_limits<float>::max();
    for (uint32_t i = 0; i < n; i++) {
        if (slots[i].second < info.lowestSimilarity) {
            info.lowestSimilarityIndex = i;
            info.lowestSimilarity = slots[i].second;
        }
    }
}

// OrderPairsBySecondGreaterThenByFirstLess (src/orderPairs.hpp), used by SimilarPairs::sort (src/SimilarPairs.cpp:399-405).
bool bySimilarityThenId(const Pair& x, const Pair& y)
{
    if (x.second > y.second) return true;
    if (x.second < y.second) return false;
    return x.first < y.first;
}

}  // namespace

extern "C" {

// exact[] receives the similarity of every unordered pair, cell0 ascending, cell1 > cell0 ascending.
void em2r_pair_similarities(const uint64_t* toc, const void* data, uint32_t cellCount, uint32_t geneCount, double* exact)
{
    const Count* counts = static_cast<const Count*>(data);
    const std::vector<Sums> sums = computeSums(toc, counts, cellCount);
    size_t at = 0;
    for (uint32_t cell0 = 0; cell0 + 1 < cellCount; cell0++) {
        for (uint32_t cell1 = cell0 + 1; cell1 < cellCount; cell1++) exact[at++] = cellSimilarity(toc, counts, geneCount, sums, cell0, cell1);
    }
}

double em2r_cell_similarity(const uint64_t* toc, const void* data, uint32_t cellCount, uint32_t geneCount, uint32_t cell0, uint32_t cell1)
{
    const Count* counts = static_cast<const Count*>(data);
    return cellSimilarity(toc, counts, geneCount, computeSums(toc, counts, cellCount), cell0, cell1);
}

// The pair loop of rows [rowBegin, rowEnd) without the container: what a timing of the reference's arithmetic needs.
// Returns the number of pairs above the threshold.
uint64_t em2r_count_similar_pairs_of_rows(const uint64_t* toc, const void* data, uint32_t cellCount, uint32_t geneCount,
                                          uint32_t rowBegin, uint32_t rowEnd, double similarityThreshold)
{
    const Count* counts = static_cast<const Count*>(data);
    const std::vector<Sums> sums = computeSums(toc, counts, cellCount);
    uint64_t found = 0;
    for (uint32_t cell0 = rowBegin; cell0 < rowEnd; cell0++) {
        for (uint32_t cell1 = cell0 + 1; cell1 < cellCount; cell1++) {
            if (cellSimilarity(toc, counts, geneCount, sums, cell0, cell1) > similarityThreshold) ++found;
        }
    }
    return found;
}

// findSimilarPairs0 after its lookups (src/ExpressionMatrixFindSimilarPairs.cpp:57-82).  cell / similarity [cellCount][k]
// (unused slots untouched), usedCount / lowestSimilarityIndex / lowestSimilarity [cellCount].  Returns 1 for
// similarityThreshold > 1 (:26).
int em2r_find_similar_pairs0(const uint64_t* toc, const void* data, uint32_t cellCount, uint32_t geneCount, uint32_t k,
                             double similarityThreshold, uint32_t* cell, float* similarity, uint32_t* usedCount,
                             uint32_t* lowestSimilarityIndex, float* lowestSimilarity)
{
    if (!(similarityThreshold <= 1.)) return 1;
    const Count* counts = static_cast<const Count*>(data);
    const std::vector<Sums> sums = computeSums(toc, counts, cellCount);
    std::vector<std::vector<Pair> > slots(cellCount);
    std::vector<CellInfo> info(cellCount);
    for (uint32_t cell0 = 0; cell0 + 1 < cellCount; cell0++) {                                 // :60
        for (uint32_t cell1 = cell0 + 1; cell1 < cellCount; cell1++) {                         // :66
            const double s = cellSimilarity(toc, counts, geneCount, sums, cell0, cell1);
            if (s > similarityThreshold) {                                                     // :72
                add(slots[cell0], info[cell0], k, Pair(cell1, float(s)));                      // SimilarPairs.cpp:133
                add(slots[cell1], info[cell1], k, Pair(cell0, float(s)));                      // :134
            }
        }
    }
    for (uint32_t c = 0; c < cellCount; c++) {
        std::sort(slots[c].begin(), slots[c].end(), bySimilarityThenId);                       // :82
        for (size_t i = 0; i < slots[c].size(); i++) {
            cell[size_t(c) * k + i] = slots[c][i].first;
            similarity[size_t(c) * k + i] = slots[c][i].second;
        }
        usedCount[c] = info[c].usedCount;
        lowestSimilarityIndex[c] = info[c].lowestSimilarityIndex;
        lowestSimilarity[c] = info[c].lowestSimilarity;
    }
    return 0;
}

// The same for the rows [rowBegin, rowEnd) only: cell / similarity [rowEnd - rowBegin][k] and the three per-row arrays
// are indexed by row - rowBegin.  In the loop above cell c is offered (c1, s) for c1 < c while c is the inner index and
// then for c1 > c while it is the outer one, i.e. its candidates in ascending id of the other cell, and add() touches
// the state of that one cell only: the cells are independent, so a row's list is what its candidates in that order
// leave.  cellSimilarity is called with the smaller id first, as above.  Returns 1 for similarityThreshold > 1, 2 for a
// range that is not within the cells.
int em2r_find_similar_pairs0_rows(const uint64_t* toc, const void* data, uint32_t cellCount, uint32_t geneCount, uint32_t rowBegin,
                                  uint32_t rowEnd, uint32_t k, double similarityThreshold, uint32_t* cell, float* similarity,
                                  uint32_t* usedCount, uint32_t* lowestSimilarityIndex, float* lowestSimilarity)
{
    if (!(similarityThreshold <= 1.)) return 1;
    if (rowBegin > rowEnd || rowEnd > cellCount) return 2;
    const Count* counts = static_cast<const Count*>(data);
    const std::vector<Sums> sums = computeSums(toc, counts, cellCount);
    for (uint32_t row = rowBegin; row < rowEnd; row++) {
        std::vector<Pair> slots;
        CellInfo info;
        for (uint32_t other = 0; other < cellCount; other++) {
            if (other == row) continue;
            const double s = cellSimilarity(toc, counts, geneCount, sums, std::min(row, other), std::max(row, other));
            if (s > similarityThreshold) add(slots, info, k, Pair(other, float(s)));
        }
        std::sort(slots.begin(), slots.end(), bySimilarityThenId);
        const size_t at = size_t(row - rowBegin);
        for (size_t i = 0; i < slots.size(); i++) {
            cell[at * k + i] = slots[i].first;
            similarity[at * k + i] = slots[i].second;
        }
        usedCount[at] = info.usedCount;
        lowestSimilarityIndex[at] = info.lowestSimilarityIndex;
        lowestSimilarity[at] = info.lowestSimilarity;
    }
    return 0;
}

// analyzeSimilarPairs after its lookups (src/ExpressionMatrixLsh.cpp:71-148).  Returns 1 where CZI_ASSERT(bin < binCount)
// fires (:111), 2 where a file cannot be opened.
int em2r_analyze_similar_pairs(const uint64_t* toc, const void* data, uint32_t cellCount, uint32_t geneCount, const uint32_t* cell,
                               const float* similarity, const uint32_t* usedCount, uint32_t k, const uint32_t* globalCellIds,
                               double csvDownsample, const char* pairsCsvPath, const char* statisticsCsvPath)
{
    const Count* counts = static_cast<const Count*>(data);
    const std::vector<Sums> sums = computeSums(toc, counts, cellCount);
    std::ofstream csvOut(pairsCsvPath);
    if (!csvOut) return 2;
    csvOut << "GlobalCellId0,GlobalCellId1,ExactSimilarity,StoredSimilarity\n";               // :73
    const size_t binCount = 200;                                                               // :76-80
    const double binWidth = 2. / binCount;
    std::vector<size_t> sum0(binCount, 0);
    std::vector<double> sum1(binCount, 0.), sum2(binCount, 0.);
    std::mt19937 randomSource(231);                              // :84-90: boost::mt19937 is std::mt19937
    const double factor = 1. / (double(std::mt19937::max()) + 1.);   // boost::uniform_01 over a 32-bit engine: value * 2^-32
    for (uint32_t cell0 = 0; cell0 < cellCount; cell0++) {                                     // :95
        for (uint32_t i = 0; i < usedCount[cell0]; i++) {                                      // :100
            const uint32_t cell1 = cell[size_t(cell0) * k + i];
            const float& storedSimilarity = similarity[size_t(cell0) * k + i];
            const double exactSimilarity = cellSimilarity(toc, counts, geneCount, sums, cell0, cell1);
            const double delta = storedSimilarity - exactSimilarity;                           // :109
            // :110-111; size_t(x) is undefined for a NaN, infinite or negative x (a cell without variance gives NaN or
            // +-inf): the assert fires for every value that is not one of the 200 bins, whatever a compiler makes of it
            const double binAsDouble = std::floor((exactSimilarity + 1.) / binWidth);
            if (!(binAsDouble >= 0. && binAsDouble < double(binCount))) return 1;
            const size_t bin = size_t(binAsDouble);
            ++sum0[bin];
            sum1[bin] += delta;
            sum2[bin] += delta * delta;
            if (double(randomSource()) * factor < csvDownsample) {                             // :117
                csvOut << globalCellIds[cell0] << ",";
                csvOut << globalCellIds[cell1] << ",";
                csvOut << exactSimilarity << ",";
                csvOut << storedSimilarity << "\n";
            }
        }
    }
    std::ofstream statsOut(statisticsCsvPath);                                                 // :133-148
    if (!statsOut) return 2;
    statsOut << "Similarity,Bias,Rms\n";
    for (size_t bin = 0; bin < binCount; bin++) {
        if (sum0[bin] < 2) continue;
        const double binSimilarity = (double(bin) + 0.5) * binWidth - 1.;
        const double s0 = double(sum0[bin]);
        statsOut << binSimilarity << ",";
        statsOut << sum1[bin] / s0 << ",";
        statsOut << std::sqrt(sum2[bin] / s0) << "\n";
    }
    return 0;
}

}  // extern "C"
